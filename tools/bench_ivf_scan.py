"""The IVF list scan on the device (IVFIndex.scan_device / search_device, vidc_ivf_scan_dev) against the two torch forms it stands
beside, on the same index and the same probes.

Shapes: the reference's (custom_invlist_cpp/bench_invlists.py): 10^6 clustered vectors, IVF1024, PQ16, d = 128, k = 20, nprobe 1 / 4 /
16; and IVF1024,Flat at d = 32.  Batches of 10, 10^3 and 10^4 queries.  Arms, alternating in one process after a warm-up:
  device   scan_device (probes given: the coarse quantiser is outside every arm)
  loop     IVFIndex._scan, the per-query torch loop (nq <= 10^3 only; its probes are its own cdist + topk; results go to the host)
  batch    a padded all-torch batch: the probed lists gathered to a common length, PQ by table lookup, one topk per chunk of queries
           (chunks sized to ~1 GiB of gathered codes) -- the fairest torch form
  search_device / search_defer_id_decoding: end to end over a packed-bits container (nq <= 10^3 for the latter)
Recorded per arm: every wall time (perf_counter around the call, ending in a synchronise), median, minimum, maximum; for the device
arm vidc_ctx_last_kernel_ms, the cut S, the code bytes the probed lists hold and bytes per second of kernel time, next to the copy
rate of torch's own copy kernel (the measurement of tools/bw_calib.py); the kernel time of the same batch with every probe -1 (the
launch, the row handling and, for PQ, the per-item table); agreement of D with the batch arm.  No threshold: every arm is reported,
also where it loses.  Hardware counters are not collected.

  python tools/bench_ivf_scan.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r43_ivf_scan.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def torch_batch(index, xq, k, probes, off, codes, budget=1 << 30):
    """the padded all-torch scan -> (D, labels) CUDA tensors"""
    import torch

    nq, nprobe = probes.shape
    sizes = off[1:] - off[:-1]
    M, d = index.M, index.d
    width = M if M else 4 * d
    outD, outL = [], []
    q0 = 0
    maxlen_all = int(sizes[probes].max().item())
    step = max(1, budget // max(1, nprobe * maxlen_all * width * 8))
    while q0 < nq:
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        c = pr.shape[0]
        sz = sizes[pr]
        maxlen = max(1, int(sz.max().item()))
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sz[:, :, None]).reshape(c, -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).reshape(c, -1).clamp(max=codes.shape[0] - 1)
        if M:
            dsub = d // M
            tab = ((q.view(c, M, 1, dsub) - index.pq[None]) ** 2).sum(-1)  # [c, M, 256]
            cd = codes[pos].permute(0, 2, 1).long()  # [c, M, P]
            dist = tab.gather(2, cd).sum(1)
        else:
            vec = codes.view(torch.float32).reshape(-1, d)[pos]
            dist = ((vec - q[:, None, :]) ** 2).sum(-1)
        dist = torch.where(valid, dist, torch.full_like(dist, float("inf")))
        kk = min(k, dist.shape[1])
        top = dist.topk(kk, largest=False, sorted=True)
        lab = ((pr << 32)[:, :, None] + ar[None, None, :]).reshape(c, -1).gather(1, top.indices)
        lab = torch.where(torch.isfinite(top.values), lab, torch.full_like(lab, -1))
        outD.append(top.values)
        outL.append(lab)
        q0 += step
    return torch.cat(outD), torch.cat(outL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nprobe", default="1,4,16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r43_ivf_scan.json"))
    a = ap.parse_args()
    import torch

    import ivf_scan_ref as ir
    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib
    from vector_db_id_compression_amd.custom_invlists import CompressedIDInvertedListsPackedBits
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    k = 20
    nqs = [int(v) for v in a.nq.split(",")]

    def copy_rate():
        n = 1 << 25
        x = torch.empty(n, dtype=torch.int64, device="cuda").random_()
        y = torch.empty_like(x)
        for _ in range(3):
            y.copy_(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        return 2 * n * 8 / (e0.elapsed_time(e1) / 20 * 1e-3)

    res = dict(tool="tools/bench_ivf_scan.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, k=k, steps=a.steps,
               warmup=a.warmup, num_cu=ctx.num_cu(), torch_copy_bytes_per_s=round(copy_rate()),
               arms=dict(device="IVFIndex.scan_device (vidc_ivf_scan_dev), probes given",
                         loop="IVFIndex._scan: per-query torch loop, results on the host",
                         batch="padded all-torch batch, probes given, chunked to ~1 GiB of gathered codes",
                         search_device="scan_device + translate_labels, packed-bits container, probes picked inside",
                         search_defer="search_defer_id_decoding over the same container"),
               not_measured="hardware counters; a cap on S for PQ8 (S is what the plan chose, recorded per row); other k, other M",
               rows=[])

    for code, d in ((("PQ", 16), 128), ("Flat", 32)):
        data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
        index = IVFIndex(d, a.nlist, code)
        index.train(data.get_train())
        index.add(data.get_database())
        index.parallel_mode = 3
        index.replace_invlists(CompressedIDInvertedListsPackedBits(index.invlists))
        off_np, codes = index._device_lists()
        off = torch.from_numpy(off_np.astype(np.int64)).cuda()
        sizes = off[1:] - off[:-1]
        kind = ir.PQ8 if index.M else ir.FLAT
        allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()
        for nprobe in [int(v) for v in a.nprobe.split(",")]:
            index.nprobe = nprobe
            for nq in nqs:
                xq = allq[:nq].contiguous()
                xq_host = xq.cpu().numpy()
                probes = torch.cdist(xq, index.centroids).topk(nprobe, largest=False).indices.contiguous()
                code_bytes = int(sizes[probes].sum().item()) * index.code_size
                arms = ["device", "batch", "search_device"] + (["loop", "search_defer"] if nq <= 1000 else [])
                wall = {arm: [] for arm in arms}
                kms, got = [], {}
                for it in range(a.warmup + a.steps):
                    for arm in arms:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        if arm == "device":
                            out = index.scan_device(xq, k, probes=probes)
                        elif arm == "batch":
                            out = torch_batch(index, xq, k, probes, off, codes)
                        elif arm == "loop":
                            out = index._scan(xq_host, k)
                        elif arm == "search_device":
                            out = index.search_device(xq, k)
                        else:
                            out = index.search_defer_id_decoding(xq_host, k)
                        torch.cuda.synchronize()
                        ms = 1e3 * (time.perf_counter() - t0)
                        if arm == "device":
                            km = ctx.last_kernel_ms()
                        if it >= a.warmup:
                            wall[arm].append(ms)
                            if arm == "device":
                                kms.append(km)
                        if arm in ("device", "batch"):
                            got[arm] = out[0]
                        del out
                none = torch.full_like(probes, -1)
                zero = []
                for _ in range(a.steps):
                    index.scan_device(xq, k, probes=none)
                    zero.append(ctx.last_kernel_ms())
                lds = ir.plan_lds(kind, k, nprobe, d, index.M)
                resident = ir.plan_resident(ctx.num_cu(), lds)
                km = float(np.median(kms))
                same = torch.isclose(got["device"], got["batch"], rtol=1e-4, atol=0).all(dim=1)
                row = dict(code="PQ16" if index.M else "Flat", d=d, nprobe=nprobe, nq=nq, S=ir.plan_pieces(nq, nprobe, resident),
                           lds_bytes=lds, resident_slots=resident, code_bytes=code_bytes,
                           device=dict(wall_ms=spread(wall["device"]), last_kernel_ms=spread(kms),
                                       last_kernel_ms_zero_probes=spread(zero),
                                       code_bytes_per_s_of_kernel_time=round(code_bytes / (km * 1e-3)) if km > 0 else None),
                           D_rows_close_to_batch=int(same.sum().item()))
                for arm in arms[1:]:
                    row[arm] = dict(wall_ms=spread(wall[arm]))
                for arm in ("batch", "loop"):
                    if arm in wall:
                        row[f"wall_ratio_{arm}_over_device"] = round(float(np.median(wall[arm]) / np.median(wall["device"])), 2)
                if "search_defer" in wall:
                    row["wall_ratio_search_defer_over_search_device"] = round(float(np.median(wall["search_defer"]) / np.median(wall["search_device"])), 2)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                del got
                torch.cuda.empty_cache()
        del index, codes, data
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
