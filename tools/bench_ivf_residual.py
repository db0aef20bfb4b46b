"""Residual PQ in the device IVF scan and range search (IVFIndex(..., by_residual=True): vidc_ivf_scan_residual_dev and the two
residual range calls) against what stands beside it, on the same data, lists and probes.

Shape: the reference's (custom_invlist_cpp/bench_invlists.py): 10^6 clustered vectors, IVF1024, PQ16, d = 128, k = 20, nprobe 1 and
16, batches of 10, 10^3 and 10^4 queries.  Two indexes share their centroids and therefore their lists: `residual` encodes
vector - centroid, `raw` the vector.  Arms, alternating in one process after a warm-up, inputs device-resident, probes given:
  residual   scan_device on the residual index
  raw        scan_device on the raw-PQ index: the same code traffic without per-list tables (the floor, recorded, not bounded)
  batch      a padded all-torch batch with residual decoding: a table per (query, probe), the probed lists gathered to a common
             length, one topk per chunk of queries (chunks sized to ~1 GiB) -- the arm `residual` is judged against
Range: ivf_range.range_scan_device at a radius that gives about 100 results per query (the median 100th distance of the batch),
residual against raw (each at its own radius).  Table share: the residual kernels' time on the same probes with every list cut to
one code (one table and one trip per list), next to the full kernel time.  Recall: recall@20 of search_device against exact search
for both indexes -- the reason the feature exists; recorded, not asserted.  Recorded per arm: every wall time (perf_counter around the
call, ending in a synchronise), median, minimum, maximum, and vidc_ctx_last_kernel_ms for the device arms.  Hardware counters are
not collected.

  python tools/bench_ivf_residual.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r45_ivf_residual.json]
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


def torch_batch_residual(index, xq, k, probes, off, codes, budget=1 << 30):
    """the padded all-torch scan with residual decoding -> (D, labels) CUDA tensors"""
    import torch

    nq, nprobe = probes.shape
    sizes = off[1:] - off[:-1]
    M, d = index.M, index.d
    dsub = d // M
    outD, outL = [], []
    maxlen_all = int(sizes[probes].max().item())
    step = max(1, min(budget // max(1, nprobe * maxlen_all * M * 8), budget // (nprobe * M * 256 * dsub * 4 * 2)))
    q0 = 0
    while q0 < nq:
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        c = pr.shape[0]
        sz = sizes[pr]
        maxlen = max(1, int(sz.max().item()))
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sz[:, :, None]).reshape(c, -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).clamp(max=codes.shape[0] - 1)  # [c, nprobe, P]
        r = q[:, None, :] - index.centroids[pr]  # [c, nprobe, d]
        tab = ((r.view(c, nprobe, M, 1, dsub) - index.pq[None, None]) ** 2).sum(-1)  # [c, nprobe, M, 256]
        cd = codes[pos].permute(0, 1, 3, 2).long()  # [c, nprobe, M, P]
        dist = tab.gather(3, cd).sum(2).reshape(c, -1)
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
    ap.add_argument("--nprobe", default="1,16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r45_ivf_residual.json"))
    a = ap.parse_args()
    import torch

    import ivf_residual_ref as rs
    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    k, d, M = 20, 128, 16
    nqs = [int(v) for v in a.nq.split(",")]
    data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
    res_index = IVFIndex(d, a.nlist, ("PQ", M), by_residual=True)
    res_index.train(data.get_train())
    raw_index = IVFIndex(d, a.nlist, ("PQ", M))
    raw_index.train(data.get_train())
    raw_index.centroids = res_index.centroids.clone()  # the same lists: the same probes and the same code traffic
    for index in (res_index, raw_index):
        index.add(data.get_database())
        index.parallel_mode = 3
    off_np, codes = res_index._device_lists()
    raw_off_np, raw_codes = raw_index._device_lists()
    assert np.array_equal(off_np, raw_off_np)
    off = torch.from_numpy(off_np.astype(np.int64)).cuda()
    sizes = off[1:] - off[:-1]
    allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()
    # every list cut to one code (its first; an empty list borrows one): offsets 0 .. nlist
    one_codes = codes[off[:-1].clamp(max=codes.shape[0] - 1)].contiguous()
    one_off = torch.arange(a.nlist + 1, dtype=torch.int64, device="cuda")
    pq, cent = res_index.pq.to(torch.float32).contiguous(), res_index.centroids.to(torch.float32).contiguous()
    ptr = _lib.ptr

    def one_code_scan(xq, probes):
        nq, nprobe = probes.shape
        D = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        L = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().vidc_ivf_scan_residual_dev(ctx.h, a.nlist, ptr(one_off), a.nlist, ptr(one_codes), d, M, ptr(pq), ptr(cent), nq,
                                                         ptr(xq), nprobe, ptr(probes), k, ptr(D), ptr(L), None))
        return ctx.last_kernel_ms()

    def one_code_count(xq, probes, radius):
        nq, nprobe = probes.shape
        lims = torch.empty(nq * nprobe + 1, dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().vidc_ivf_range_count_residual_dev(ctx.h, a.nlist, ptr(one_off), a.nlist, ptr(one_codes), d, M, ptr(pq), ptr(cent),
                                                                nq, ptr(xq), nprobe, ptr(probes), float(radius), ptr(lims), None))
        return ctx.last_kernel_ms()

    # recall@20 against exact search, both indexes, 1000 queries
    nr = min(1000, allq.shape[0])
    xb = torch.from_numpy(np.ascontiguousarray(data.get_database(), dtype=np.float32)).cuda()
    exact = torch.cat([torch.cdist(allq[i:i + 100], xb).topk(k, largest=False).indices for i in range(0, nr, 100)])
    del xb
    recall = {}
    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        for name, index in (("residual", res_index), ("raw", raw_index)):
            index.nprobe = nprobe
            I = index.search_device(allq[:nr], k)[1]
            hit = (I[:, :, None] == exact[:, None, :]).any(2).float().sum(1).mean().item() / k
            recall[f"{name}_nprobe{nprobe}"] = round(hit, 4)
    print(json.dumps(dict(recall_at_20=recall)), flush=True)

    res = dict(tool="tools/bench_ivf_residual.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, d=d, M=M, k=k, steps=a.steps,
               warmup=a.warmup, num_cu=ctx.num_cu(), recall_at_20=recall, recall_queries=nr,
               arms=dict(residual="IVFIndex(by_residual=True).scan_device (vidc_ivf_scan_residual_dev), probes given",
                         raw="IVFIndex.scan_device on raw-PQ codes of the same vectors and lists (vidc_ivf_scan_dev), probes given",
                         batch="padded all-torch batch with residual decoding, probes given, chunked to ~1 GiB"),
               table_share="last_kernel_ms of the residual calls on the same probes over one-code lists (one table, one trip per list)",
               not_measured="hardware counters; the precomputed-table form (not built); other k, M, d; per-kernel split of a cut call",
               rows=[])

    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        res_index.nprobe = raw_index.nprobe = nprobe
        for nq in nqs:
            xq = allq[:nq].contiguous()
            probes = torch.cdist(xq, res_index.centroids).topk(nprobe, largest=False).indices.contiguous()
            code_bytes = int(sizes[probes].sum().item()) * M
            nonempty = int((sizes[probes] > 0).sum().item())
            arms = ["residual", "raw", "batch"]
            wall = {arm: [] for arm in arms}
            kms = {"residual": [], "raw": []}
            got = {}
            for it in range(a.warmup + a.steps):
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if arm == "residual":
                        out = res_index.scan_device(xq, k, probes=probes)
                    elif arm == "raw":
                        out = raw_index.scan_device(xq, k, probes=probes)
                    else:
                        out = torch_batch_residual(res_index, xq, k, probes, off, codes)
                    torch.cuda.synchronize()
                    ms = 1e3 * (time.perf_counter() - t0)
                    km = ctx.last_kernel_ms() if arm in kms else None
                    if it >= a.warmup:
                        wall[arm].append(ms)
                        if arm in kms:
                            kms[arm].append(km)
                    got[arm] = out[0]
                    del out
            tables = [one_code_scan(xq, probes) for _ in range(a.steps)]
            same = torch.isclose(got["residual"], got["batch"], rtol=1e-4, atol=0).all(dim=1)
            lds = rs.plan_lds(k, nprobe, d, M)
            resident = rs.plan_resident(ctx.num_cu(), lds)
            row = dict(kind="scan", nprobe=nprobe, nq=nq, S=rs.plan_pieces(nq, nprobe, resident), lds_bytes=lds, resident_slots=resident,
                       code_bytes=code_bytes, tables_built=nonempty, codebook_bytes_read=nonempty * 256 * d * 4,
                       residual=dict(wall_ms=spread(wall["residual"]), last_kernel_ms=spread(kms["residual"]),
                                     last_kernel_ms_one_code_lists=spread(tables)),
                       raw=dict(wall_ms=spread(wall["raw"]), last_kernel_ms=spread(kms["raw"])),
                       batch=dict(wall_ms=spread(wall["batch"])),
                       table_share_of_kernel_time=round(float(np.median(tables) / np.median(kms["residual"])), 3),
                       kernel_ratio_residual_over_raw=round(float(np.median(kms["residual"]) / np.median(kms["raw"])), 2),
                       wall_ratio_residual_over_raw=round(float(np.median(wall["residual"]) / np.median(wall["raw"])), 2),
                       wall_ratio_batch_over_residual=round(float(np.median(wall["batch"]) / np.median(wall["residual"])), 2),
                       D_rows_close_to_batch=int(same.sum().item()))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            # the range search at about 100 results per query, each index at its own radius
            D100 = {name: index.scan_device(xq, 100, probes=probes)[0][:, -1] for name, index in (("residual", res_index), ("raw", raw_index))}
            radius = {name: float(v[torch.isfinite(v)].median().item()) if torch.isfinite(v).any() else float("inf") for name, v in D100.items()}
            rwall, rk, per_q = {"residual": [], "raw": []}, {"residual": [], "raw": []}, {}
            for it in range(a.warmup + a.steps):
                for name, index in (("residual", res_index), ("raw", raw_index)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lims, rD, _ = ivf_range.range_scan_device(index, xq, radius[name], probes=probes)
                    torch.cuda.synchronize()
                    ms = 1e3 * (time.perf_counter() - t0)
                    if it >= a.warmup:
                        rwall[name].append(ms)
                        rk[name].append(ctx.last_kernel_ms())  # (the fill's: the call that ran last)
                    per_q[name] = float((lims[1:] - lims[:-1]).float().median().item())
                    del lims, rD
            rtab = [one_code_count(xq, probes, radius["residual"]) for _ in range(a.steps)]
            row = dict(kind="range", nprobe=nprobe, nq=nq, radius=radius, results_per_query_median=per_q,
                       residual=dict(wall_ms=spread(rwall["residual"]), fill_kernel_ms=spread(rk["residual"]),
                                     count_kernel_ms_one_code_lists=spread(rtab)),
                       raw=dict(wall_ms=spread(rwall["raw"]), fill_kernel_ms=spread(rk["raw"])),
                       wall_ratio_residual_over_raw=round(float(np.median(rwall["residual"]) / np.median(rwall["raw"])), 2))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del got
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
