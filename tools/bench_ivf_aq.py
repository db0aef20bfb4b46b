"""Additive-quantiser codes in the device IVF scan (IVFIndex(d, nlist, ("RQ", 8), by_residual=True): vidc_ivf_scan_aq_dev and its table
GEMM vidc_ivf_aq_lut_dev) against what stands beside them, on the same data, lists and probes.

Shape: 10^6 clustered vectors, IVF1024, RQ8x8_Nfloat (12 bytes a vector), d = 128, k = 20, nprobe 1 and 16, batches of 10, 10^3 and
10^4 queries.  Arms, alternating in one process after a warm-up, inputs device-resident, probes given:
  aq       scan_device on the RQ8 residual index: one GEMM-built 8 KB table per query, copied into LDS per (query, piece)
  batch    a padded all-torch batch that decodes the codes (sum of 8 codewords + centroid) and takes one topk per chunk of queries
           (chunks sized to ~1 GiB) -- the arm `aq` is judged against
  pq8      scan_device on a raw PQ8 index (8 bytes a vector) over the same lists and probes: the same scan with a table built per item
           by its own wavefront and no GEMM -- the floor
The table GEMM alone: vidc_ivf_aq_lut_dev on the batch's queries, its kernel time and 2 nq M 256 d / time in TFLOP/s.  Recorded per
arm: every wall time (perf_counter around the call, ending in a synchronise), median, minimum, maximum, and vidc_ctx_last_kernel_ms
for the device arms.  Hardware counters are not collected.

  python tools/bench_ivf_aq.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r50_ivf_aq.json]
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

M = 8


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def torch_batch(index, xq, k, probes, off, codes, budget=1 << 30):
    """the padded all-torch scan that decodes additive residual codes -> (D, labels) CUDA tensors"""
    import torch

    nq, nprobe = probes.shape
    sizes = off[1:] - off[:-1]
    outD, outL = [], []
    maxlen_all = max(1, int(sizes[probes].max().item()))
    step = max(1, budget // (nprobe * maxlen_all * index.d * 4 * 3))
    for q0 in range(0, nq, step):
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        c = pr.shape[0]
        sz = sizes[pr]
        maxlen = max(1, int(sz.max().item()))
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sz[:, :, None]).reshape(c, -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).clamp(max=codes.shape[0] - 1)  # [c, nprobe, P]
        idx = codes[pos][..., :M].long()
        vecs = index.centroids[pr][:, :, None, :].expand(c, nprobe, maxlen, index.d).clone()
        for m in range(M):
            vecs += index.pq[m][idx[..., m]]
        dist = ((vecs - q[:, None, None, :]) ** 2).sum(-1).reshape(c, -1)
        dist = torch.where(valid, dist, torch.full_like(dist, float("inf")))
        top = dist.topk(min(k, dist.shape[1]), largest=False, sorted=True)
        lab = ((pr << 32)[:, :, None] + ar[None, None, :]).reshape(c, -1).gather(1, top.indices)
        outD.append(top.values)
        outL.append(torch.where(torch.isfinite(top.values), lab, torch.full_like(lab, -1)))
    return torch.cat(outD), torch.cat(outL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nprobe", default="1,16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r50_ivf_aq.json"))
    a = ap.parse_args()
    import torch

    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf_aq
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    k, d = 20, 128
    nqs = [int(v) for v in a.nq.split(",")]
    data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
    aq_index = IVFIndex(d, a.nlist, ("RQ", M), by_residual=True)
    pq_index = IVFIndex(d, a.nlist, ("PQ", M))
    for index in (aq_index, pq_index):
        index.train_device = index.pq_device = index.coarse_device = True
        index.train(data.get_train())
    pq_index.centroids = aq_index.centroids.clone()  # the same lists and the same probes
    for index in (aq_index, pq_index):
        index.add(data.get_database())
    off_np, codes = aq_index._device_lists()
    assert np.array_equal(off_np, pq_index._device_lists()[0]) and codes.shape[1] == M + 4
    off = torch.from_numpy(off_np.astype(np.int64)).cuda()
    sizes = off[1:] - off[:-1]
    allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()

    res = dict(tool="tools/bench_ivf_aq.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, d=d, M=M, k=k, steps=a.steps,
               warmup=a.warmup, num_cu=ctx.num_cu(),
               arms=dict(aq="IVFIndex((\"RQ\", 8), by_residual=True).scan_device (vidc_ivf_scan_aq_dev), probes given",
                         batch="padded all-torch batch that decodes the additive codes, probes given, chunked to ~1 GiB",
                         pq8="IVFIndex((\"PQ\", 8)).scan_device over the same lists and probes (vidc_ivf_scan_dev)"),
               lut="vidc_ivf_aq_lut_dev on the batch's queries: last_kernel_ms and 2 nq M 256 d / time",
               not_measured="hardware counters; raw (non-residual) RQ codes; other k, M, d; the per-kernel split of a scan call", rows=[])

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        for nq in nqs:
            xq = allq[:nq].contiguous()
            probes = torch.cdist(xq, aq_index.centroids).topk(nprobe, largest=False).indices.contiguous()
            arms = ["aq", "batch", "pq8"]
            wall = {arm: [] for arm in arms}
            kms = {"aq": [], "pq8": []}
            got = {}
            for it in range(a.warmup + a.steps):
                for arm in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if arm == "aq":
                        out = aq_index.scan_device(xq, k, probes=probes)
                    elif arm == "pq8":
                        out = pq_index.scan_device(xq, k, probes=probes)
                    else:
                        out = torch_batch(aq_index, xq, k, probes, off, codes)
                    torch.cuda.synchronize()
                    ms = 1e3 * (time.perf_counter() - t0)
                    if it >= a.warmup:
                        wall[arm].append(ms)
                        if arm in kms:
                            kms[arm].append(ctx.last_kernel_ms())
                    got[arm] = out[0]
                    del out
            lut = []
            for it in range(a.warmup + a.steps):
                ivf_aq.lut_device(aq_index.pq, xq)
                if it >= a.warmup:
                    lut.append(ctx.last_kernel_ms())
            same = torch.isclose(got["aq"], got["batch"], rtol=1e-3, atol=1e-3).all(dim=1)
            row = dict(kind="scan", nprobe=nprobe, nq=nq, code_bytes=int(sizes[probes].sum().item()) * (M + 4),
                       aq=dict(wall_ms=spread(wall["aq"]), last_kernel_ms=spread(kms["aq"])),
                       batch=dict(wall_ms=spread(wall["batch"])),
                       pq8=dict(wall_ms=spread(wall["pq8"]), last_kernel_ms=spread(kms["pq8"])),
                       lut=dict(last_kernel_ms=spread(lut), tflops=round(2.0 * nq * M * 256 * d / (np.median(lut) * 1e-3) / 1e12, 3)),
                       lut_share_of_kernel_time=round(float(np.median(lut) / np.median(kms["aq"])), 3),
                       kernel_ratio_aq_over_pq8=round(float(np.median(kms["aq"]) / np.median(kms["pq8"])), 2),
                       wall_ratio_batch_over_aq=round(float(np.median(wall["batch"]) / np.median(wall["aq"])), 2),
                       D_rows_close_to_batch=int(same.sum().item()))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            save()
            del got
            torch.cuda.empty_cache()
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
