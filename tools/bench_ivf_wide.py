"""Short lists of 500 and 1000 results from the wide IVF scan (vidc_ivf_scan_aq_wide_dev / vidc_ivf_scan_wide_dev through
IVFIndex.scan_device with k > 256) against what stands beside it, on the same data, lists and probes.

Shape: that of tools/bench_ivf_aq.py -- 10^6 clustered vectors, IVF1024, d = 128, RQ8x8_Nfloat by_residual; nprobe 16 and 64; batches of
10, 10^3 and 10^4 queries; k = 500 and 1000.  Arms, alternating in one process after a warm-up, inputs device-resident, probes given:
  wide     scan_device(xq, k) on the RQ8 residual index
  batch    the padded all-torch batch of tools/bench_ivf_aq.py (decode, one topk per chunk of queries)
The equal-k rows: k = 256, the wide C call against the narrow one over the same probes -- the one comparison at equal k.
The Flat rows: Flat, d = 32, k = 1000, wide against a padded torch batch over the raw vectors.
Recorded per arm: every wall time (perf_counter around the call, ending in a synchronise), median, minimum, maximum, and
vidc_ctx_last_kernel_ms for the device arms.  Flushes per item: the kernel's round / quarter / threshold rule replayed on the host over
the wide arm's own probes for the first queries of a batch, rows uncut (S = 1).  Hardware counters are not collected.

  python tools/bench_ivf_wide.py [--nb 1000000] [--nq 10,1000,10000] [--steps 5] [--out profiles/r51_ivf_wide.json]
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

from bench_ivf_aq import M, spread, torch_batch  # noqa: E402


def flat_batch(xq, k, probes, off, vecs, budget=1 << 30):
    """the padded all-torch scan over raw vectors -> D"""
    import torch

    sizes = off[1:] - off[:-1]
    maxlen = max(1, int(sizes[probes].max().item()))
    step = max(1, budget // (probes.shape[1] * maxlen * vecs.shape[1] * 4 * 2))
    out = []
    for q0 in range(0, xq.shape[0], step):
        pr, q = probes[q0:q0 + step], xq[q0:q0 + step]
        ar = torch.arange(maxlen, device=xq.device)
        valid = (ar[None, None, :] < sizes[pr][:, :, None]).reshape(pr.shape[0], -1)
        pos = (off[pr][:, :, None] + ar[None, None, :]).clamp(max=vecs.shape[0] - 1)
        dist = ((vecs[pos] - q[:, None, None, :]) ** 2).sum(-1).reshape(pr.shape[0], -1)
        dist = torch.where(valid, dist, torch.full_like(dist, float("inf")))
        out.append(dist.topk(min(k, dist.shape[1]), largest=False, sorted=True).values)
    return torch.cat(out)


def flushes(dist_lists, k):
    """the flushes of one uncut item: dist_lists, the float32 distances of its lists in scan order (ivf_wide_plan.h's sizes)"""
    K2 = max(512, 1 << (k - 1).bit_length())
    Q = max(1024, K2) // 4
    pool, cnt, n, pos = np.empty(0, np.uint64), np.zeros(4, np.int64), 0, 0
    buf = []
    for dl in dist_lists:
        keys = (dl.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (pos + np.arange(dl.size, dtype=np.uint64))
        pos += dl.size
        for p0 in range(0, dl.size, 256):
            thr = pool[k - 1] if pool.size >= k else np.uint64(2 ** 64 - 1)
            for w in range(4):
                kw = keys[p0 + 64 * w:p0 + 64 * w + 64]
                kw = kw[kw < thr]
                cnt[w] += kw.size
                buf.append(kw)
            if (cnt + 64 > Q).any():
                pool, cnt, buf, n = np.sort(np.concatenate([pool] + buf))[:K2], np.zeros(4, np.int64), [], n + 1
    return n + (1 if cnt.sum() else 0)


def timed(arms, steps, warmup, ctx, device_arms):
    import torch

    wall, kms, got = {a: [] for a in arms}, {a: [] for a in device_arms}, {}
    for it in range(warmup + steps):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            if it >= warmup:
                wall[name].append(ms)
                if name in kms:
                    kms[name].append(ctx.last_kernel_ms())
            got[name] = out[0] if isinstance(out, tuple) else out
            del out
    row = {a: dict(wall_ms=spread(wall[a]), **({"last_kernel_ms": spread(kms[a])} if a in kms else {})) for a in arms}
    return row, got, wall, kms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nprobe", default="16,64")
    ap.add_argument("--k", default="500,1000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r51_ivf_wide.json"))
    a = ap.parse_args()
    import torch

    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    d = 128
    nqs = [int(v) for v in a.nq.split(",")]
    data = ClusteredVectors(nq=max(nqs), d=d, nt=min(200_000, a.nb), nb=a.nb)
    index = IVFIndex(d, a.nlist, ("RQ", M), by_residual=True)
    index.train_device = index.pq_device = index.coarse_device = True
    index.train(data.get_train())
    index.add(data.get_database())
    off_np, codes = index._device_lists()
    off = torch.from_numpy(off_np.astype(np.int64)).cuda()
    allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()
    res = dict(tool="tools/bench_ivf_wide.py", device=torch.cuda.get_device_name(0), nb=a.nb, nlist=a.nlist, d=d, M=M, steps=a.steps,
               warmup=a.warmup, num_cu=ctx.num_cu(),
               arms=dict(wide="IVFIndex((\"RQ\", 8), by_residual=True).scan_device, k > 256 (vidc_ivf_scan_aq_wide_dev), probes given",
                         batch="padded all-torch batch that decodes the additive codes, probes given, chunked to ~1 GiB",
                         narrow="the same index, k = 256 (vidc_ivf_scan_aq_dev)", wide256="the wide call at k = 256, same probes"),
               flushes="per uncut item, replayed on the host for the first 4 queries of the batch: mean",
               not_measured="hardware counters; other M, d; raw RQ and PQ8 codes; the per-kernel split of a call; flushes of cut items", rows=[])

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    def emit(row):
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        save()
        torch.cuda.empty_cache()

    def replay(D_of, probes, k):
        """mean flushes over the first 4 queries; D_of(q, list) -> float32 distances of the list for query q"""
        sizes = np.diff(off_np)
        return round(float(np.mean([flushes([D_of(q, int(l)) for l in probes[q].tolist() if sizes[int(l)]], k) for q in range(min(4, len(probes)))])), 2)

    def rq_dist(xq):
        def f(q, l):
            rows = codes[int(off_np[l]):int(off_np[l + 1])]
            y = index._decode_codes(rows) + index.centroids[l]
            return ((y - xq[q]) ** 2).sum(1).float().cpu().numpy()
        return f

    for nprobe in [int(v) for v in a.nprobe.split(",")]:
        for nq in nqs:
            xq = allq[:nq].contiguous()
            probes = torch.cdist(xq, index.centroids).topk(nprobe, largest=False).indices.contiguous()
            for k in [int(v) for v in a.k.split(",")]:
                row, got, wall, _ = timed(dict(wide=lambda: index.scan_device(xq, k, probes=probes),
                                               batch=lambda: torch_batch(index, xq, k, probes, off, codes)), a.steps, a.warmup, ctx, ("wide",))
                close = torch.isclose(got["wide"], got["batch"], rtol=1e-3, atol=1e-3).all(dim=1)
                emit(dict(kind="rq8", nprobe=nprobe, nq=nq, k=k, **row, flushes_per_item=replay(rq_dist(xq), probes.cpu().numpy(), k),
                          wall_ratio_batch_over_wide=round(float(np.median(wall["batch"]) / np.median(wall["wide"])), 2),
                          D_rows_close_to_batch=int(close.sum().item())))
            # the one comparison at equal k: the dispatch threshold moved for the wide arm only
            def wide256():
                ivf.NARROW_K = 255
                try:
                    return index.scan_device(xq, 256, probes=probes)
                finally:
                    ivf.NARROW_K = 256
            row, got, wall, kms = timed(dict(narrow=lambda: index.scan_device(xq, 256, probes=probes), wide256=wide256), a.steps, a.warmup, ctx,
                                        ("narrow", "wide256"))
            emit(dict(kind="rq8 equal k", nprobe=nprobe, nq=nq, k=256, **row, equal_bytes=bool(torch.equal(got["narrow"], got["wide256"])),
                      kernel_ratio_narrow_over_wide=round(float(np.median(kms["narrow"]) / np.median(kms["wide256"])), 2)))
    # Flat, d = 32, k = 1000
    fd = 32
    fdata = ClusteredVectors(nq=max(nqs), d=fd, nt=min(200_000, a.nb), nb=a.nb)
    flat = IVFIndex(fd, a.nlist)
    flat.train_device = flat.coarse_device = True
    flat.train(fdata.get_train())
    flat.add(fdata.get_database())
    foff_np, fcodes = flat._device_lists()
    foff, vecs = torch.from_numpy(foff_np.astype(np.int64)).cuda(), fcodes.view(torch.float32).reshape(-1, fd)
    fq = torch.from_numpy(np.ascontiguousarray(fdata.get_queries(), dtype=np.float32)).cuda()
    for nq in nqs:
        xq = fq[:nq].contiguous()
        probes = torch.cdist(xq, flat.centroids).topk(16, largest=False).indices.contiguous()
        row, got, wall, _ = timed(dict(wide=lambda: flat.scan_device(xq, 1000, probes=probes),
                                       batch=lambda: flat_batch(xq, 1000, probes, foff, vecs)), a.steps, a.warmup, ctx, ("wide",))
        close = torch.isclose(got["wide"], got["batch"], rtol=1e-3, atol=1e-3).all(dim=1)
        emit(dict(kind="flat d=32", nprobe=16, nq=nq, k=1000, **row,
                  wall_ratio_batch_over_wide=round(float(np.median(wall["batch"]) / np.median(wall["wide"])), 2),
                  D_rows_close_to_batch=int(close.sum().item())))
    if a.out:
        print("wrote", a.out)


if __name__ == "__main__":
    main()
