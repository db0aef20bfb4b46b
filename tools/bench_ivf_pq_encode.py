"""The PQ encoder on the device (ivf_encode.pq_encode_device, vidc_ivf_pq_encode_dev) against the torch body of
IVFIndex._encode_dev (M calls of torch.cdist(...).argmin(1) in chunks of 65 536 rows, x - centroids[assign] in front for the residual
form), on the same device-resident inputs; and IVFIndex.add of --nadd host vectors into a packed-bits container with coarse_device
on, pq_device off against on (a fresh index per repetition; both arms pay the same upload).

Grid: n = 10^4 / 10^5 / 10^6 crossed with (d, M) = (128, 16), (128, 32), (128, 4), (96, 16), each raw and residual (nlist 1024).
Gaussian data (the kernel's time does not depend on the values).  Arms alternate in one process, every shape warmed.  Recorded per
row: wall ms (perf_counter around the call, ending in a synchronise) as median, min, max and count; for the device arm
vidc_ctx_last_kernel_ms; FLOP/s = 2 n 256 d over the kernel time next to the float32 matrix peak (the MFMAs issued are
2 n 256 M round_up(d / M, 16): flop_issued_per_s); the bytes the kernel has to move; the share of rows whose codes equal torch's.  No
threshold: every row is reported, also where the device arm loses.  Hardware counters are not collected.

  python tools/bench_ivf_pq_encode.py [--n 10000,100000,1000000] [--steps 5] [--nadd 1000000] [--out profiles/r47_ivf_pq_encode.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# AMD's published MI355X figures (product brief): float32 matrix 157.3 TFLOP/s, HBM3E 8 TB/s
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
SHAPES = ((128, 16), (128, 32), (128, 4), (96, 16))


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4), n=len(v))


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000,100000,1000000")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nadd", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r47_ivf_pq_encode.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, ivf_encode
    from vector_db_id_compression_amd.custom_invlists import CompressedIDInvertedListsPackedBits
    from vector_db_id_compression_amd.ivf import IVFIndex, _assign

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    ns = [int(v) for v in a.n.split(",")]
    res = dict(tool="tools/bench_ivf_pq_encode.py", device=torch.cuda.get_device_name(0), num_cu=ctx.num_cu(), steps=a.steps, warmup=a.warmup,
               peaks=dict(flops=PEAK_FLOPS, bytes_per_s=PEAK_BYTES, source="AMD Instinct MI355X product brief: FP32 matrix, HBM3E"),
               arms=dict(device="ivf_encode.pq_encode_device (vidc_ivf_pq_encode_dev)", torch="the torch body of IVFIndex._encode_dev",
                         add_on="IVFIndex.add, coarse_device = True, pq_device = True", add_off="IVFIndex.add, coarse_device = True, pq_device = False"),
               not_measured="hardware counters; a kernel trace; LDS bank conflicts; the cost of the byte stores at stride M; MT = 1; "
                            "the share of centroid gathers served by L2",
               rows=[], add_rows=[])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def torch_encode(x, pq, cent, assign):
        if cent is not None:
            x = x - cent[assign]
        dsub = x.shape[1] // pq.shape[0]
        return torch.stack([_assign(x[:, m * dsub:(m + 1) * dsub].contiguous(), pq[m]) for m in range(pq.shape[0])], 1).to(torch.uint8)

    for d, M in SHAPES:
        dsub = d // M
        pq = torch.randn((M, 256, dsub), generator=gen, device="cuda")
        cent = torch.randn((a.nlist, d), generator=gen, device="cuda")
        allx = torch.randn((max(ns), d), generator=gen, device="cuda")
        alla = torch.randint(0, a.nlist, (max(ns),), generator=gen, device="cuda")
        for n in ns:
            x, assign = allx[:n].contiguous(), alla[:n].contiguous()
            for residual in (False, True):
                c, s = (cent, assign) if residual else (None, None)
                arms = dict(device=lambda: ivf_encode.pq_encode_device(x, pq, c, s), torch=lambda: torch_encode(x, pq, c, s))
                wall, kms, got = {k: [] for k in arms}, [], {}
                for it in range(a.warmup + a.steps):
                    for name, fn in arms.items():
                        ms, out = timed(torch, fn)
                        if it >= a.warmup:
                            wall[name].append(ms)
                            if name == "device":
                                kms.append(ctx.last_kernel_ms())
                        got[name] = out
                        del out
                km = float(np.median(kms)) * 1e-3
                flop, issued = 2.0 * n * 256 * d, 2.0 * n * 256 * M * (-(-dsub // 16) * 16)
                nbytes = float(n) * d * 4 * (2 if residual else 1) + float(n) * M + (8.0 * n if residual else 0)
                row = dict(n=n, d=d, M=M, dsub=dsub, residual=residual, device_wall_ms=spread(wall["device"]), torch_wall_ms=spread(wall["torch"]),
                           last_kernel_ms=spread(kms), wall_ratio_torch_over_device=round(float(np.median(wall["torch"]) / np.median(wall["device"])), 2),
                           flop_per_s=round(flop / km), flop_issued_per_s=round(issued / km), share_of_fp32_matrix_peak=round(flop / km / PEAK_FLOPS, 4),
                           bytes_moved=int(nbytes), bytes_per_s=round(nbytes / km),
                           bound="compute" if flop / PEAK_FLOPS > nbytes / PEAK_BYTES else "memory",
                           share_of_bound=round(max(flop / PEAK_FLOPS, nbytes / PEAK_BYTES) / km, 4),
                           rows_equal_to_torch=round(float((got["device"] == got["torch"]).all(1).float().mean().item()), 6))
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                del got
        del pq, cent, allx, alla
        torch.cuda.empty_cache()

    # end to end: add into packed-bits lists (PQ16, d = 128, nlist 1024), list assignment from the probe kernel, the flag off against on
    d, M = 128, 16
    pq = torch.randn((M, 256, d // M), generator=gen, device="cuda")
    cent = torch.randn((a.nlist, d), generator=gen, device="cuda")
    xb = torch.randn((a.nadd, d), generator=gen, device="cuda")
    xb = xb.cpu().numpy()  # (add takes host vectors: both arms pay the same upload)
    seed = xb[:1000]
    for residual in (False, True):
        wall = dict(add_on=[], add_off=[])
        for it in range(a.warmup + a.steps):
            for name in wall:
                index = IVFIndex(d, a.nlist, ("PQ", M), by_residual=residual)
                index.centroids, index.pq, index.coarse_device, index.pq_device = cent, pq, True, name == "add_on"
                index.add(seed)
                index.replace_invlists(CompressedIDInvertedListsPackedBits(index.invlists))
                ms, _ = timed(torch, lambda: index.add(xb))
                if it >= a.warmup:
                    wall[name].append(ms)
                del index
        row = dict(code="PQ16", ids="packed bits", nadd=a.nadd, nlist=a.nlist, d=d, residual=residual, on_wall_ms=spread(wall["add_on"]),
                   off_wall_ms=spread(wall["add_off"]), wall_ratio_off_over_on=round(float(np.median(wall["add_off"]) / np.median(wall["add_on"])), 2))
        res["add_rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        head = [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in res.items() if k not in ("rows", "add_rows")]
        body = [f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in res[name]) + "\n ]" for name in ("rows", "add_rows")]
        with open(a.out, "w") as f:  # one record a line
            f.write("{\n" + "\n".join(head) + "\n" + ",\n".join(body) + "\n}\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
