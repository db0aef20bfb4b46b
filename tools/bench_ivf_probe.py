"""The coarse quantiser on the device (ivf_probe.probe_device, vidc_ivf_probe_dev) against the parent's path,
torch.cdist(xq, centroids).topk(nprobe, largest=False), on the same centroids and queries; and search_device over a packed-bits /
PQ16 index with IVFIndex.coarse_device on against off.

Shapes: nlist 1024 and 65536 at 10 / 10^3 / 10^4 queries, 2^20 at 10 and 10^3; d = 32 and 128; nprobe 1 / 16 / 64 / 256.  Gaussian
centroids and queries (the kernels' time does not depend on the values).  Arms alternate in one process, every shape warmed.
Recorded per row: wall ms (perf_counter around the call, ending in a synchronise) as median, min, max and count; for the device arm
vidc_ctx_last_kernel_ms, the plan's TQ and S, FLOP/s = 2 nq nlist d over the kernel time, the centroid bytes read = nlist d 4 per
query tile, and which of the two bounds the shape at the peak figures below.  No threshold: every row is reported, also where the
device arm loses.  Hardware counters are not collected.

  python tools/bench_ivf_probe.py [--nq 10,1000,10000] [--steps 5] [--nb 200000] [--out profiles/r46_ivf_probe.json]
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

# AMD's published MI355X figures (product brief): float32 matrix 157.3 TFLOP/s, HBM3E 8 TB/s
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


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
    ap.add_argument("--nq", default="10,1000,10000")
    ap.add_argument("--nlist", default="1024,65536,1048576")
    ap.add_argument("--nprobe", default="1,16,64,256")
    ap.add_argument("--nb", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r46_ivf_probe.json"))
    a = ap.parse_args()
    import torch

    from _harness import ClusteredVectors
    from vector_db_id_compression_amd import _lib, ivf_probe
    from vector_db_id_compression_amd.custom_invlists import CompressedIDInvertedListsPackedBits
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    num_cu = ctx.num_cu()
    nqs, nprobes = [int(v) for v in a.nq.split(",")], [int(v) for v in a.nprobe.split(",")]
    res = dict(tool="tools/bench_ivf_probe.py", device=torch.cuda.get_device_name(0), num_cu=num_cu, steps=a.steps, warmup=a.warmup,
               peaks=dict(flops=PEAK_FLOPS, bytes_per_s=PEAK_BYTES, source="AMD Instinct MI355X product brief: FP32 matrix, HBM3E"),
               arms=dict(device="ivf_probe.probe_device (vidc_ivf_probe_dev)", torch="torch.cdist(xq, centroids).topk(nprobe, largest=False)",
                         search_on="IVFIndex.search_device, coarse_device = True", search_off="IVFIndex.search_device, coarse_device = False"),
               not_measured="hardware counters; LDS bank conflicts; the share of centroid reads served by L2 / MALL; other TC / KC",
               rows=[], search_rows=[])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    for nlist in [int(v) for v in a.nlist.split(",")]:
        for d in (32, 128):
            idx = IVFIndex(d, nlist)
            idx.centroids = torch.randn((nlist, d), generator=gen, device="cuda")
            allq = torch.randn((max(nqs), d), generator=gen, device="cuda")
            for nq in (n for n in nqs if nlist < (1 << 20) or n <= 1000):
                xq = allq[:nq].contiguous()
                for nprobe in nprobes:
                    arms = dict(device=lambda: ivf_probe.probe_device(idx, xq, nprobe),
                                torch=lambda: torch.cdist(xq, idx.centroids).topk(nprobe, largest=False))
                    wall, kms, got = {k: [] for k in arms}, [], {}
                    for it in range(a.warmup + a.steps):
                        for name, fn in arms.items():
                            ms, out = timed(torch, fn)
                            if it >= a.warmup:
                                wall[name].append(ms)
                                if name == "device":
                                    kms.append(ctx.last_kernel_ms())
                            got[name] = out[0] if name == "device" else out.indices
                            del out
                    TQ = 32 if nprobe <= 64 else 16
                    qtiles, km = -(-nq // TQ), float(np.median(kms)) * 1e-3
                    flop, cbytes = 2.0 * nq * nlist * d, float(nlist) * d * 4 * qtiles
                    row = dict(nlist=nlist, d=d, nq=nq, nprobe=nprobe, TQ=TQ, query_tiles=qtiles, device_wall_ms=spread(wall["device"]),
                               torch_wall_ms=spread(wall["torch"]), last_kernel_ms=spread(kms),
                               wall_ratio_torch_over_device=round(float(np.median(wall["torch"]) / np.median(wall["device"])), 2),
                               flop_per_s=round(flop / km), centroid_bytes_read=int(cbytes), centroid_bytes_per_s=round(cbytes / km),
                               bound="compute" if flop / PEAK_FLOPS > cbytes / PEAK_BYTES else "memory",
                               share_of_bound=round(max(flop / PEAK_FLOPS, cbytes / PEAK_BYTES) / km, 3),
                               rows_equal_to_torch=int((got["device"] == got["torch"]).all(1).sum().item()))
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
                    del got
            del idx, allq
            torch.cuda.empty_cache()

    # end to end: search_device over packed-bits ids and PQ16 codes, the flag on against off
    data = ClusteredVectors(nq=max(nqs), d=128, nt=min(50_000, a.nb), nb=a.nb)
    index = IVFIndex(128, 1024, ("PQ", 16))
    index.train(data.get_train())
    index.add(data.get_database())
    index.replace_invlists(CompressedIDInvertedListsPackedBits(index.invlists))
    allq = torch.from_numpy(np.ascontiguousarray(data.get_queries(), dtype=np.float32)).cuda()
    for nq in nqs:
        xq = allq[:nq].contiguous()
        for nprobe in nprobes:
            index.nprobe = nprobe
            wall = dict(search_on=[], search_off=[])
            for it in range(a.warmup + a.steps):
                for name in wall:
                    index.coarse_device = name == "search_on"
                    ms, out = timed(torch, lambda: index.search_device(xq, 20))
                    if it >= a.warmup:
                        wall[name].append(ms)
                    del out
            row = dict(code="PQ16", ids="packed bits", nb=a.nb, nlist=1024, d=128, k=20, nq=nq, nprobe=nprobe, on_wall_ms=spread(wall["search_on"]),
                       off_wall_ms=spread(wall["search_off"]),
                       wall_ratio_off_over_on=round(float(np.median(wall["search_off"]) / np.median(wall["search_on"])), 2))
            res["search_rows"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        head = [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in res.items() if k not in ("rows", "search_rows")]
        body = [f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in res[name]) + "\n ]" for name in ("rows", "search_rows")]
        with open(a.out, "w") as f:  # one record a line
            f.write("{\n" + "\n".join(head) + "\n" + ",\n".join(body) + "\n}\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
