"""One Lloyd iteration on the device (ivf_train.kmeans_step_device, vidc_ivf_kmeans_step_dev) against the torch body of one
ivf._kmeans iteration (chunked cdist + argmin, index_add_, bincount, where; for G groups G such bodies one after the other on the
column views train passes), on the same device-resident inputs; and IVFIndex.train end to end with train_device off against on
(IVF1024, PQ16, 2 * 10^5 host vectors; a fresh index per repetition).

Shapes (n, G, dsub, k): (2 * 10^5, 1, 128, 1024), (2 * 10^6, 1, 128, 65536), (2 * 10^5, 16, 8, 256), (2 * 10^5, 4, 32, 256).  Gaussian
data.  Arms alternate in one process, every shape warmed.  Recorded per row: wall ms (perf_counter around the call, ending in a
synchronise) as median, min, max and count; for the device arm vidc_ctx_last_kernel_ms (all kernels of the call); FLOP/s of the
assignment = 2 n G k dsub over that time next to the float32 matrix peak (an upper bound of the assignment's own share: the time
includes the sort and the update); the share of points whose assignment equals torch's.  No threshold: every row is reported, also
where the device arm loses.  Hardware counters and a kernel trace are not collected.

  python tools/bench_ivf_train.py [--steps 5] [--skip-large] [--out profiles/r48_ivf_train.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12  # AMD's published MI355X figure (product brief): float32 matrix
SHAPES = ((200_000, 1, 128, 1024), (2_000_000, 1, 128, 65536), (200_000, 16, 8, 256), (200_000, 4, 32, 256))


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 2 * 10^6 x 65536 shape")
    ap.add_argument("--ntrain", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r48_ivf_train.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, ivf_train
    from vector_db_id_compression_amd.ivf import IVFIndex, _assign

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_ivf_train.py", device=torch.cuda.get_device_name(0), num_cu=ctx.num_cu(), steps=a.steps, warmup=a.warmup,
               peak_flops=PEAK_FLOPS, peak_source="AMD Instinct MI355X product brief: FP32 matrix",
               arms=dict(device="ivf_train.kmeans_step_device (vidc_ivf_kmeans_step_dev)", torch="the torch body of one ivf._kmeans iteration per group",
                         train_on="IVFIndex.train, train_device = True", train_off="IVFIndex.train, train_device = False"),
               not_measured="hardware counters; a kernel trace (the split of last_kernel_ms between assignment, sort and update); LDS bank "
                            "conflicts; points staged in LDS instead of re-read per centroid tile; more than two workgroups a compute unit",
               rows=[], train_rows=[])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def torch_step(x, c):
        outs = []
        for g in range(c.shape[0]):
            xg, cg = x[:, g * c.shape[2]:(g + 1) * c.shape[2]], c[g]
            asg = _assign(xg, cg)
            sums = torch.zeros_like(cg).index_add_(0, asg, xg)
            cnt = torch.bincount(asg, minlength=cg.shape[0]).to(xg.dtype)[:, None]
            outs.append((torch.where(cnt > 0, sums / cnt.clamp(min=1), cg), asg))
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])

    for n, G, dsub, k in SHAPES:
        if a.skip_large and n * k > 10 ** 10:
            continue
        x = torch.randn((n, G * dsub), generator=gen, device="cuda")
        c = torch.stack([x[torch.randperm(n, generator=gen, device="cuda")[:k], g * dsub:(g + 1) * dsub] for g in range(G)]).contiguous()
        arms = dict(device=lambda: ivf_train.kmeans_step_device(x, c, groups=G), torch=lambda: torch_step(x, c))
        wall, kms, got = {name: [] for name in arms}, [], {}
        for it in range(a.warmup + a.steps):
            for name, fn in arms.items():
                ms, out = timed(torch, fn)
                if it >= a.warmup:
                    wall[name].append(ms)
                    if name == "device":
                        kms.append(ctx.last_kernel_ms())
                got[name] = out[1]
                del out
        km = float(np.median(kms)) * 1e-3
        flop = 2.0 * n * G * k * dsub
        row = dict(n=n, G=G, dsub=dsub, k=k, device_wall_ms=spread(wall["device"]), torch_wall_ms=spread(wall["torch"]), last_kernel_ms=spread(kms),
                   wall_ratio_torch_over_device=round(float(np.median(wall["torch"]) / np.median(wall["device"])), 2),
                   assign_flop_over_call_kernel_time=round(flop / km), share_of_fp32_matrix_peak_lower_bound=round(flop / km / PEAK_FLOPS, 4),
                   assign_equal_to_torch=round(float((got["device"].long() == got["torch"]).float().mean().item()), 6))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del got, x, c
        torch.cuda.empty_cache()

    d, M, nlist = 128, 16, 1024
    xt = torch.randn((a.ntrain, d), generator=gen, device="cuda").cpu().numpy()  # (train takes host vectors: both arms pay the same upload)
    wall = dict(train_on=[], train_off=[])
    for it in range(a.warmup + a.steps):
        for name in wall:
            index = IVFIndex(d, nlist, ("PQ", M))
            index.train_device = name == "train_on"
            ms, _ = timed(torch, lambda: index.train(xt))
            if it >= a.warmup:
                wall[name].append(ms)
            del index
    row = dict(index="IVF1024,PQ16", ntrain=a.ntrain, d=d, on_wall_ms=spread(wall["train_on"]), off_wall_ms=spread(wall["train_off"]),
               wall_ratio_off_over_on=round(float(np.median(wall["train_off"]) / np.median(wall["train_on"])), 2))
    res["train_rows"].append(row)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        head = [f" {json.dumps(k)}: {json.dumps(v)}," for k, v in res.items() if k not in ("rows", "train_rows")]
        body = [f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in res[name]) + "\n ]" for name in ("rows", "train_rows")]
        with open(a.out, "w") as f:  # one record a line
            f.write("{\n" + "\n".join(head) + "\n" + ",\n".join(body) + "\n}\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
