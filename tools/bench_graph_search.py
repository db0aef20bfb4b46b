"""The one-launch graph search (graph_search.search_device, vidc_*_search_dev) against the batched torch search it stands beside
(graph_search.search_batched, unchanged by the commit that added the kernel), on the same inputs.

Shape: the 10^6 x 64 rows of BASELINE configs[3] as an exact kNN graph (graph_search.knn_graph: out-degrees in [32, 64]) over d = 16
Gaussian vectors; k = 10, L = 64, entry 0; 10^3 and 10^4 queries.  Arms, alternating in one process after a warm-up, for raw, compact
and Elias-Fano rows: "device" = search_device, "batched" = search_batched (results copied to the host, as it always does).
Recorded per arm: every wall time (perf_counter around the call, ending in a synchronise), median, minimum and maximum;
vidc_ctx_last_kernel_ms of the device arm, and of the same launch capped at one step per query (clear + entry + one row: an upper
bound of what the visited clear costs); the peak of torch's allocator during the arm and, for the device arm, the visited-set
scratch the library takes from its own cache (slots * ceil(N / 64) * 8 bytes); how many result rows the two arms agree on (they sum a
distance in different orders, so a last-bit difference can reorder a near-tie).  No threshold: every arm is reported, also where it loses.

  python tools/bench_graph_search.py [--n 1000000] [--nq 1000,10000] [--steps 5] [--out profiles/r41_graph_search.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--nq", default="1000,10000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r41_graph_search.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, altid
    from vector_db_id_compression_amd.graph_search import RawGraph, knn_graph, search_batched, search_device

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    k, L = 10, 64
    rng = np.random.default_rng(41)
    x = rng.normal(size=(a.n, a.d)).astype(np.float32)
    t0 = time.perf_counter()
    rows = knn_graph(x, a.K, seed=3)
    build_s = time.perf_counter() - t0
    xt = torch.from_numpy(x).cuda()
    graphs = dict(raw=RawGraph(rows), compact=altid.CompactBitNSGGraph(rows.copy()))
    graphs["elias-fano"] = altid.EliasFanoNSGGraph(rows.copy())
    res = dict(tool="tools/bench_graph_search.py", device=torch.cuda.get_device_name(0), N=a.n, K=a.K, d=a.d, k=k, L=L, entry=0,
               steps=a.steps, warmup=a.warmup, graph=f"knn_graph of {a.n} x {a.d} Gaussian vectors, out-degrees in [{a.K // 2}, {a.K}]",
               graph_build_s=round(build_s, 1), edges=int((rows >= 0).sum()),
               arms=dict(device="graph_search.search_device (one launch, a wavefront per query)",
                         batched="graph_search.search_batched (torch, one round of ~20 kernels per expansion, nq x (N + 1) visited matrix)"),
               not_measured="hardware counters, other d, other L, other K, inner product", rows=[])
    slots = lambda nq: max(1, min(nq, ctx.num_cu() * 32, 1024))

    for nq in [int(v) for v in a.nq.split(",")]:
        xq = rng.normal(size=(nq, a.d)).astype(np.float32)
        for name, g in graphs.items():
            wall = dict(device=[], batched=[])
            kms, peak, got = [], dict(device=0, batched=0), {}
            for it in range(a.warmup + a.steps):
                for arm in ("device", "batched"):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    t0 = time.perf_counter()
                    if arm == "device":
                        D, I, st = search_device(g, xt, xq, k, L=L, stats=True)
                        torch.cuda.synchronize()
                        ms = 1e3 * (time.perf_counter() - t0)
                        got[arm] = (I.cpu().numpy(), st.cpu().numpy())
                        km = ctx.last_kernel_ms()
                    else:
                        D, I = search_batched(g, xt, xq, k, L=L)
                        torch.cuda.synchronize()
                        ms = 1e3 * (time.perf_counter() - t0)
                        got[arm] = (I,)
                    peak[arm] = max(peak[arm], torch.cuda.max_memory_allocated() - base)
                    if it >= a.warmup:
                        wall[arm].append(ms)
                        if arm == "device":
                            kms.append(km)
                    del D, I
            # what the visited clear can cost at most: the same launch capped at ONE step per query still clears every slot in front
            # of every query, computes the entry's distance and expands one row
            one = []
            for _ in range(a.steps):
                search_device(g, xt, xq, k, L=L, max_rounds=1)
                one.append(ctx.last_kernel_ms())
            st = got["device"][1]
            row = dict(rows=name, nq=nq, device=dict(wall_ms=spread(wall["device"]), last_kernel_ms=spread(kms),
                                                      last_kernel_ms_one_step_per_query=spread(one),
                                                      torch_peak_bytes=int(peak["device"]),
                                                      library_scratch_bytes=slots(nq) * ((a.n + 63) // 64) * 8),
                       batched=dict(wall_ms=spread(wall["batched"]), torch_peak_bytes=int(peak["batched"])),
                       wall_ratio_batched_over_device=round(float(np.median(wall["batched"]) / np.median(wall["device"])), 2),
                       result_rows_equal=int((got["device"][0] == got["batched"][0]).all(axis=1).sum()),
                       steps_per_query=dict(min=int(st[:, 0].min()), median=float(np.median(st[:, 0])), max=int(st[:, 0].max())),
                       distances_per_query=dict(min=int(st[:, 1].min()), median=float(np.median(st[:, 1])), max=int(st[:, 1].max())))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
