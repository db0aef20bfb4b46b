"""update_rows against the rebuild from the entry points that existed before it (profiles/r32_rows_update.json).

Workload: the 10^6 x 64 graph rows of BASELINE configs[3] (synth.make_graph_rows).  Batches of 10^3 and 10^5 rows of distinct random
nodes, at N_new = N_old (rows of existing nodes replaced) and at N_new = N_old + batch (the batch rows are the new nodes' rows).
Inputs are device-resident.  Two arms per (codec, batch, growth), timed alternately, wall ms (perf_counter around the call, the device
synchronised on both sides), median of --steps after --warmup:
  update_rows   codecs.update_rows(obj, nodes, rows, n_new)
  rebuild       decode_rows of every node + a torch scatter of the batch rows (+ a torch.cat of empty rows for the new nodes) +
                encode_rows of the whole matrix
The results of the two arms are compared once per case (decode_rows of every node).
usage: python tools/bench_rows_update.py [--N 1000000] [--K 64] [--steps 5] [--warmup 1] [--out profiles/r32_rows_update.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--batches", default="1000,100000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_rows_update.json"))
    args = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import CompactRows, EfLists, RocLists, update_rows

    N, K = args.N, args.K
    rows = torch.from_numpy(synth.make_graph_rows(N, K)).cuda()
    ctx = _lib.default_context()
    results = []
    for cname, cls in (("compact", CompactRows), ("elias-fano", EfLists), ("roc", RocLists)):
        obj = cls.encode_rows(rows)
        for m in [int(x) for x in args.batches.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(m)
            for grow in (False, True):
                n_new = N + m if grow else N
                nodes = (torch.arange(N, n_new, device="cuda") if grow else torch.randperm(N, generator=g, device="cuda")[:m]).long()
                # batch rows: rows of other nodes of the graph (ids below N <= n_new, real degree distribution)
                batch = rows[torch.randperm(N, generator=g, device="cuda")[:m]].contiguous()

                def update():
                    return update_rows(obj, nodes, batch, n_new=n_new)

                def rebuild():
                    full = obj.decode_rows(None, K, want_counts=False)[0]
                    if grow:
                        full = torch.cat([full, torch.full((m, K), -1, dtype=torch.int32, device="cuda")])
                    full[nodes] = batch
                    return cls.encode_rows(full)

                t_u, t_r, k_u = [], [], []
                for it in range(args.warmup + args.steps):
                    a, u = wall_ms(update)
                    ku = ctx.last_kernel_ms()
                    b, r = wall_ms(rebuild)
                    if it == 0:  # (against the encoder on the updated INPUT rows: a ROC decode of a lossy reference case is not its input)
                        want = torch.cat([rows, torch.full((m, K), -1, dtype=torch.int32, device="cuda")]) if grow else rows.clone()
                        want[nodes] = batch
                        ref = cls.encode_rows(want)
                        du, dr = u.decode_rows(None, K, want_counts=False)[0], ref.decode_rows(None, K, want_counts=False)[0]
                        assert torch.equal(du, dr), f"{cname}: update_rows and encode_rows of the updated rows disagree"
                        del du, dr, ref, want
                    del u, r
                    if it >= args.warmup:
                        t_u.append(a); t_r.append(b); k_u.append(ku)
                rec = dict(codec=cname, N=N, K=K, batch=m, n_new=n_new, update_rows_ms=round(float(np.median(t_u)), 3),
                           update_rows_kernel_ms=round(float(np.median(k_u)), 3), rebuild_ms=round(float(np.median(t_r)), 3))
                rec["speedup"] = round(rec["rebuild_ms"] / rec["update_rows_ms"], 2)
                results.append(rec)
                print(json.dumps(rec), flush=True)
        del obj
    out = dict(workload=f"{N} x {K} graph rows (synth.make_graph_rows)", timing=f"wall ms, median of {args.steps}, arms alternating",
               device=torch.cuda.get_device_name(0), results=results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
