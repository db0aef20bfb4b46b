"""Rank inside compressed Elias-Fano lists and graph rows (vidc_ef_rank_dev) against what a caller has without it.

List arms, per (workload, batch), alternating in one process (warm-up first), inputs device-resident:
  "rank"      rank.rank(obj, list_nos, ids, found=...): the search inside the compressed lists, no scratch
  "locate"    locate.locate(obj, list_nos, ids): vidc_ef_locate_dev in pairs mode (decode_all into 8 * ntotal bytes of scratch, a sort of
              the batch, the mark and label kernels)
  "baseline"  obj.decode_all(), the keys list << 32 | id over the decoded array (ascending as a whole: every list is, and the ids of
              these workloads lie below 2^32) and one torch.searchsorted of the batch's keys
Graph arms on the 10^6 x 64 rows of BASELINE configs[3]:
  "has_edges" EliasFanoNSGGraph.has_edges(u, v)
  "decode"    decode_rows of the u (CUDA nodes) and a torch compare against v
Recorded per arm: every wall time (perf_counter, ending in a synchronise), median, minimum and maximum; the device span between two
events; whether the arms agree; and the scratch the locate arm allocates (8 * ntotal bytes for the decoded ids) next to the rank's 0.
No threshold: every arm is reported, also where it loses.

  python tools/bench_ef_rank.py [--workloads s1,zipf_16m,graph] [--steps 5] [--out profiles/r40_ef_rank.json]
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
    ap.add_argument("--workloads", default="s1,zipf_16m,graph")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r40_ef_rank.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, altid, locate, rank, synth
    from vector_db_id_compression_amd.codecs import EfLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_ef_rank.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               arms=dict(rank="rank.rank with found (vidc_ef_rank_dev)", locate="locate.locate in pairs mode (vidc_ef_locate_dev)",
                         baseline="decode_all + torch.searchsorted inside each pair's list (device-resident throughout)",
                         has_edges="EliasFanoNSGGraph.has_edges", decode="decode_rows of the u + torch compare with v"),
               rows=[])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)

    def run(arms, row, agree):
        wall = {k: [] for k in arms}
        span = {k: [] for k in arms}
        got = {}
        for it in range(a.warmup + a.steps):
            for arm, fn in arms.items():
                got[arm], ms, ev = timed(fn)
                if it >= a.warmup:
                    wall[arm].append(ms)
                    span[arm].append(ev)
        row["results_equal"] = bool(agree(got))
        for arm in arms:
            row[arm] = dict(wall_ms=spread(wall[arm]), device_span_ms=spread(span[arm]))
        first = next(iter(arms))
        for arm in list(arms)[1:]:
            row[f"wall_ratio_{arm}_over_{first}"] = round(row[arm]["wall_ms"]["median"] / row[first]["wall_ms"]["median"], 3)
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

    for wname in a.workloads.split(","):
        if wname == "graph":
            rows = synth.make_graph_rows()
            N, K = rows.shape
            g = altid.EliasFanoNSGGraph(torch.from_numpy(rows).cuda())
            rng = np.random.default_rng(40)
            for n in (1000, 100_000):
                u = rng.integers(0, N, n)
                deg = (rows[u] >= 0).sum(axis=1)
                v = np.where(rng.random(n) < 0.5, rows[u, rng.integers(0, 1 << 30, n) % deg], rng.integers(0, N, n))  # half of them edges
                d_u, d_v = torch.from_numpy(u).cuda(), torch.from_numpy(v.astype(np.int64)).cuda()

                def decode():
                    r = g.get_neighbors_device(d_u)
                    return (r == d_v[:, None].to(torch.int32)).any(dim=1)

                run(dict(has_edges=lambda: g.has_edges(d_u, d_v), decode=decode),
                    dict(workload="graph", describe=f"{N} x {K} graph rows (BASELINE configs[3])", batch=f"{n} (u, v) pairs, half of them edges",
                         n_pairs=n, rank_scratch_bytes=0, decode_output_bytes=int(n) * K * 4),
                    lambda got: torch.equal(got["has_edges"], got["decode"]) and bool(got["has_edges"].any()))
            del g
            continue
        if wname == "zipf_16m":
            off, ids = synth.make_lists_torch(1 << 24, 1 << 16, 0.75, 42, cap=65536)
            describe = "16.8M ids in 65536 Zipf(s=0.75) lists capped at 65536"
        else:
            w = synth.workload(wname)
            off, ids, describe = w["offsets"], w["ids"], w["describe"]
        d_ids = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
        o = off.astype(np.int64)
        sizes = o[1:] - o[:-1]
        nlist, ntotal = sizes.size, int(o[-1])
        d_off = torch.from_numpy(o).cuda()
        list_of = torch.repeat_interleave(torch.arange(nlist, device="cuda"), torch.from_numpy(sizes).cuda())
        rng = np.random.default_rng(40)
        short = np.flatnonzero(sizes < np.median(sizes))
        short_pos = np.concatenate([np.arange(o[l], o[l + 1]) for l in short]) if short.size else np.zeros(0, np.int64)
        longest = int(np.argmax(sizes))
        batches = [(f"{n} pairs from lists below the median length", rng.choice(short_pos, min(n, short_pos.size), replace=False))
                   for n in (1000, 100_000)]
        if wname == "s1":
            batches.append((f"1000 pairs inside the longest list ({int(sizes[longest])} ids)",
                            o[longest] + rng.choice(int(sizes[longest]), 1000, replace=False)))
        obj = EfLists.encode(off, d_ids)
        dec = obj.decode_all()
        assert bool(((dec >= 0) & (dec < (1 << 32))).all()) and nlist < (1 << 30)  # (the baseline's keys: list << 32 | id)
        for bname, pos in batches:
            d_pos = torch.from_numpy(pos).cuda()
            d_want, d_ln = dec[d_pos].clone(), list_of[d_pos].clone()  # every pair hits
            found = torch.empty(pos.size, dtype=torch.uint8, device="cuda")

            def baseline():
                # every list is ascending and the ids lie below 2^32: list << 32 | id ascends over the whole decoded array
                keys = (list_of << 32) | obj.decode_all()
                return torch.searchsorted(keys, (d_ln << 32) | d_want) - d_off[d_ln]

            def do_rank():
                return rank.rank(obj, d_ln, d_want, found=found)

            def do_locate():
                return locate.locate(obj, d_ln, d_want) & 0xFFFFFFFF  # (every pair hits: the label's offset is the rank)

            run(dict(rank=do_rank, locate=do_locate, baseline=baseline),
                dict(workload=wname, describe=describe, batch=bname, n_pairs=int(pos.size), nlist=nlist, ntotal=ntotal,
                     lists_touched=int(np.unique(np.searchsorted(o, pos, side="right") - 1).size), rank_scratch_bytes=0,
                     locate_scratch_bytes_decoded_ids=8 * ntotal),
                lambda got: torch.equal(got["rank"], got["locate"]) and torch.equal(got["rank"], got["baseline"]) and bool(found.all()))
        del obj, dec
        torch.cuda.empty_cache()
        _lib.check(_lib.lib().vidc_ctx_trim(ctx.h, None))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
