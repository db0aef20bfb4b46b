"""Locating a batch of ids in a compressed container (id -> list << 32 | offset): the device locate against what a caller has without it.

  arm "pairs"     locate.locate(obj, list_nos, ids): vidc_*_locate_dev in pairs mode
  arm "any"       locate.locate(obj, None, ids): any-list mode (Faiss's direct map)
  arm "baseline"  what a caller does today: obj.decode_all(), a stable torch.sort of the ids, torch.searchsorted of the batch, and the
                  label arithmetic over the offsets (device-resident throughout)

Inputs are device-resident in every arm.  Per (workload, codec, batch) the three arms alternate in one process (warm-up first);
recorded per arm: every wall time (perf_counter, ending in a synchronise), their median, minimum and maximum, the device span of the
call between two events on torch's stream, and -- for the locate arms of the codecs whose call waits (packed bits, Elias-Fano, ROC) --
vidc_ctx_last_kernel_ms.  Batches: pairs drawn from the lists below the median length (every pair hits), and for ROC one batch inside
the longest list of S1.  After the timed steps the three label arrays are compared (the workloads hold every id once: both modes and
the baseline must agree).  No threshold: every arm is reported, also where it loses to the baseline.

  python tools/bench_locate.py [--workloads s1,zipf_16m] [--codecs roc,ef,packed,wt] [--steps 5] [--out profiles/r35_locate.json]
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
    ap.add_argument("--workloads", default="s1,zipf_16m")
    ap.add_argument("--codecs", default="roc,ef,packed,wt")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_locate.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, locate, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists, WaveletTreeLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_locate.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               arms=dict(pairs="locate.locate in pairs mode", any="locate.locate in any-list mode",
                         baseline="decode_all + stable torch.sort + torch.searchsorted + label arithmetic (device-resident throughout)"),
               rows=[])
    encoders = dict(roc=RocLists.encode, ef=EfLists.encode, packed=PackedLists.encode, wt=WaveletTreeLists.build)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)

    for wname in a.workloads.split(","):
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
        rng = np.random.default_rng(35)
        short = np.flatnonzero(sizes < np.median(sizes))
        short_pos = np.concatenate([np.arange(o[l], o[l + 1]) for l in short]) if short.size else np.zeros(0, np.int64)
        longest = int(np.argmax(sizes))
        batches = [(f"{n} pairs from lists below the median length", rng.choice(short_pos, min(n, short_pos.size), replace=False), None)
                   for n in (1000, 100_000)]
        if wname == "s1":
            batches.append((f"1000 pairs inside the longest list ({int(sizes[longest])} ids)",
                            o[longest] + rng.choice(int(sizes[longest]), 1000, replace=False), "roc"))
        for cname in a.codecs.split(","):
            obj = encoders[cname](off, d_ids)
            dec = obj.decode_all()
            waits = cname != "wt"  # (the wavelet tree's call only enqueues: it leaves no kernel time behind)
            for bname, pos, only in batches:
                if only and only != cname:
                    continue
                d_pos = torch.from_numpy(pos).cuda()  # batch order: as drawn
                d_want, d_ln = dec[d_pos].clone(), list_of[d_pos].clone()  # ids in the object's own order: every pair hits
                got = {}

                def baseline():
                    all_ids = obj.decode_all()
                    s, order = torch.sort(all_ids, stable=True)  # (stable: of equal ids the first position, the smallest label)
                    at = torch.searchsorted(s, d_want).clamp_(max=ntotal - 1)
                    p = order[at]
                    lists = torch.searchsorted(d_off, p, right=True) - 1
                    return torch.where(s[at] == d_want, (lists << 32) | (p - d_off[lists]), torch.full_like(p, -1))

                arms = dict(pairs=lambda: locate.locate(obj, d_ln, d_want), any=lambda: locate.locate(obj, None, d_want), baseline=baseline)
                wall = {k: [] for k in arms}
                span = {k: [] for k in arms}
                kern = {k: [] for k in arms}
                for it in range(a.warmup + a.steps):
                    for arm, fn in arms.items():
                        got[arm], ms, ev = timed(fn)
                        if it >= a.warmup:
                            wall[arm].append(ms)
                            span[arm].append(ev)
                            if waits and arm != "baseline":
                                kern[arm].append(ctx.last_kernel_ms())
                row = dict(workload=wname, describe=describe, codec=cname, batch=bname, n_pairs=int(pos.size), nlist=nlist, ntotal=ntotal,
                           lists_touched=int(np.unique(np.searchsorted(o, pos, side="right") - 1).size),
                           results_equal=bool(all(torch.equal(got[k], got["baseline"]) for k in arms) and bool((got["any"] >= 0).all())))
                for arm in arms:
                    row[arm] = dict(wall_ms=spread(wall[arm]), device_span_ms=spread(span[arm]),
                                    kernel_ms=spread(kern[arm]) if kern[arm] else None)
                for arm in ("pairs", "any"):
                    row[f"wall_ratio_baseline_over_{arm}"] = round(row["baseline"]["wall_ms"]["median"] / row[arm]["wall_ms"]["median"], 3)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                got.clear()
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
