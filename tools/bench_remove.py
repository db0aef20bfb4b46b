"""Removing a batch of ids from a compressed container: the device remove against the rebuild a caller has without it.

  arm "pairs"    removal.remove(obj, list_nos, ids): vidc_*_remove_dev in pairs mode
  arm "any"      removal.remove(obj, None, ids): any-list mode (Faiss's remove_ids over an IDSelectorBatch)
  arm "rebuild"  what a caller has today: obj.decode_all(), a torch.isin mask, the new offsets from a segmented count, and the codec's
                 device-offsets encoder (vidc_*_encode_dev) on the survivors

Inputs are device-resident in every arm.  Per (workload, codec, batch) the three arms alternate in one process (warm-up first);
recorded per arm: every wall time (perf_counter, ending in a synchronise), their median, minimum and maximum, and
vidc_ctx_last_kernel_ms of the call (rebuild: decode + encode).  Batches: pairs drawn from the lists below the median length (every pair
hits), and one batch inside the longest list of S1.  After the timed steps the three results are compared (decode_all, ntotal).

  python tools/bench_remove.py [--workloads s1,zipf_16m] [--codecs roc,ef,packed] [--steps 5] [--out profiles/r25_remove.json]
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
    ap.add_argument("--codecs", default="roc,ef,packed")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_remove.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, removal, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_remove.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               arms=dict(pairs="removal.remove in pairs mode", any="removal.remove in any-list mode",
                         rebuild="decode_all + torch.isin mask + *_encode_dev on the survivors (device-resident throughout)"), rows=[])
    classes = dict(roc=RocLists, ef=EfLists, packed=PackedLists)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

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
        rng = np.random.default_rng(25)
        short = np.flatnonzero(sizes < np.median(sizes))
        short_pos = np.concatenate([np.arange(o[l], o[l + 1]) for l in short]) if short.size else np.zeros(0, np.int64)
        longest = int(np.argmax(sizes))
        batches = [(f"{n} pairs from lists below the median length", rng.choice(short_pos, min(n, short_pos.size), replace=False))
                   for n in (1000, 100_000)]
        if wname == "s1":
            batches.append((f"1000 pairs inside the longest list ({int(sizes[longest])} ids)",
                            o[longest] + rng.choice(int(sizes[longest]), 1000, replace=False)))
        for cname in a.codecs.split(","):
            cls = classes[cname]
            obj = cls.encode(off, d_ids)
            dec = obj.decode_all()
            for bname, pos in batches:
                d_pos = torch.from_numpy(np.sort(pos)).cuda()
                d_rm, d_ln = dec[d_pos].clone(), list_of[d_pos].clone()  # ids in the object's own order: every pair hits
                new = {}

                def rebuild():
                    all_ids = obj.decode_all()
                    ms = ctx.last_kernel_ms()
                    keep = ~torch.isin(all_ids, d_rm)
                    kills = torch.zeros(nlist, dtype=torch.int64, device="cuda").index_add_(0, list_of, (~keep).to(torch.int64))
                    new_off = d_off - torch.cat([kills.new_zeros(1), torch.cumsum(kills, 0)])
                    out = cls.encode(new_off, all_ids[keep], **({'bits': obj.bits} if cname == 'packed' else {}))
                    rebuild.kernel_ms = ms + ctx.last_kernel_ms()
                    return out

                arms = dict(pairs=lambda: removal.remove(obj, d_ln, d_rm, removed=True)[0],
                            any=lambda: removal.remove(obj, None, d_rm, removed=True)[0], rebuild=rebuild)
                wall = {k: [] for k in arms}
                kern = {k: [] for k in arms}
                for it in range(a.warmup + a.steps):
                    for arm, fn in arms.items():
                        new.pop(arm, None)
                        new[arm], ms = timed(fn)
                        if it >= a.warmup:
                            wall[arm].append(ms)
                            kern[arm].append(rebuild.kernel_ms if arm == "rebuild" else ctx.last_kernel_ms())
                ref = new["rebuild"].decode_all()
                row = dict(workload=wname, describe=describe, codec=cname, batch=bname, n_pairs=int(pos.size), nlist=nlist, ntotal=ntotal,
                           lists_touched=int(np.unique(np.searchsorted(o, pos, side="right") - 1).size),
                           results_equal=bool(all(new[k].ntotal == ntotal - pos.size and torch.equal(new[k].decode_all(), ref) for k in arms)))
                for arm in arms:
                    row[arm] = dict(wall_ms=spread(wall[arm]), kernel_ms=spread(kern[arm]))
                for arm in ("pairs", "any"):
                    row[f"wall_ratio_rebuild_over_{arm}"] = round(row["rebuild"]["wall_ms"]["median"] / row[arm]["wall_ms"]["median"], 3)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                new.clear()
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
