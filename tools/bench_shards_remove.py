"""Removing a batch from a sharded object (sharding.DeviceShards.remove, vidc_remove_sharded_dev), ALL CONTEXTS ON ONE DEVICE.

Nothing here measures scaling over GPUs: the container has never been run on more than one, and on ONE device sharding can only cost.
The path of a shard on another device (staging through hipMemcpyAsync) is NOT RUN by this tool.  What is recorded, per codec, batch size
and mode (pairs / any-list), the arms alternating inside every step (warm-up first), wall ms (perf_counter, device synchronised on both
sides), median of --steps with min-max:

  unsharded   removal.remove(obj, list_nos | None, ids) on the unsharded object      (vidc_*_remove_dev)
  sharded_N   DeviceShards.remove at N = 1 / 2 / 4 / 8 shards                        (vidc_remove_sharded_dev)
  rebuild     the only way before the sharded remove existed: decode_all of the sharded object, a torch.isin mask and a segmented count
              on the device, DeviceShards.encode of the survivors (a fresh LPT partition and a fresh cut), at --rebuild-shards shards

and the home context's last_kernel_ms after a sharded remove (route + mask inverse cut + join).  Every arm writes the removed mask and the
missing / invalid counters.  The pairs come from the lists below the median length, as in tools/bench_remove.py, and every pair hits; the
ids of the workload are distinct over the whole object, so the any-list batch removes the same entries.  After the timed steps every
arm's result is compared with the unsharded one (decode_all, ntotal, compressed_bytes; the sharded arms' masks and counters too).

Recorded, not gated.

  python tools/bench_shards_remove.py [--steps 5] [--out profiles/r30_shards_remove.json]
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
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1 << 24)
    ap.add_argument("--nlist", type=int, default=1 << 16)
    ap.add_argument("--zipf", type=float, default=0.75)
    ap.add_argument("--batches", default="1000,100000")
    ap.add_argument("--codecs", default="packed,ef,roc")
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--rebuild-shards", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_shards_remove.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, removal, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists
    from vector_db_id_compression_amd.sharding import DeviceShards

    torch.cuda.set_device(0)
    off, ids = synth.make_lists_torch(a.ids, a.nlist, a.zipf, 42, cap=65536)
    o = off.astype(np.int64)
    sizes = o[1:] - o[:-1]
    ntotal = int(o[-1])
    d_ids = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    d_off = torch.from_numpy(o).cuda()
    list_of = torch.repeat_interleave(torch.arange(a.nlist, device="cuda"), torch.from_numpy(sizes).cuda())
    torch.cuda.synchronize()
    home = _lib.Context(0)
    ctxs = [_lib.Context(0) for _ in range(8)]
    shard_counts = [int(s) for s in a.shards.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
    bits = PackedLists.bits_for(ntotal)
    short = np.flatnonzero(sizes < np.median(sizes))
    short_pos = np.concatenate([np.arange(o[l], o[l + 1]) for l in short])
    res = dict(tool="tools/bench_shards_remove.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               caveat="every context on ONE device; never run on more than one GPU; no scaling figure follows from this file; the path of a "
                      "shard on another device is not run",
               workload=dict(ids=ntotal, nlist=int(a.nlist), zipf=a.zipf, max_list=int(sizes.max()), median_list=int(np.median(sizes)),
                             short_lists=int(short.size), packed_bits=bits),
               arms=dict(unsharded="removal.remove (vidc_*_remove_dev)", sharded_N="DeviceShards.remove at N shards (vidc_remove_sharded_dev)",
                         rebuild=f"decode_all + torch.isin + DeviceShards.encode at {a.rebuild_shards} shards"),
               wall=[])

    def args(kind):
        return dict(bits=bits) if kind == "packed" else {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def counters():
        return torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    def rebuild(kind, S, rm):
        dec = S.decode_all()
        gone = torch.isin(dec, rm)
        kills = torch.zeros(a.nlist, dtype=torch.int64, device="cuda").index_add_(0, list_of, gone.to(torch.int64))
        new_off = d_off - torch.cat([kills.new_zeros(1), torch.cumsum(kills, 0)])
        keep = dec[~gone]
        torch.cuda.synchronize()  # (the shard contexts run on streams of their own)
        return DeviceShards.encode(kind, new_off, keep, ctxs=ctxs[: a.rebuild_shards], home=home, **args(kind)), gone.to(torch.uint8)

    single = dict(packed=PackedLists, ef=EfLists, roc=RocLists)
    rng = np.random.default_rng(3030)
    for kind in a.codecs.split(","):
        U = single[kind].encode(off, d_ids, **args(kind))
        dec = U.decode_all()
        S = {ns: DeviceShards.encode(kind, off, d_ids, ctxs=ctxs[:ns], home=home, **args(kind)) for ns in shard_counts}
        if a.rebuild_shards not in S:
            S[a.rebuild_shards] = DeviceShards.encode(kind, off, d_ids, ctxs=ctxs[: a.rebuild_shards], home=home, **args(kind))
        for n in batches:
            pos = torch.from_numpy(np.sort(rng.choice(short_pos, min(n, short_pos.size), replace=False))).cuda()
            rm, ln_pairs = dec[pos].clone(), list_of[pos].clone()  # ids in the object's own order: every pair hits
            for mode in ("pairs", "any"):
                ln = ln_pairs if mode == "pairs" else None
                arms = ["unsharded"] + [f"sharded_{ns}" for ns in shard_counts] + ["rebuild"]
                wall = {k: [] for k in arms}
                home_ms = {ns: [] for ns in shard_counts}
                objs, masks, counts = {}, {}, {}
                for it in range(a.warmup + a.steps):
                    for arm in arms:
                        objs.pop(arm, None)
                        miss, inv = counters()
                        if arm == "unsharded":
                            (obj, mask), ms = timed(lambda: removal.remove(U, ln, rm, removed=True, missing=miss, invalid=inv))
                        elif arm == "rebuild":
                            (obj, mask), ms = timed(lambda: rebuild(kind, S[a.rebuild_shards], rm))
                        else:
                            ns = int(arm.split("_")[1])
                            (obj, mask), ms = timed(lambda: S[ns].remove(ln, rm, removed=True, missing=miss, invalid=inv))
                            if it >= a.warmup:
                                home_ms[ns].append(home.last_kernel_ms())
                        objs[arm], masks[arm], counts[arm] = obj, mask, (int(miss.item()), int(inv.item()))
                        if it >= a.warmup:
                            wall[arm].append(ms)
                want = objs["unsharded"].decode_all()
                equal = {}
                for arm in arms[1:]:
                    ok = objs[arm].ntotal == ntotal - pos.numel() and bool(torch.equal(objs[arm].decode_all(), want))
                    ok = ok and objs[arm].compressed_bytes == objs["unsharded"].compressed_bytes and bool(torch.equal(masks[arm], masks["unsharded"]))
                    equal[arm] = ok and (arm == "rebuild" or counts[arm] == counts["unsharded"] == (0, 0))
                row = dict(kind=kind, mode=mode, n_rm=int(pos.numel()), touched_lists=int(torch.unique(ln_pairs).numel()), results_equal=equal,
                           wall_ms={arm: spread(wall[arm]) for arm in arms},
                           home_kernel_ms={f"sharded_{ns}": spread(home_ms[ns]) for ns in shard_counts},
                           loads_after={f"sharded_{ns}": [int(x) for x in objs[f"sharded_{ns}"].loads] for ns in shard_counts})
                res["wall"].append(row)
                print(json.dumps({k: v for k, v in row.items() if k != "loads_after"}), flush=True)
                objs.clear(), masks.clear()
        del U, S, dec
        torch.cuda.empty_cache()
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
