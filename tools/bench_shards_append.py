"""Appending a batch to a sharded object (sharding.DeviceShards.append, vidc_sharded_append_dev), ALL CONTEXTS ON ONE DEVICE.

Nothing here measures scaling over GPUs: the container has never been run on more than one, and on ONE device sharding can only cost.
What is recorded, per codec and batch size, the arms alternating inside every step (warm-up first), wall ms (perf_counter, device
synchronised on both sides), median of --steps with min-max:

  unsharded   obj.append(list_nos, ids) on the unsharded object                      (vidc_*_append_dev)
  sharded_N   DeviceShards.append at N = 1 / 2 / 4 / 8 shards                        (vidc_sharded_append_dev)
  rebuild     the only way before the append existed: decode_all of the sharded object, a torch merge on the device,
              DeviceShards.encode of the merged CSR (a fresh LPT partition and a fresh cut), at --rebuild-shards shards

and, separately, the kernel time of route + join (the home context's last_kernel_ms after a sharded append: two hipEvent intervals on the
home stream) against a device-to-device copy that moves the same bytes (torch's contiguous copy_ of half of them: a copy reads and writes
every byte once), alternating.  The batches go to lists no longer than the median length, as tools/bench_append.py's "short" draw.

Recorded, not gated.

  python tools/bench_shards_append.py [--steps 5] [--out profiles/r17_shards_append.json]
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_shards_append.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists
    from vector_db_id_compression_amd.sharding import DeviceShards

    torch.cuda.set_device(0)
    off, ids = synth.make_lists_torch(a.ids, a.nlist, a.zipf, 42, cap=65536)
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    ntotal = int(off[-1])
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()
    home = _lib.Context(0)
    ctxs = [_lib.Context(0) for _ in range(8)]
    shard_counts = [int(s) for s in a.shards.split(",")]
    batches = [int(b) for b in a.batches.split(",")]
    bits = PackedLists.bits_for(ntotal + max(batches))
    short = np.flatnonzero(sizes <= np.median(sizes))
    res = dict(tool="tools/bench_shards_append.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               caveat="every context on ONE device; never run on more than one GPU; no scaling figure follows from this file",
               workload=dict(ids=ntotal, nlist=int(a.nlist), zipf=a.zipf, max_list=int(sizes.max()), median_list=int(np.median(sizes)),
                             short_lists=int(short.size), packed_bits=bits),
               arms=dict(unsharded="obj.append (vidc_*_append_dev)", sharded_N="DeviceShards.append at N shards (vidc_sharded_append_dev)",
                         rebuild=f"decode_all + torch merge + DeviceShards.encode at {a.rebuild_shards} shards"),
               wall=[], route_join=[])

    def args(kind):
        return dict(bits=bits) if kind == "packed" else {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def rebuild(kind, S, ln, add):
        dec = S.decode_all()
        cnt = torch.bincount(ln, minlength=a.nlist)
        add_off = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
        new_off = d_off + add_off
        merged = torch.empty(dec.numel() + ln.numel(), dtype=torch.int64, device=dec.device)
        l_old = torch.repeat_interleave(torch.arange(a.nlist, device=dec.device), d_off[1:] - d_off[:-1])
        merged[torch.arange(dec.numel(), device=dec.device) + add_off[l_old]] = dec
        order = torch.sort(ln, stable=True).indices  # batch order inside a list
        ls = ln[order]
        rank = torch.arange(ln.numel(), device=dec.device) - add_off[ls]
        merged[d_off[ls + 1] + add_off[ls] + rank] = add[order]
        torch.cuda.synchronize()  # (the shard contexts run on streams of their own)
        return DeviceShards.encode(kind, new_off, merged, ctxs=ctxs[: a.rebuild_shards], home=home, **args(kind))

    def copy_ms(nbytes):
        n = max(nbytes // 16, 1)  # int64 elements of half the bytes: the copy reads and writes each once
        src, dst = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream()
        torch.cuda.synchronize()
        e0.record(st)
        dst.copy_(src)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    single = dict(packed=PackedLists, ef=EfLists, roc=RocLists)
    rng = np.random.default_rng(1717)
    for kind in a.codecs.split(","):
        U = single[kind].encode(off, ids, **args(kind))
        S = {ns: DeviceShards.encode(kind, off, ids, ctxs=ctxs[:ns], home=home, **args(kind)) for ns in shard_counts}
        if a.rebuild_shards not in S:
            S[a.rebuild_shards] = DeviceShards.encode(kind, off, ids, ctxs=ctxs[: a.rebuild_shards], home=home, **args(kind))
        for n in batches:
            ln = torch.from_numpy(rng.choice(short, n).astype(np.int64)).cuda()
            add = torch.arange(ntotal, ntotal + n, dtype=torch.int64, device="cuda")
            arms = ["unsharded"] + [f"sharded_{ns}" for ns in shard_counts] + ["rebuild"]
            wall = {k: [] for k in arms}
            rj = {ns: [] for ns in shard_counts}
            cp = {ns: [] for ns in shard_counts}
            moved = {ns: (ns * 8 + 8 + 1) * n + (8 + 8 + 1 + 8) * n for ns in shard_counts}  # route: reads ln, writes ns slots + owner; join
            objs = {}
            for it in range(a.warmup + a.steps):
                for arm in arms:
                    objs.pop(arm, None)
                    if arm == "unsharded":
                        (obj, _), ms = timed(lambda: U.append(ln, add, **args(kind)))
                    elif arm == "rebuild":
                        obj, ms = timed(lambda: rebuild(kind, S[a.rebuild_shards], ln, add))
                    else:
                        ns = int(arm.split("_")[1])
                        (obj, _), ms = timed(lambda: S[ns].append(ln, add, **args(kind)))
                        k_ms, c_ms = home.last_kernel_ms(), copy_ms(moved[ns])
                        if it >= a.warmup:
                            rj[ns].append(k_ms), cp[ns].append(c_ms)
                    objs[arm] = obj
                    if it >= a.warmup:
                        wall[arm].append(ms)
            want = objs["unsharded"].decode_all()
            equal = {arm: bool(torch.equal(objs[arm].decode_all(), want)) and objs[arm].compressed_bytes == objs["unsharded"].compressed_bytes
                     for arm in arms if arm != "unsharded"}
            row = dict(kind=kind, n_add=n, touched_lists=int(torch.unique(ln).numel()), objects_equal=equal,
                       wall_ms={arm: spread(wall[arm]) for arm in arms},
                       loads_after={f"sharded_{ns}": [int(x) for x in objs[f"sharded_{ns}"].loads] for ns in shard_counts})
            res["wall"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "loads_after"}), flush=True)
            if kind == a.codecs.split(",")[0]:  # route and join do not depend on the codec
                for ns in shard_counts:
                    r = dict(n_add=n, nshards=ns, bytes_moved=moved[ns], route_plus_join_kernel_ms=spread(rj[ns]), memcpy_d2d_ms=spread(cp[ns]))
                    res["route_join"].append(r)
                    print(json.dumps(r), flush=True)
            objs.clear()
        del U, S
        torch.cuda.empty_cache()
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
