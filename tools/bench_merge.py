"""Merging two compressed list objects over the same lists: the device merge against what a caller has without it.

  arm "merge"    merge.merge(a, b, add_id): vidc_*_merge_dev
  arm "append"   what the parent commit offers: b.decode_all(), a repeat_interleave of list numbers, a.append(list_nos, ids + add_id)
                 (vidc_*_append_dev: a stable sort of the whole batch by list number first)
  arm "encode"   decode_all of both, the torch placement of b's lists behind a's (index arithmetic over the two offset arrays), and the
                 from-scratch encoder on device offsets (*_encode_dev)

Inputs are device-resident in every arm.  Per (workload, split, codec) the three arms alternate in one process behind one warm-up
round; recorded per arm: every wall time (perf_counter, ending in a synchronise), their median, minimum and maximum, and for the
merge and the append vidc_ctx_last_kernel_ms of the last step.  After the timed steps the three results are compared: decode_all of
each and, for the merge against the from-scratch encode, compressed_bytes (results_equal).  Splits of a workload's ids into two
objects: "id" -- by id parity, every list on both sides --, and "list" -- by list parity, every list one-sided, so ROC re-encodes
nothing (add_id 0 in both: the halves hold different ids).  The wavelet tree holds a permutation of 0 .. ntotal - 1, ascending
inside every list: its halves are renumbered (every id becomes its rank inside its half, every list is sorted) and merged with
add_id = ntotal(a).  No threshold: every arm is reported, also where the merge loses.

  python tools/bench_merge.py [--workloads s1,zipf_16m] [--codecs roc,ef,packed,wt] [--steps 5] [--out profiles/r38_merge.json]
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


def split(off, ids, how):
    """-> ((off_a, ids_a), (off_b, ids_b)): numpy offsets, ids in list order"""
    off = np.asarray(off, dtype=np.int64)
    sizes = off[1:] - off[:-1]
    lists = np.repeat(np.arange(sizes.size), sizes)
    to_b = (ids & 1).astype(bool) if how == "id" else (lists & 1).astype(bool)
    out = []
    for sel in (~to_b, to_b):
        cnt = np.bincount(lists[sel], minlength=sizes.size)
        out.append((np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), ids[sel]))
    return out


def renumber(off, ids):
    """what a wavelet tree takes: the rank of every id inside the object, ascending inside every list"""
    off = np.asarray(off, dtype=np.int64)
    rank = np.empty(ids.size, np.int64)
    rank[np.argsort(ids, kind="stable")] = np.arange(ids.size)
    lists = np.repeat(np.arange(off.size - 1), off[1:] - off[:-1])
    return rank[np.lexsort((rank, lists))].astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="s1,zipf_16m")
    ap.add_argument("--codecs", default="roc,ef,packed,wt")
    ap.add_argument("--splits", default="id,list")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r38_merge.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, merge, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists, WaveletTreeLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_merge.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=1,
               arms=dict(merge="merge.merge (vidc_*_merge_dev)", append="b.decode_all + repeat_interleave + a.append (vidc_*_append_dev)",
                         encode="decode_all of both + torch placement + *_encode_dev"), rows=[])
    classes = dict(roc=RocLists, ef=EfLists, packed=PackedLists, wt=WaveletTreeLists)

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
        ids = (ids.cpu().numpy() if hasattr(ids, "cpu") else np.asarray(ids)).view(np.uint64)
        bits = PackedLists.bits_for(int(ids.max()) + 1)
        for how in a.splits.split(","):
            (off_a, ids_a), (off_b, ids_b) = split(off, ids, how)
            d_off = [torch.from_numpy(o.astype(np.int64)).cuda() for o in (off_a, off_b)]
            sizes = [o[1:] - o[:-1] for o in d_off]
            new_off = d_off[0] + d_off[1]
            lists_b = torch.repeat_interleave(torch.arange(sizes[1].numel(), device="cuda"), sizes[1])
            for codec in a.codecs.split(","):
                cls = classes[codec]
                kw = dict(bits=bits) if codec == "packed" else {}
                halves = ((off_a, ids_a), (off_b, ids_b))
                if codec == "wt":
                    halves = tuple((o, renumber(o, i)) for o, i in halves)
                build = cls.build if codec == "wt" else cls.encode
                add_id = int(ids_a.size) if codec == "wt" else 0
                objs = [build(o, torch.from_numpy(i.view(np.int64)).cuda(), **kw) for o, i in halves]

                def arm_merge():
                    return merge.merge(objs[0], objs[1], add_id)

                def arm_append():
                    d = objs[1].decode_all()
                    ln = torch.repeat_interleave(torch.arange(sizes[1].numel(), device="cuda"), sizes[1])
                    return objs[0].append(ln, d + add_id, labels=False)[0]

                def arm_encode():
                    da, db = objs[0].decode_all(), objs[1].decode_all()
                    out = torch.empty(da.numel() + db.numel(), dtype=torch.int64, device="cuda")
                    la = torch.repeat_interleave(torch.arange(sizes[0].numel(), device="cuda"), sizes[0])
                    out[torch.arange(da.numel(), device="cuda") + d_off[1][la]] = da
                    out[torch.arange(db.numel(), device="cuda") + d_off[0][lists_b + 1]] = db + add_id
                    return build(new_off, out, **kw)

                arms = dict(merge=arm_merge, append=arm_append, encode=arm_encode)
                for fn in arms.values():  # the warm-up round
                    timed(fn)
                wall = {k: [] for k in arms}
                kernel = {}
                last = {}
                for _ in range(a.steps):
                    for k, fn in arms.items():
                        last[k], ms = timed(fn)
                        wall[k].append(ms)
                        if k != "encode":
                            kernel[k] = round(ctx.last_kernel_ms(), 4)
                dec = {k: v.decode_all() for k, v in last.items()}
                size = lambda o: o.size_in_bytes if codec == "wt" else o.compressed_bytes
                equal = dict(merge_vs_encode=bool(torch.equal(dec["merge"], dec["encode"])
                                                  and size(last["merge"]) == size(last["encode"])),
                             merge_vs_append=bool(torch.equal(dec["merge"], dec["append"])
                                                  and size(last["merge"]) == size(last["append"])))
                row = dict(workload=wname, describe=describe, split=how, codec=codec, ntotal_a=int(ids_a.size), ntotal_b=int(ids_b.size),
                           nlist=int(off_a.size - 1), wall_ms={k: spread(v) for k, v in wall.items()}, last_kernel_ms=kernel,
                           results_equal=equal)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                del objs, last, dec
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
