"""Append against rebuild: a batch of (list number, id) pairs added to an existing compressed object.

  arm "append"            new, labels = obj.append(list_nos, ids)   (vidc_*_append_dev)
  arm "append_no_labels"  the same call with labels=False: Elias-Fano and ROC then need no permutation of the touched lists (the
                          rebuild arm computes no labels either)
  arm "rebuild"           decode_all, a torch merge on the device, *_encode_dev / vidc_wt_build_dev on the merged CSR: only entry points that
                          existed before the append calls, i.e. what a caller had to write without them

Per shape, codec, batch size and batch draw the arms alternate in one process (warm-up first); recorded per arm: the median wall
time (perf_counter, synchronised on both sides) and the median of ctx.last_kernel_ms() (append: the library's figure for the call;
rebuild: decode + encode).  Batch draws: "size" = lists drawn in proportion to their length (what new vectors of the same distribution
do), "short" = only lists no longer than the median.  After the timed steps the two arms' objects are compared once (append against rebuild: decoded ids,
compressed size, and the ROC stream).  For ROC the append's phase times and chain launches are recorded too.

  python tools/bench_append.py [--shapes s1,uniform_16m] [--codecs packed,ef,wt,roc] [--steps 5] [--out profiles/r09_append.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s1,uniform_16m")
    ap.add_argument("--codecs", default="packed,ef,wt,roc")
    ap.add_argument("--batches", default="1000,10000,100000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_append.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists, WaveletTreeLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    batches = [int(x) for x in a.batches.split(",")]
    nmax = max(batches)

    def build(codec, off, ids, ntotal_max):
        if codec == "packed":
            return PackedLists.encode(off, ids, bits=PackedLists.bits_for(ntotal_max))
        if codec == "ef":
            return EfLists.encode(off, ids)
        if codec == "wt":
            return WaveletTreeLists.build(off, ids)
        return RocLists.encode(off, ids)

    def rebuild(codec, old, d_old_off, ln, add, bits):
        """-> (object, kernel ms): what a caller writes from decode_all, torch and the device-offsets encoders"""
        dec = old.decode_all()
        km = ctx.last_kernel_ms()
        nlist = d_old_off.numel() - 1
        cnt = torch.bincount(ln, minlength=nlist)
        add_off = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
        new_off = d_old_off + add_off
        merged = torch.empty(dec.numel() + ln.numel(), dtype=torch.int64, device=dec.device)
        l_old = torch.repeat_interleave(torch.arange(nlist, device=dec.device), d_old_off[1:] - d_old_off[:-1])
        merged[torch.arange(dec.numel(), device=dec.device) + add_off[l_old]] = dec
        order = torch.sort(ln, stable=True).indices  # batch order inside a list
        ls = ln[order]
        rank = torch.arange(ln.numel(), device=dec.device) - add_off[ls]
        merged[d_old_off[ls + 1] + add_off[ls] + rank] = add[order]
        if codec == "packed":
            obj = PackedLists.encode(new_off, merged, bits=bits)
        elif codec == "ef":
            obj = EfLists.encode(new_off, merged)
        elif codec == "wt":
            obj = WaveletTreeLists.build(new_off, merged)
        else:
            obj = RocLists.encode(new_off, merged)
        return obj, km + ctx.last_kernel_ms()

    res = dict(tool="tools/bench_append.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               arms=dict(append="obj.append (vidc_*_append_dev), labels returned", append_no_labels="obj.append(labels=False)",
                         rebuild="decode_all + torch merge + *_encode_dev"), rows=[])
    for shape in a.shapes.split(","):
        w = synth.workload(shape)
        ids = torch.from_numpy(w["ids"].view(np.int64)).cuda() if isinstance(w["ids"], np.ndarray) else w["ids"]
        off = w["offsets"]
        sizes = (off[1:] - off[:-1]).astype(np.int64)
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        rng = np.random.default_rng(909)
        short = np.flatnonzero(sizes <= np.median(sizes))
        for codec in a.codecs.split(","):
            old = build(codec, off, ids, w["ntotal"] + nmax)
            bits = old.bits if codec == "packed" else None
            for n in batches:
                for draw in ("size", "short"):
                    lists = rng.choice(sizes.size, n, p=sizes / sizes.sum()) if draw == "size" else rng.choice(short, n)
                    ln = torch.from_numpy(lists.astype(np.int64)).cuda()
                    add = torch.arange(w["ntotal"], w["ntotal"] + n, dtype=torch.int64, device="cuda")
                    ARMS = ("append", "append_no_labels", "rebuild")
                    wall, kern = {k: [] for k in ARMS}, {k: [] for k in ARMS}
                    objs, extra = {}, {}
                    for it in range(a.warmup + a.steps):
                        for arm in ARMS:
                            objs.pop(arm, None)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if arm != "rebuild":
                                obj, _ = old.append(ln, add, labels=arm == "append")
                                km = ctx.last_kernel_ms()
                            else:
                                obj, km = rebuild(codec, old, d_off, ln, add, bits)
                            torch.cuda.synchronize()
                            t1 = time.perf_counter()
                            objs[arm] = obj
                            if arm == "append" and codec == "roc":
                                extra = dict(phase_ms=dict(encode=round(ctx.phase_ms(0), 4), compact=round(ctx.phase_ms(1), 4),
                                                           decode=round(ctx.phase_ms(2), 4), encode_chain=round(ctx.phase_ms(3), 4),
                                                           decode_chain=round(ctx.phase_ms(4), 4)),
                                             chain_encode=ctx.chain_info(0), chain_decode=ctx.chain_info(1))
                            if it >= a.warmup:
                                wall[arm].append(1e3 * (t1 - t0))
                                kern[arm].append(km)
                    x, y = objs["append"], objs["rebuild"]
                    equal = bool(torch.equal(x.decode_all(), y.decode_all()))
                    if codec == "wt":
                        equal = equal and x.size_in_bytes == y.size_in_bytes
                    else:
                        equal = equal and x.compressed_bytes == y.compressed_bytes
                    if codec == "roc":
                        equal = equal and bool(np.array_equal(x.all_words(), y.all_words()))
                    row = dict(shape=shape, codec=codec, n_add=n, draw=draw, touched_lists=int(np.unique(lists).size),
                               longest_touched=int(sizes[np.unique(lists)].max()), objects_equal=equal)
                    for arm in ARMS:
                        row[arm] = dict(wall_ms=round(float(np.median(wall[arm])), 4), last_kernel_ms=round(float(np.median(kern[arm])), 4),
                                        wall_ms_all=[round(v, 4) for v in wall[arm]])
                    row["wall_ratio_rebuild_over_append"] = round(row["rebuild"]["wall_ms"] / row["append"]["wall_ms"], 3)
                    row.update(extra)
                    res["rows"].append(row)
                    print(json.dumps({k: v for k, v in row.items() if k not in ("phase_ms", "chain_encode", "chain_decode")}), flush=True)
                    objs.clear()
            del old
        res.setdefault("shapes", []).append(dict(shape=shape, describe=w["describe"], nlist=w["nlist"], ntotal=w["ntotal"],
                                                 max_list=w["max_list"], median_list=w["median_list"],
                                                 short_lists=int(short.size)))
        del ids, d_off
        torch.cuda.empty_cache()
        _lib.check(_lib.lib().vidc_ctx_trim(ctx.h, None))
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
