"""Re-balancing a sharded object (sharding.DeviceShards.rebalance, vidc_rebalance_sharded), ALL CONTEXTS ON ONE DEVICE.

Nothing here measures scaling over GPUs: one device, no scaling figure.  The path of a source shard on another device (a temporary
object, its copy through hipMemcpyAsync) is NOT RUN by this tool.  The workload is skewed first: --pairs (list, id) pairs are appended
into lists that shard 0 owns (DeviceShards.append keeps the map), so the re-balance has a drift to undo.  What is recorded, per codec and
shard count, the two arms alternating inside every step (warm-up first), wall ms (perf_counter, device synchronised on both sides),
median of --steps with min-max:

  rebalance   DeviceShards.rebalance()                                                  (vidc_rebalance_sharded)
  rebuild     the only way before it existed: decode_all of the skewed object and DeviceShards.encode of the result with its offsets

the home context's last_kernel_ms and the largest last_kernel_ms among the shard contexts after a rebalance, moved_ids, and whether the two
arms agree: same_map (owner, local numbers, loads) and, per arm, arm_equal (ntotal, compressed_bytes and decode_all against the skewed
object's own); results_equal is all of them.  For ROC also the word-copy kernel
of one vidc_roc_regroup over every list of the unsharded object in a shuffled order (vidc_ctx_phase_ms, VIDC_PHASE_ROC_REGROUP_COPY)
against a device-to-device copy of the same bytes (hipEvents around Tensor.copy_), median of --steps.

Recorded, not gated.

  python tools/bench_shards_rebalance.py [--steps 5] [--out profiles/r31_shards_rebalance.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASE_REGROUP_COPY = 6


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=1 << 24)
    ap.add_argument("--nlist", type=int, default=1 << 16)
    ap.add_argument("--zipf", type=float, default=0.75)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--codecs", default="packed,ef,roc")
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_shards_rebalance.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import PackedLists, RocLists, roc_regroup
    from vector_db_id_compression_amd.sharding import DeviceShards

    torch.cuda.set_device(0)
    off, ids = synth.make_lists_torch(a.ids, a.nlist, a.zipf, 42, cap=65536)
    o = off.astype(np.int64)
    sizes = o[1:] - o[:-1]
    ntotal = int(o[-1])
    d_ids = ids if torch.is_tensor(ids) else torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    torch.cuda.synchronize()
    home = _lib.Context(0)
    ctxs = [_lib.Context(0) for _ in range(8)]
    shard_counts = [int(s) for s in a.shards.split(",")]
    # the batch ids lie above every id of the workload: distinct inside every list.  They start behind a power of two: a list whose
    # largest id is one is lossy in the reference ROC codec (VIDC_PREC_REFERENCE), and what such a list decodes to encodes to another
    # stream, so the rebuild arm would no longer answer as the skewed object does (the re-balance, which copies the stream, would)
    top = int(d_ids.max().item()) + 1
    while any(top <= (1 << b) < top + a.pairs for b in range(64)):
        top = max((1 << b) + 1 for b in range(64) if top <= (1 << b) < top + a.pairs)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3131)
    bits = PackedLists.bits_for(top + a.pairs)
    res = dict(tool="tools/bench_shards_rebalance.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               caveat="every context on ONE device: one device, no scaling figure; the path of a source shard on another device is not run",
               workload=dict(ids=ntotal, nlist=int(a.nlist), zipf=a.zipf, max_list=int(sizes.max()), skew_pairs=a.pairs, packed_bits=bits),
               arms=dict(rebalance="DeviceShards.rebalance (vidc_rebalance_sharded)", rebuild="decode_all + DeviceShards.encode of the skewed object"),
               wall=[])

    def args(kind):
        return dict(bits=bits) if kind == "packed" else {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def rebuild(kind, S1, d_off):
        dec = S1.decode_all()
        torch.cuda.synchronize()  # (the shard contexts run on streams of their own)
        return DeviceShards.encode(kind, d_off, dec, ctxs=S1.ctxs, home=home, **args(kind))

    rng = np.random.default_rng(3131)
    for kind in a.codecs.split(","):
        for ns in shard_counts:
            S = DeviceShards.encode(kind, off, d_ids, ctxs=ctxs[:ns], home=home, **args(kind))
            # (lists that stay below the 65 536 ids up to which the reference ROC codec reproduces its input)
            mine = np.flatnonzero((S.owner == 0) & (sizes < 32768))
            ln = torch.from_numpy(mine[rng.integers(0, mine.size, a.pairs)].astype(np.int64)).cuda()
            add = (top + torch.randperm(a.pairs, device="cuda", generator=gen)).to(torch.int64)
            torch.cuda.synchronize()
            S1, _ = S.append(ln, add, labels=False)
            del S
            d_off = torch.from_numpy(S1.offsets.astype(np.int64)).cuda()
            want = S1.decode_all().clone()
            loads_before = [int(x) for x in S1.loads]
            wall = dict(rebalance=[], rebuild=[])
            home_ms, shard_ms = [], []
            objs, moved = {}, 0
            for it in range(a.warmup + a.steps):
                for arm in ("rebalance", "rebuild"):
                    objs.pop(arm, None)
                    if arm == "rebalance":
                        (obj, moved), ms = timed(lambda: S1.rebalance())
                        if it >= a.warmup:
                            home_ms.append(home.last_kernel_ms())
                            shard_ms.append(max(c.last_kernel_ms() for c in ctxs[:ns]))
                    else:
                        obj, ms = timed(lambda: rebuild(kind, S1, d_off))
                    objs[arm] = obj
                    if it >= a.warmup:
                        wall[arm].append(ms)
            R, B = objs["rebalance"], objs["rebuild"]
            same_map = bool(np.array_equal(R.owner, B.owner)) and bool(np.array_equal(R.local_no, B.local_no)) and bool(np.array_equal(R.loads, B.loads))
            arm_equal = {arm: o.ntotal == S1.ntotal and o.compressed_bytes == S1.compressed_bytes and bool(torch.equal(o.decode_all(), want))
                         for arm, o in (("rebalance", R), ("rebuild", B))}  # each arm against the skewed object itself
            equal = same_map and all(arm_equal.values())
            row = dict(kind=kind, shards=ns, moved_ids=int(moved), results_equal=equal, same_map=same_map, arm_equal=arm_equal,
                       wall_ms={k: spread(v) for k, v in wall.items()},
                       home_kernel_ms=spread(home_ms), max_shard_kernel_ms=spread(shard_ms), loads_before=loads_before,
                       loads_after=[int(x) for x in R.loads])
            res["wall"].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.startswith("loads")}), flush=True)
            objs.clear()
            del S1, R, B, want
            torch.cuda.empty_cache()
    if "roc" in a.codecs.split(","):
        # the regroup's word copy against a device-to-device copy of the same bytes
        ctx = ctxs[0]
        U = RocLists.encode(off, d_ids, ctx=ctx)
        order = np.random.default_rng(7).permutation(a.nlist).astype(np.uint64)
        words = U.total_words
        src = torch.empty(words, dtype=torch.int32, device="cuda")
        dst = torch.empty_like(src)
        copy_ms, d2d_ms, all_ms = [], [], []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            G = roc_regroup([U], np.zeros(a.nlist, np.uint32), order, ctx=ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                copy_ms.append(ctx.phase_ms(PHASE_REGROUP_COPY))
                all_ms.append(ctx.last_kernel_ms())
                d2d_ms.append(e0.elapsed_time(e1))
        same = bool(torch.equal(G.decode_lists(np.arange(64))[0], U.decode_lists(order[:64])[0])) and G.total_words == words
        res["regroup_copy"] = dict(lists=int(a.nlist), words=int(words), bytes=int(words) * 4, order="every list once, shuffled",
                                   word_copy_kernel_ms=spread(copy_ms), regroup_all_kernels_ms=spread(all_ms), d2d_copy_ms=spread(d2d_ms),
                                   results_equal=same)
        print(json.dumps(res["regroup_copy"]), flush=True)
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
