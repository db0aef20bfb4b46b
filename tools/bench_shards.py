"""The single-process sharded container (vidc_shards, sharding.DeviceShards) against the unsharded objects, ALL CONTEXTS ON ONE DEVICE.

Nothing here measures scaling over GPUs: the container has never been run on more than one.  What is recorded:

  copy    the cut (inside encode) and its inverse (inside decode_all): kernel time on the home stream (hipEvents, the home context's
          last_kernel_ms) against a device-to-device copy of the same bytes in the same process (torch's contiguous copy_, which
          issues hipMemcpyAsync device-to-device on the current stream), alternating; median of
          --steps with min-max.  The cut and the copy both read and write 8 bytes per id.
  wall    encode + decode_all, and translate_labels of --labels labels, for 1 / 2 / 4 / 8 shards against the unsharded object
          (perf_counter, device synchronised on both sides); packed bits and Elias-Fano at every shard count, ROC once (--roc-shards).

Recorded, not gated.

  python tools/bench_shards.py [--steps 5] [--out profiles/r15_shards.json]
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
    ap.add_argument("--labels", type=int, default=200_000)
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--roc-shards", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_shards.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists
    from vector_db_id_compression_amd.sharding import DeviceShards

    torch.cuda.set_device(0)
    off, ids = synth.make_lists_torch(a.ids, a.nlist, a.zipf, 42, cap=65536)
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    torch.cuda.synchronize()
    home = _lib.Context(0)
    ctxs = [_lib.Context(0) for _ in range(8)]
    res = dict(tool="tools/bench_shards.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               caveat="every context on ONE device; never run on more than one GPU; no scaling figure follows from this file",
               workload=dict(ids=int(off[-1]), nlist=int(a.nlist), zipf=a.zipf, max_list=int(sizes.max()), median_list=int(np.median(sizes)),
                             lists_of_one_id=int((sizes == 1).sum()), bytes=int(off[-1]) * 8), copy=[], wall=[])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def memcpy_ms():
        dst = torch.empty_like(ids)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = torch.cuda.current_stream()
        e0.record(st)
        dst.copy_(ids)  # contiguous, same dtype, same device: torch issues hipMemcpyAsync(..., hipMemcpyDeviceToDevice, stream)
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # -- the cut and its inverse against the plain copy, alternating (packed bits: the cheapest codec around them)
    nbytes = int(off[-1]) * 8
    for ns in [int(s) for s in a.shards.split(",")]:
        cut, uncut, copy = [], [], []
        for it in range(a.warmup + a.steps):
            S = DeviceShards.encode("packed", off, ids, ctxs=ctxs[:ns], home=home)
            c = home.last_kernel_ms()
            out = S.decode_all()
            u = home.last_kernel_ms()
            m = memcpy_ms()
            if it >= a.warmup:
                cut.append(c), uncut.append(u), copy.append(m)
            if it == 0:
                assert torch.equal(out, ids), "decode_all of the sharded object is not its input"
            del S, out
        row = dict(nshards=ns, cut_ms=spread(cut), uncut_ms=spread(uncut), memcpy_d2d_ms=spread(copy),
                   cut_gb_s=round(2 * nbytes / np.median(cut) / 1e6, 1), uncut_gb_s=round(2 * nbytes / np.median(uncut) / 1e6, 1),
                   memcpy_gb_s=round(2 * nbytes / np.median(copy) / 1e6, 1))
        row["cut_rate_over_memcpy"] = round(np.median(copy) / np.median(cut), 3)
        row["uncut_rate_over_memcpy"] = round(np.median(copy) / np.median(uncut), 3)
        res["copy"].append(row)
        print(json.dumps(row), flush=True)

    # -- wall times against the unsharded object
    rng = np.random.default_rng(3)
    lists = rng.integers(0, a.nlist, a.labels)
    lists = lists[sizes[lists] > 0]
    labels = torch.from_numpy((lists << 32) | (rng.random(lists.size) * sizes[lists]).astype(np.int64)).cuda()
    single = dict(packed=PackedLists, ef=EfLists, roc=RocLists)

    def arm(kind, ns):
        enc, dec, tr = [], [], []
        for it in range(a.warmup + a.steps):
            if ns == 0:
                obj, e = timed(lambda: single[kind].encode(off, ids))
            else:
                obj, e = timed(lambda: DeviceShards.encode(kind, off, ids, ctxs=ctxs[:ns], home=home))
            out, d = timed(obj.decode_all)
            got, t = timed(lambda: obj.translate_labels(labels))
            if it >= a.warmup:
                enc.append(e), dec.append(d), tr.append(t)
            del obj, out, got
        row = dict(kind=kind, nshards=ns if ns else "unsharded", encode_wall_ms=spread(enc), decode_all_wall_ms=spread(dec),
                   encode_plus_decode_all_wall_ms=spread(np.add(enc, dec)), translate_wall_ms=spread(tr), labels=int(labels.numel()))
        res["wall"].append(row)
        print(json.dumps(row), flush=True)

    for kind in ("packed", "ef"):
        for ns in [0] + [int(s) for s in a.shards.split(",")]:
            arm(kind, ns)
    arm("roc", 0)
    arm("roc", a.roc_shards)
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
