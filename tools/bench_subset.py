"""Subsets of compressed list objects (Faiss's copy_subset_to): the device subset against what a caller has without it.

  arm "subset"   subset.subset(obj, subset_type, a1, a2): vidc_*_subset_dev
  arm "rebuild"  decode_all, the predicate in torch (on the ids, or on list numbers and positions made by repeat_interleave over the
                 offsets), boolean indexing, a bincount of the taken entries' list numbers for the new offsets, and the from-scratch
                 encoder on device offsets (*_encode_dev)

Inputs are device-resident in both arms (the list number and the position of every entry are built once, outside the timed region).
Per (workload, case, codec) the two arms alternate in one process behind one warm-up round; recorded per arm: every wall time
(perf_counter, ending in a synchronise), their median, minimum and maximum, and for the subset vidc_ctx_last_kernel_ms of the last
step.  After the timed steps the two results are compared: decode_all of each and compressed_bytes (results_equal).  Cases: ID_MOD at
a1 = 2 and 8, ID_RANGE of half the id space, INVLIST_FRACTION 0 of 4, INVLIST of the lower half.  No threshold: every arm is reported,
also where the subset loses.

  python tools/bench_subset.py [--workloads s1,zipf_16m] [--codecs roc,ef,packed] [--steps 5] [--out profiles/r39_subset.json]

The mark kernels side by side (k_sub_mark_id for ID_MOD against k_rm_mark on the same decoded data) come from a kernel trace:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o g -- python tools/bench_subset.py --probe --workloads zipf_16m
  python tools/bench_subset.py ... --kernel-stats DIR/.../g_kernel_stats.csv      # copies the two kernels' rows into the result
"""
import argparse
import csv
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


def load(wname):
    from vector_db_id_compression_amd import synth

    if wname == "zipf_16m":
        off, ids = synth.make_lists_torch(1 << 24, 1 << 16, 0.75, 42, cap=65536)
        describe = "16.8M ids in 65536 Zipf(s=0.75) lists capped at 65536"
    else:
        w = synth.workload(wname)
        off, ids, describe = w["offsets"], w["ids"], w["describe"]
    ids = (ids.cpu().numpy() if hasattr(ids, "cpu") else np.asarray(ids)).view(np.uint64)
    return off, ids, describe


def mark_rows(path):
    """the rows of a rocprofv3 kernel_stats.csv that name the two mark kernels: name, calls, average ns"""
    out = []
    for r in list(csv.reader(open(path)))[1:]:
        for k in ("k_sub_mark_id", "k_rm_mark"):
            if k in r[0]:
                out.append(dict(kernel=k, calls=int(r[1]), avg_us=round(float(r[3]) / 1e3, 2)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="s1,zipf_16m")
    ap.add_argument("--codecs", default="roc,ef,packed")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--probe", action="store_true", help="only run packed-bits ID_MOD subsets and an any-list remove (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --probe run: its mark kernels go into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r39_subset.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, removal, subset
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    classes = dict(roc=RocLists, ef=EfLists, packed=PackedLists)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    if a.probe:
        for wname in a.workloads.split(","):
            off, ids, _ = load(wname)
            obj = PackedLists.encode(off, torch.from_numpy(ids.view(np.int64)).cuda(), bits=PackedLists.bits_for(int(ids.max()) + 1))
            batch = torch.from_numpy(ids[:: max(1, ids.size // 1024)].view(np.int64).copy()).cuda()
            for _ in range(3):
                subset.subset(obj, subset.ID_MOD, 2, 1)
                subset.subset(obj, subset.ID_MOD, 8, 3)
                subset.subset(obj, subset.ID_MOD, 3, 1)
                removal.remove(obj, None, batch)
            torch.cuda.synchronize()
        return

    res = dict(tool="tools/bench_subset.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=1,
               arms=dict(subset="subset.subset (vidc_*_subset_dev)",
                         rebuild="decode_all + torch predicate + boolean index + bincount + *_encode_dev"), rows=[])
    for wname in a.workloads.split(","):
        off, ids, describe = load(wname)
        nlist, T = off.size - 1, int(ids.size)
        bits = PackedLists.bits_for(int(ids.max()) + 1)
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        sizes = d_off[1:] - d_off[:-1]
        lists = torch.repeat_interleave(torch.arange(nlist, device="cuda"), sizes)
        pos = torch.arange(T, device="cuda") - d_off[lists]
        half_id = int(np.median(ids))
        cases = [("id_mod_2", subset.ID_MOD, 2, 1), ("id_mod_8", subset.ID_MOD, 8, 3), ("id_range_half", subset.ID_RANGE, 0, half_id),
                 ("fraction_0_of_4", subset.INVLIST_FRACTION, 4, 0), ("invlist_lower_half", subset.INVLIST, 0, nlist // 2)]
        for codec in a.codecs.split(","):
            cls = classes[codec]
            kw = dict(bits=bits) if codec == "packed" else {}
            obj = cls.encode(off, torch.from_numpy(ids.view(np.int64)).cuda(), **kw)
            for cname, t, a1, a2 in cases:
                def arm_subset():
                    return subset.subset(obj, t, a1, a2, taken=False)[0]

                def arm_rebuild():
                    d = obj.decode_all()
                    if t == subset.ID_MOD:
                        mask = d % a1 == a2
                    elif t == subset.ID_RANGE:
                        mask = (d >= a1) & (d < a2)
                    elif t == subset.INVLIST_FRACTION:
                        i1, i2 = sizes * a2 // a1, sizes * (a2 + 1) // a1
                        mask = (pos >= i1[lists]) & (pos < i2[lists])
                    else:
                        mask = (lists >= a1) & (lists < a2)
                    cnt = torch.bincount(lists[mask], minlength=nlist)
                    new_off = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)])
                    return cls.encode(new_off, d[mask], **kw)

                arms = dict(subset=arm_subset, rebuild=arm_rebuild)
                for fn in arms.values():  # the warm-up round
                    timed(fn)
                wall = {k: [] for k in arms}
                last, kernel = {}, None
                for _ in range(a.steps):
                    for k, fn in arms.items():
                        last[k], ms = timed(fn)
                        wall[k].append(ms)
                        if k == "subset":
                            kernel = round(ctx.last_kernel_ms(), 4)
                dec = {k: v.decode_all() for k, v in last.items()}
                equal = bool(torch.equal(dec["subset"], dec["rebuild"]) and last["subset"].compressed_bytes == last["rebuild"].compressed_bytes)
                row = dict(workload=wname, describe=describe, case=cname, subset_type=t, a1=a1, a2=a2, codec=codec, ntotal=T, nlist=nlist,
                           n_taken=int(last["subset"].ntotal), wall_ms={k: spread(v) for k, v in wall.items()},
                           subset_last_kernel_ms=kernel, results_equal=equal)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                del last, dec
            del obj
    if a.kernel_stats:
        res["mark_kernels"] = dict(how="rocprofv3 --kernel-trace --stats of `--probe --workloads zipf_16m` (packed bits, 16.8M decoded ids): "
                                       "k_sub_mark_id over ID_MOD a1 = 2, 8, 3 (three calls each); k_rm_mark: any-list remove of 1024 ids",
                                   rows=mark_rows(a.kernel_stats))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
