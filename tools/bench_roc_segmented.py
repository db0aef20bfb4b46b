"""Segmented ROC lists (vidc_rocseg) against the plain ROC object -> profiles/r33_roc_segmented.json.

Shapes: S1 (10^6 ids, 1024 Zipf lists, longest 52 114) and 16.8 M ids in 65 536 Zipf lists (capped at 65 536).  Inputs are device-resident
(offsets and ids as CUDA tensors: vidc_roc_encode_dev / vidc_rocseg_encode_dev).  Arms: the plain object under VIDC_PREC_REFERENCE and
VIDC_PREC_EXACT (the yardstick), the segmented object at T = 1024 / 2048 / 4096 / 8192.  The arms ALTERNATE inside every repetition of
one process; medians of --steps repetitions behind --warmup, with min and max (the run-to-run spread the choice of
VIDC_ROCSEG_DEFAULT_IDS is judged by).  Per arm: wall and kernel ms (vidc_ctx_last_kernel_ms) of encode, of decode_all and of
translate_labels on 10^4 x 20 labels drawn as tools/bench_device_requests.py draws them (list by size, offset uniform, seed 1234: the
label set of profiles/r07_device_requests.txt); bytes per id; the partition kernels' share of the encode's kernel time
(VIDC_PHASE_ROCSEG_PARTITION).  Every arm's decode_all is compared with the input as a set, its translate with its own decode_all.

  python tools/bench_roc_segmented.py [--shapes s1,zipf_16m] [--seg-ids 1024,2048,4096,8192] [--steps 5] [--warmup 1] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s1,zipf_16m")
    ap.add_argument("--seg-ids", default="1024,2048,4096,8192")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_roc_segmented.json"))
    a = ap.parse_args()

    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import RocLists, RocSegLists

    ctx = _lib.default_context()
    seg_ids = [int(t) for t in a.seg_ids.split(",")]
    arms = [("plain-reference", lambda o, i: RocLists.encode(o, i, precision_mode=_lib.VIDC_PREC_REFERENCE)),
            ("plain-exact", lambda o, i: RocLists.encode(o, i, precision_mode=_lib.VIDC_PREC_EXACT))]
    arms += [(f"segmented-{t}", (lambda t: lambda o, i: RocSegLists.encode(o, i, seg_ids=t))(t)) for t in seg_ids]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0), ctx.last_kernel_ms()

    result = dict(tool="tools/bench_roc_segmented.py", steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), shapes={})
    for shape in a.shapes.split(","):
        if shape == "s1":
            off, ids = synth.make_lists_numpy(1_000_000, 1024, 0.75, 42)
            d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
        elif shape == "zipf_16m":
            off, d_ids = synth.make_lists_torch(1 << 24, 1 << 16, 0.75, 42, cap=65536)
        else:
            raise ValueError(shape)
        d_off = torch.from_numpy(off.view(np.int64)).cuda()
        sizes = torch.from_numpy((off[1:] - off[:-1]).astype(np.int64)).cuda()
        ntotal = int(off[-1])
        g = torch.Generator(device="cuda").manual_seed(1234)
        nq, k = 10_000, 20
        l = torch.multinomial(sizes.double() / sizes.sum(), nq * k, replacement=True, generator=g)
        o = (torch.rand(nq * k, device="cuda", generator=g, dtype=torch.float64) * sizes[l].double()).long()
        labels = ((l << 32) | o).contiguous()
        label_pos = torch.from_numpy(off[:-1].view(np.int64)).cuda()[l] + o
        sorted_ids = torch.sort(d_ids).values
        rec = {name: dict(encode_wall=[], encode_kernel=[], partition_kernel=[], decode_wall=[], decode_kernel=[], translate_wall=[],
                          translate_kernel=[]) for name, _ in arms}
        out_buf = torch.empty(ntotal, dtype=torch.int64, device="cuda")
        for it in range(a.warmup + a.steps):
            for name, enc in arms:
                obj, ew, ek = timed(lambda: enc(d_off, d_ids))
                part = ctx.phase_ms(_lib.VIDC_PHASE_ROCSEG_PARTITION) if name.startswith("segmented") else 0.0
                dec, dw, dk = timed(lambda: obj.decode_all(out=out_buf))
                tr, tw, tk = timed(lambda: obj.translate_labels(labels))
                r = rec[name]
                if it == 0:  # checked once per arm
                    lossless = bool(torch.equal(torch.sort(dec).values, sorted_ids))
                    r["lossless"] = lossless  # (plain-reference loses the ids of lists whose maximum is a power of two)
                    assert lossless or name == "plain-reference", name
                    assert torch.equal(tr, dec[label_pos]), name
                    r["bytes_per_id"] = obj.compressed_bytes / ntotal
                    r["compressed_bytes"] = obj.compressed_bytes
                    if name.startswith("segmented"):
                        sf, _ = obj.seg_info()
                        r["inner_lists"], r["universe_bits"] = int(sf[-1]), obj.universe_bits
                        r["longest_segment"] = int(obj.inner.info()["sizes"].max())
                if it >= a.warmup:
                    for key, v in (("encode_wall", ew), ("encode_kernel", ek), ("partition_kernel", part), ("decode_wall", dw),
                                   ("decode_kernel", dk), ("translate_wall", tw), ("translate_kernel", tk)):
                        r[key].append(v)
                del obj, dec, tr
        shape_out = dict(ntotal=ntotal, nlist=int(off.size - 1), longest_list=int(sizes.max().item()), labels=nq * k, arms={})
        for name, _ in arms:
            r = rec[name]
            arm = {key: (stats(v) if isinstance(v, list) else v) for key, v in r.items()}
            if name.startswith("segmented"):
                arm["partition_share_of_encode_kernel"] = arm["partition_kernel"]["median"] / arm["encode_kernel"]["median"]
            else:
                del arm["partition_kernel"]
            shape_out["arms"][name] = arm
        base = shape_out["arms"]["plain-exact"]
        for name, arm in shape_out["arms"].items():
            arm["speedup_vs_plain_exact"] = {key: base[key]["median"] / arm[key]["median"] for key in
                                             ("encode_wall", "decode_wall", "translate_wall", "encode_kernel", "decode_kernel", "translate_kernel")}
            arm["speedup_vs_plain_exact"]["encode_plus_decode_wall"] = (base["encode_wall"]["median"] + base["decode_wall"]["median"]) / (
                arm["encode_wall"]["median"] + arm["decode_wall"]["median"])
            arm["size_vs_plain_exact"] = arm["compressed_bytes"] / base["compressed_bytes"]
        result["shapes"][shape] = shape_out
        print(f"## {shape}: {ntotal} ids, {off.size - 1} lists, longest {shape_out['longest_list']}")
        print(f"{'arm':18s} {'enc wall':>9s} {'enc kern':>9s} {'part':>7s} {'dec wall':>9s} {'dec kern':>9s} {'tr wall':>8s} {'tr kern':>8s} {'B/id':>7s}")
        for name, arm in shape_out["arms"].items():
            m = lambda key: arm[key]["median"]
            print(f"{name:18s} {m('encode_wall'):9.3f} {m('encode_kernel'):9.3f} {arm.get('partition_kernel', dict(median=0))['median']:7.3f} "
                  f"{m('decode_wall'):9.3f} {m('decode_kernel'):9.3f} {m('translate_wall'):8.3f} {m('translate_kernel'):8.3f} {arm['bytes_per_id']:7.4f}",
                  flush=True)
        del d_ids, d_off, out_buf, sorted_ids
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(a.out)


if __name__ == "__main__":
    main()
