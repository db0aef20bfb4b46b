"""Host offsets vs device offsets (vidc_*_encode_dev) for packed bits and Elias-Fano: one step = encode + decode_all.

Per shape, codec and offsets kind: the median of separately timed steps (as bench.py's secondaries) of
  wall_ms    -- perf_counter around the step, synchronised on both sides,
  kernel_ms  -- ctx.last_kernel_ms() of the encode + that of the decode,
  host_ms    -- wall_ms - kernel_ms.
The decoded ids are checked against the input after the timed steps.  Prints one JSON document; --out writes it to a file.

  python tools/bench_dev_offsets.py [--shapes s2,uniform_16m,s1] [--steps 7] [--out profiles/r07_dev_offsets.json]
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
    ap.add_argument("--shapes", default="s2,uniform_16m,s1")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, synth
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_dev_offsets.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup, shapes=[])
    for shape in a.shapes.split(","):
        w = synth.workload(shape, seed=1042)
        ids = torch.from_numpy(w["ids"].view(np.int64)).cuda() if isinstance(w["ids"], np.ndarray) else w["ids"]
        h_off = w["offsets"]
        d_off = torch.from_numpy(h_off.view(np.int64)).cuda()
        out = torch.empty(w["ntotal"], dtype=torch.int64, device="cuda")
        entry = dict(shape=shape, describe=w["describe"], nlist=w["nlist"], ntotal=w["ntotal"], codecs={})
        for name, cls in (("packed", PackedLists), ("ef", EfLists)):
            row = {}
            for kind, off in (("host", h_off), ("device", d_off)):
                wall, kern = [], []
                obj = None
                for it in range(a.warmup + a.steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    obj = cls.encode(off, ids, ctx=ctx)
                    ke = ctx.last_kernel_ms()
                    obj.decode_all(out)
                    kd = ctx.last_kernel_ms()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if it >= a.warmup:
                        wall.append(1e3 * (t1 - t0))
                        kern.append(ke + kd)
                ok = bool(torch.equal(out, ids))
                wm, km = float(np.median(wall)), float(np.median(kern))
                row[kind] = dict(wall_ms=round(wm, 4), kernel_ms=round(km, 4), host_ms=round(wm - km, 4),
                                 wall_ms_all=[round(x, 4) for x in wall], kernel_ms_all=[round(x, 4) for x in kern], correct=ok)
                del obj
            row["kernel_ratio_device_over_host"] = round(row["device"]["kernel_ms"] / row["host"]["kernel_ms"], 4)
            entry["codecs"][name] = row
            print(json.dumps({shape: {name: {k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if not kk.endswith("_all")})
                                             for k, v in row.items()}}}), flush=True)
        res["shapes"].append(entry)
        del ids, d_off, out
        torch.cuda.empty_cache()
        _lib.check(_lib.lib().vidc_ctx_trim(ctx.h, None))
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
