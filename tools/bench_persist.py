"""Loading an image against rebuilding from raw input: what a restart costs with and without persist.

  arm "import"   persist.wt_from_image / persist.compact_from_image on the image arrays resident on the host (vidc_wt_import /
                 vidc_compact_import): wall time, and the library's split of it into the host -> device copies of the image
                 (ctx.phase_ms(5), hipEvents) and the kernels that rebuild the derived tables and check the image (ctx.last_kernel_ms())
  arm "rebuild"  the same object built from the raw ids / rows resident on the host: their upload and WaveletTreeLists.build /
                 CompactRows.encode_rows -- what a restart costs without an image (and what needs the raw input kept)

Per object the two arms alternate in one process (warm-up first); recorded per arm: every wall time (perf_counter, synchronised on
both sides), their median, minimum and maximum.  Once per object: the export (persist.wt_image / compact_image) and save / load wall
times and the file's bytes; after the timed steps the imported object is compared with the rebuilt one (decode, size).

  python tools/bench_persist.py [--objects wt0,wt1,compact] [--steps 5] [--out profiles/r13_persist.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4),
                all=[round(float(x), 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", default="wt0,wt1,compact")
    ap.add_argument("--wt-shape", default="uniform_16m")
    ap.add_argument("--rows", default="1000000x64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_persist.json"))
    a = ap.parse_args()
    import torch

    from vector_db_id_compression_amd import _lib, persist, synth
    from vector_db_id_compression_amd.codecs import CompactRows, WaveletTreeLists

    torch.cuda.set_device(0)
    ctx = _lib.default_context()
    res = dict(tool="tools/bench_persist.py", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup,
               arms=dict(**{"import": "vidc_*_import of the image arrays on the host (h2d_ms + kernel_ms inside wall_ms)"},
                         rebuild="upload of the raw ids / rows from the host + build / encode_rows"), rows=[])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def run(name, describe, raw_bytes, rebuild, export, from_image, equal):
        obj, _ = timed(rebuild)
        image, export_ms = timed(lambda: export(obj))
        with tempfile.TemporaryDirectory() as d:
            path, save_ms = timed(lambda: persist.save(obj, os.path.join(d, name)))
            file_bytes = os.path.getsize(path)
            loaded, load_ms = timed(lambda: persist.load(path))
            del loaded
        wall = {"import": [], "rebuild": []}
        h2d, kern, rkern = [], [], []
        objs = {}
        for it in range(a.warmup + a.steps):
            for arm in ("import", "rebuild"):
                objs.pop(arm, None)
                o, ms = timed((lambda: from_image(image)) if arm == "import" else rebuild)
                objs[arm] = o
                if it >= a.warmup:
                    wall[arm].append(ms)
                    if arm == "import":
                        h2d.append(ctx.phase_ms(5))
                        kern.append(ctx.last_kernel_ms())
                    else:
                        rkern.append(ctx.last_kernel_ms())
        row = dict(object=name, describe=describe, raw_input_bytes=int(raw_bytes), file_bytes=int(file_bytes),
                   size_in_bytes=int(obj.size_in_bytes), export_wall_ms=round(export_ms, 4), save_wall_ms=round(save_ms, 4),
                   load_wall_ms=round(load_ms, 4), objects_equal=bool(equal(objs["import"], objs["rebuild"])))
        row["import"] = dict(wall_ms=spread(wall["import"]), h2d_ms=spread(h2d), kernel_ms=spread(kern))
        row["rebuild"] = dict(wall_ms=spread(wall["rebuild"]), last_kernel_ms=spread(rkern))
        row["wall_ratio_rebuild_over_import"] = round(row["rebuild"]["wall_ms"]["median"] / row["import"]["wall_ms"]["median"], 3)
        res["rows"].append(row)
        print(json.dumps({k: v for k, v in row.items()}), flush=True)
        objs.clear()
        del obj, image
        torch.cuda.empty_cache()
        _lib.check(_lib.lib().vidc_ctx_trim(ctx.h, None))

    objects = a.objects.split(",")
    if any(o.startswith("wt") for o in objects):
        w = synth.workload(a.wt_shape)
        ids = w["ids"].cpu().numpy().view(np.uint64) if not isinstance(w["ids"], np.ndarray) else w["ids"]
        off = w["offsets"]
        for wt_type in (0, 1):
            if f"wt{wt_type}" not in objects:
                continue
            run(f"wt{wt_type}", f"wavelet tree wt_type {wt_type}: {w['describe']}", ids.nbytes + off.nbytes,
                lambda: WaveletTreeLists.build(off, torch.from_numpy(ids.view(np.int64)).cuda(), wt_type=wt_type),
                persist.wt_image,
                lambda im: persist.wt_from_image(im["offsets"], im["wt_type"], im["bits"], im["cls"], im["offs"], im["off_bits"]),
                lambda x, y: bool(torch.equal(x.decode_all(), y.decode_all())) and x.size_in_bytes == y.size_in_bytes)
        del ids, w
    if "compact" in objects:
        N, K = (int(v) for v in a.rows.split("x"))
        rows = synth.make_graph_rows(N, K)
        run("compact", f"compact graph rows {N} x {K}, degree ~ U[{K // 2}, {K}]", rows.nbytes,
            lambda: CompactRows.encode_rows(torch.from_numpy(rows).cuda()), persist.compact_image,
            lambda im: persist.compact_from_image(N, K, im),
            lambda x, y: bool(torch.equal(x.decode_rows(None, want_counts=False)[0], y.decode_rows(None, want_counts=False)[0]))
            and x.size_in_bytes == y.size_in_bytes)
    doc = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
