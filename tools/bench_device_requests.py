"""Device-resident requests against the host-array calls (profiles/r07_device_requests.txt).

Per codec and shape, the median over --steps timed repetitions (after --warmup) of
  wall_ms    -- perf_counter around the request, the stream synchronised on both sides,
  kernel_ms  -- torch CUDA events around it on the current stream (PCIe copies and waits inside the call included).
Sections:
  decode section (C3 shape: 10^4 queries x k on S1 lists, labels made on the device by torch): "gather call only" is the library call
    of the host-array path alone (vidc_*_decode_gather with its request arrays ready on the host: what README's deferred-search row
    and profiles/r06_search_paths.txt time); "host arrays + gather" is what a caller whose labels are on the device pays for it --
    labels to the host, np.unique of the touched lists, the gather call, ids back up; "translate_labels" is the device request.
    k = 20 and 100, and the same on a 16.8 M-id / 65 536-list index;
  ef forms: the Elias-Fano translate kernel alone at n = 2*10^5 and 10^6, in both forms: the 16-lane group form of the default build,
    and (--ef-wave-lib) the wave-per-label form, measured in a child process that loads a library built with
    -DVIDC_EF_TRANSLATE_WAVE=1 (--build-ef-wave PATH builds it; hipcc only, no GPU);
  rows: 10^6 x 64 graph rows, a frontier of 10^4 random nodes, decode_rows with numpy nodes against CUDA nodes;
  search: graph_search.search_batched, 10^3 queries on a knn_graph, the frontier handed over through the host (as before) against
    the CUDA tensor.
Results are checked against each other.
usage: python tools/bench_device_requests.py [--sections a,b] [--ef-wave-lib LIB] [--out FILE]
       python tools/bench_device_requests.py --build-ef-wave LIB
"""
import argparse
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    import torch

    wall, kern = [], []
    r = None
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            wall.append(1e3 * (t1 - t0))
            kern.append(e0.elapsed_time(e1))
    return float(np.median(wall)), float(np.median(kern)), r


def build_codecs(off, ids_np, which):
    from vector_db_id_compression_amd import codecs as cd

    out = {}
    ntotal = int(off[-1])
    for name in which:
        if name == "packed":
            out[name] = cd.PackedLists.encode(off, ids_np, bits=max(cd.PackedLists.bits_for(ntotal), int(ids_np.max()).bit_length()))
        elif name == "ef":
            out[name] = cd.EfLists.encode(off, ids_np)
        elif name == "wt":  # (a permutation of 0..ntotal-1, ascending in every list: ids = positions)
            out[name] = cd.WaveletTreeLists.build(off, np.arange(ntotal, dtype=np.uint64), 0)
        elif name == "roc":
            out[name] = cd.RocLists.encode(off, ids_np)
    return out


def decode_section(lines, shape, off, ids_np, nq, k, steps, warmup, which=("packed", "ef", "wt", "roc")):
    import torch

    sizes = torch.from_numpy((off[1:] - off[:-1]).astype(np.int64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1234)
    objs = build_codecs(off, ids_np, which)
    # labels as a search makes them on the device: list by size (every result inside its list), offset uniform
    p = sizes.double() / sizes.sum()
    l = torch.multinomial(p, nq * k, replacement=True, generator=g)
    o = (torch.rand(nq * k, device="cuda", generator=g, dtype=torch.float64) * sizes[l].double()).long()
    labels = ((l << 32) | o).view(nq, k)
    lines.append(f"\n## decode section: {shape}, {nq} queries x k = {k} ({nq * k} results), labels on the device")
    lines.append(f"{'codec':8s} {'path':22s} {'wall_ms':>9s} {'kernel_ms':>10s}")
    for name, obj in objs.items():
        lab_h = labels.cpu().numpy().reshape(-1)
        g_uniq, g_slot = np.unique((lab_h >> 32).astype(np.uint64), return_inverse=True)
        g_slot, g_off = g_slot.astype(np.uint64), (lab_h & 0xFFFFFFFF).astype(np.uint64)

        def host_path():
            lab = labels.cpu().numpy().reshape(-1)
            ln = (lab >> 32).astype(np.uint64)
            lo = (lab & 0xFFFFFFFF).astype(np.uint64)
            uniq, slot = np.unique(ln, return_inverse=True)
            ids = obj.decode_gather(uniq, slot.astype(np.uint64), lo)
            return torch.from_numpy(ids).cuda().view(nq, k)

        def dev_path():
            return obj.translate_labels(labels)

        wg, kg, rg = timed(lambda: obj.decode_gather(g_uniq, g_slot, g_off), steps, warmup)
        w0, k0, r0 = timed(host_path, steps, warmup)
        w1, k1, r1 = timed(dev_path, steps, warmup)
        assert torch.equal(r0, r1) and np.array_equal(rg, r0.cpu().numpy().reshape(-1)), name
        lines.append(f"{name:8s} {'gather call only':22s} {wg:9.3f} {kg:10.3f}")
        lines.append(f"{name:8s} {'host arrays + gather':22s} {w0:9.3f} {k0:10.3f}")
        lines.append(f"{name:8s} {'translate_labels':22s} {w1:9.3f} {k1:10.3f}")
    return objs


def ef_forms(lines, obj, off, steps, warmup, form):
    import torch

    sizes = torch.from_numpy((off[1:] - off[:-1]).astype(np.int64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(99)
    label = {"group": "16-lane group form, default build", "wave": "wave-per-label form, build with -DVIDC_EF_TRANSLATE_WAVE=1"}[form]
    lines.append(f"\n## Elias-Fano translate kernel alone ({label}), S1 lists")
    for n in (200_000, 1_000_000):
        l = torch.multinomial(sizes.double() / sizes.sum(), n, replacement=True, generator=g)
        o = (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * sizes[l].double()).long()
        lab = (l << 32) | o
        out = torch.empty_like(lab)
        w, kms, _ = timed(lambda: obj.translate_labels(lab, out=out), steps, warmup)
        lines.append(f"n = {n:8d}: wall {w:7.3f} ms, kernel {kms:7.3f} ms")


def rows_section(lines, steps, warmup):
    import torch

    from vector_db_id_compression_amd import codecs as cd
    from vector_db_id_compression_amd import synth

    N, K, m = 1_000_000, 64, 10_000
    rows = synth.make_graph_rows(N, K)
    d_rows = torch.from_numpy(rows).cuda()
    nodes = np.random.default_rng(5).integers(0, N, m).astype(np.int64)
    d_nodes = torch.from_numpy(nodes).cuda()
    lines.append(f"\n## rows: {N} x {K} graph, frontier of {m} random nodes")
    lines.append(f"{'codec':8s} {'nodes':8s} {'wall_ms':>9s} {'kernel_ms':>10s}")
    for name, cls in (("compact", cd.CompactRows), ("ef", cd.EfLists), ("roc", cd.RocLists)):
        obj = cls.encode_rows(d_rows)
        w0, k0, r0 = timed(lambda: obj.decode_rows(nodes.astype(np.uint64), K, want_counts=False)[0], steps, warmup)
        w1, k1, r1 = timed(lambda: obj.decode_rows(d_nodes, K, want_counts=False)[0], steps, warmup)
        assert torch.equal(r0, r1), name
        lines.append(f"{name:8s} {'host':8s} {w0:9.3f} {k0:10.3f}")
        lines.append(f"{name:8s} {'device':8s} {w1:9.3f} {k1:10.3f}")


class _HostFrontier:
    """the frontier handed over as before: CUDA tensor -> numpy (a finished query asks for node 0) -> the graph"""

    def __init__(self, g):
        self.g = g

    def get_neighbors_device(self, nodes):
        import torch

        out = self.g.get_neighbors_device(nodes.clamp(min=0).cpu().numpy())
        return torch.where((nodes >= 0)[:, None], out, torch.full_like(out, -1))


def search_section(lines, steps, warmup):
    from vector_db_id_compression_amd import altid
    from vector_db_id_compression_amd.graph_search import RawGraph, knn_graph, search_batched

    rng = np.random.default_rng(12)
    x = rng.normal(size=(100_000, 32)).astype(np.float32)
    xq = rng.normal(size=(1000, 32)).astype(np.float32)
    rows = knn_graph(x, 32, seed=3)
    lines.append(f"\n## search_batched: {xq.shape[0]} queries, knn_graph of {x.shape[0]} x 32, L = 64, k = 10")
    lines.append(f"{'graph':12s} {'frontier':9s} {'wall_ms':>9s} {'kernel_ms':>10s}")
    graphs = [("raw", RawGraph(rows))] + [(n, c(rows.copy())) for n, c in altid.AVAILABLE_COMPRESSED_GRAPHS.items() if c]
    ref = None
    for name, g in graphs:
        w0, k0, r0 = timed(lambda: search_batched(_HostFrontier(g), x, xq, 10, L=64), steps, warmup)
        w1, k1, r1 = timed(lambda: search_batched(g, x, xq, 10, L=64), steps, warmup)
        ref = r1[1] if ref is None else ref
        assert np.array_equal(r0[1], r1[1]) and np.array_equal(r1[1], ref), name
        lines.append(f"{name:12s} {'host':9s} {w0:9.2f} {k0:10.2f}")
        lines.append(f"{name:12s} {'device':9s} {w1:9.2f} {k1:10.2f}")


def build_ef_wave(path):
    """libvidc built from the same sources with -DVIDC_EF_TRANSLATE_WAVE=1 (vidc_ef_translate_labels_dev runs the wave-per-label form)"""
    import concurrent.futures
    import tempfile

    from vector_db_id_compression_amd import build as b

    hipcc = b.find_hipcc()
    objdir = tempfile.mkdtemp(prefix="vidc_efwave_")

    def one(src):
        o = os.path.join(objdir, os.path.basename(src) + ".o")
        subprocess.check_call([hipcc] + [f for f in b.FLAGS if f != "-shared"] + ["-DVIDC_EF_TRANSLATE_WAVE=1", "-c", src, "-o", o])
        return o

    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            objs = list(ex.map(one, b.sources()))
        subprocess.check_call([hipcc] + b.FLAGS + ["-o", path] + objs)
    finally:
        shutil.rmtree(objdir, ignore_errors=True)
    print(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="c3,c3k100,c16m,ef_forms,rows,search")
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ef-wave-lib", default=None, help="library built with -DVIDC_EF_TRANSLATE_WAVE=1 (ef_forms: the second form)")
    ap.add_argument("--ef-form", default="group", choices=["group", "wave"], help=argparse.SUPPRESS)  # (set for the child process)
    ap.add_argument("--build-ef-wave", default=None, metavar="LIB", help="build that library and exit")
    a = ap.parse_args()
    if a.build_ef_wave:
        build_ef_wave(a.build_ef_wave)
        return
    import torch

    from vector_db_id_compression_amd import _lib, synth

    torch.cuda.set_device(0)
    _lib.default_context()
    sec = a.sections.split(",")
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")
    lines = [f"# tools/bench_device_requests.py on {torch.cuda.get_device_name(0)} ({arch}): medians of {a.steps} steps after {a.warmup}"]
    s1 = synth.workload("s1", seed=1042)
    objs = None
    if "c3" in sec:
        objs = decode_section(lines, "S1 (10^6 ids, 1024 Zipf lists)", s1["offsets"], s1["ids"], 10_000, 20, a.steps, a.warmup)
    if "c3k100" in sec:
        decode_section(lines, "S1 (10^6 ids, 1024 Zipf lists)", s1["offsets"], s1["ids"], 10_000, 100, a.steps, a.warmup)
    if "c16m" in sec:
        w = synth.workload("uniform_16m", seed=1042)
        ids = w["ids"].cpu().numpy().view(np.uint64) if hasattr(w["ids"], "cpu") else w["ids"]
        decode_section(lines, "16.8 M ids in 65 536 lists", w["offsets"], ids, 10_000, 20, a.steps, a.warmup)
    if "ef_forms" in sec:
        ef = objs["ef"] if objs else build_codecs(s1["offsets"], s1["ids"], ["ef"])["ef"]
        ef_forms(lines, ef, s1["offsets"], a.steps, a.warmup, a.ef_form)
        if a.ef_wave_lib:  # the other form, in a process of its own (a library is loaded once per process)
            env = dict(os.environ, VIDC_LIBRARY=os.path.abspath(a.ef_wave_lib))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sections", "ef_forms", "--ef-form", "wave", "--steps",
                                str(a.steps), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, check=True)
            out = r.stdout.strip().split("\n")
            lines.extend([""] + out[out.index(next(x for x in out if x.startswith("## Elias-Fano"))):])
    if "rows" in sec:
        rows_section(lines, a.steps, a.warmup)
    if "search" in sec:
        search_section(lines, max(3, a.steps // 3), 1)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
