"""CPU: vidc_ivf_range_count_dev and vidc_ivf_range_fill_dev are declared, listed, exported and loadable and the ABI version stays
100; every limit is VIDC_ERR_INVALID before any device work, with "range" in vidc_last_error, for both calls; nq == 0 and
capacity == 0 return VIDC_OK without a device; the plan header's LDS, resident wavefronts, cut and scratch against written-out
tables, and the one-CU batches of the GPU test run the grid-stride loop past its first trip; IVFIndex keeps exactly its public
methods and the module functions raise without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_range_ref as rr
import ivf_scan_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDC_ERR_INVALID = -1
SYMBOLS = ("vidc_ivf_range_count_dev", "vidc_ivf_range_fill_dev")


def test_symbols_declared_listed_exported_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(dll, name), name
        assert getattr(_lib.lib(), name).restype is ctypes.c_int
    assert len(_lib.lib().vidc_ivf_range_count_dev.argtypes) == 16 and len(_lib.lib().vidc_ivf_range_fill_dev.argtypes) == 18
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS))
    # the new section lies behind the scan's declaration and says what is out of scope, and the limits
    assert hdr.index("vidc_ivf_scan_dev(") < hdr.index("range search over IVF lists") < hdr.index("vidc_ivf_range_count_dev(")
    sec = hdr[hdr.index("range search over IVF lists"):hdr.index("vidc_ivf_range_fill_dev(")]
    for word in ("Per-query radii", "inner product", "residual PQ", "other than 8 bits", "coarse quantiser", "sharded", "one-pass",
                 "Faiss adapter", "d_slot_lims[::nprobe]", "2^32 - 1", "Scratch", "strictly", "capacity"):
        assert word in sec, word


def _calls():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    p = 8  # (never dereferenced)
    ok = dict(ctx=p, nlist=16, off=p, ntotal=2000, codes=p, kind=1, d=128, M=16, cb=p, nq=5, xq=p, nprobe=4, probes=p, radius=1.5, lims=p,
              total=None, capacity=10, D=p, lab=p)

    def head(a):
        return (a["ctx"], a["nlist"], a["off"], a["ntotal"], a["codes"], a["kind"], a["d"], a["M"], a["cb"], a["nq"], a["xq"], a["nprobe"],
                a["probes"], a["radius"])

    def count(**kw):
        a = dict(ok, **kw)
        return L.vidc_ivf_range_count_dev(*head(a), a["lims"], a["total"])

    def fill(**kw):
        a = dict(ok, **kw)
        return L.vidc_ivf_range_fill_dev(*head(a), a["lims"], a["capacity"], a["D"], a["lab"])

    return L, count, fill


def test_limits_are_refused_before_any_device_work():
    L, count, fill = _calls()
    bad = [dict(ctx=None), dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(lims=None),
           dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049), dict(d=2049, kind=0),
           dict(ntotal=2 ** 32), dict(ntotal=2 ** 40), dict(nlist=2 ** 31), dict(nlist=2 ** 40), dict(kind=2), dict(kind=-1), dict(kind=7),
           dict(M=0), dict(M=65, d=65), dict(M=3), dict(M=16, d=24), dict(cb=None), dict(ctx=None, nq=0),
           dict(nq=2 ** 32 - 1, nprobe=1), dict(nq=2 ** 22, nprobe=1024), dict(nq=2 ** 30), dict(nq=2 ** 64 - 1), dict(nq=1431655765, nprobe=3)]
    for kw in bad:
        for radius in (1.5, float("inf"), float("nan")):
            for call in (count, fill):
                assert call(radius=radius, **kw) == VIDC_ERR_INVALID, (call.__name__, kw)
                assert b"range" in L.vidc_last_error(), kw
    total = ctypes.c_uint64(77)
    assert count(off=None, total=ctypes.byref(total)) == VIDC_ERR_INVALID and total.value == 77  # (nothing written)
    for kw in (dict(D=None), dict(lab=None), dict(D=None, lab=None, capacity=2 ** 40)):
        assert fill(**kw) == VIDC_ERR_INVALID and b"range" in L.vidc_last_error(), kw


def test_empty_calls_need_no_device():
    L, count, fill = _calls()
    none = dict(off=None, codes=None, xq=None, probes=None, lims=None)
    # nq == 0: nothing is launched and no array is needed; the total is written when it is given
    total = ctypes.c_uint64(77)
    assert count(nq=0, total=ctypes.byref(total), **none) == 0 and total.value == 0
    assert count(nq=0, **none) == 0 and count(nq=0, kind=0, M=0, cb=None, **none) == 0
    assert fill(nq=0, **none) == 0 and fill(nq=0, capacity=0, D=None, lab=None, **none) == 0
    assert fill(nq=0, D=None, lab=None, **none) == VIDC_ERR_INVALID  # (capacity > 0 wants its arrays, whatever nq is)
    # capacity == 0: nothing is written and no output array is needed
    assert fill(capacity=0, D=None, lab=None) == 0 and fill(capacity=0) == 0
    # the limits still hold
    assert count(nq=0, kind=5, **none) == VIDC_ERR_INVALID and fill(nq=0, nprobe=0, **none) == VIDC_ERR_INVALID
    assert fill(capacity=0, d=0) == VIDC_ERR_INVALID and fill(capacity=0, lims=None) == VIDC_ERR_INVALID


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("ivf_range_plan") / "ivf_range_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "ivf_range_test.cpp")])
    return path


def plan(exe, nq, num_cu, kind, d, M, nprobe):
    out = subprocess.run([exe, "plan", *map(str, (nq, num_cu, kind, d, M, nprobe))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = ("lds", "resident", "S", "items", "nslots", "lo", "hi", "G", "V", "W", "count_bytes")
    return dict(zip(names, map(int, out.stdout.split())))


# nq, num_cu, kind, d, M, nprobe -> lds, resident, S, nslots
PLAN_TABLE = [
    ((10, 256, 1, 128, 16, 16), (16960, 2304, 16, 160)),      # the reference shape, small batch: nine wavefronts per compute unit
    ((10, 256, 1, 128, 16, 4), (16912, 2304, 4, 40)),         # S <= nprobe
    ((10, 256, 1, 128, 16, 1), (16912, 2304, 1, 10)),
    ((1000, 256, 1, 128, 16, 16), (16960, 2304, 4, 2304)),
    ((10000, 256, 1, 128, 16, 16), (16960, 2304, 1, 2304)),
    ((10, 256, 0, 32, 0, 16), (448, 8192, 16, 160)),           # Flat at d = 32
    ((1000, 256, 0, 32, 0, 16), (448, 8192, 16, 8192)),
    ((10000, 256, 0, 32, 0, 16), (448, 8192, 1, 8192)),
    ((1, 256, 1, 2048, 64, 1024), (77824, 512, 16, 16)),       # the limits: two wavefronts per compute unit
    ((5, 256, 0, 2048, 0, 1024), (12544, 3328, 16, 80)),
    ((3, 1, 0, 4, 0, 3), (288, 32, 2, 6)),
]


@pytest.mark.parametrize("args,want", PLAN_TABLE)
def test_the_plan_against_written_out_tables(exe, args, want):
    p = plan(exe, *args)
    assert (p["lds"], p["resident"], p["S"], p["nslots"]) == want, p
    nq, num_cu, kind, d, M, nprobe = args
    assert p["lds"] == rr.plan_lds(kind, nprobe, d, M) and p["lds"] % 16 == 0 and p["resident"] == ir.plan_resident(num_cu, p["lds"])
    assert p["S"] == ir.plan_pieces(nq, nprobe, p["resident"]) and p["items"] == nq * p["S"]
    assert p["lds"] * (p["resident"] // num_cu) <= 160 * 1024
    assert p["count_bytes"] == nq * nprobe * 4  # the scratch does not grow with the results
    assert p["W"] == (0 if kind == 0 else max(w for w in (1, 2, 4, 8, 16) if M % w == 0))
    if kind == 0:
        assert (p["G"], p["V"]) == {32: (8, 4), 2048: (16, 4), 4: (1, 4)}[d]


@pytest.mark.parametrize("kind", sorted(rr.ONE_CU))
def test_the_one_cu_batches_go_round_the_grid_stride_loop(exe, kind):
    b = rr.ONE_CU[kind]
    args = (1, 1 if b["M"] else 0, b["d"], b["M"], b["nprobe"])
    whole, cut = plan(exe, b["nq_whole"], *args), plan(exe, b["nq_cut"], *args)
    assert whole["resident"] == cut["resident"] == (9 if b["M"] else 32)
    assert whole["S"] == 1 and whole["nslots"] == whole["resident"]
    assert whole["lo"] >= 3 and whole["hi"] == whole["lo"] + 1  # every wavefront takes three items, some a fourth: a ragged last trip
    assert cut["S"] == 4 and cut["nslots"] == cut["resident"] and (cut["lo"], cut["hi"]) == (1, 2)


def test_ivf_index_keeps_exactly_its_public_methods():
    from vector_db_id_compression_amd import ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    public = {n for n in dir(IVFIndex) if not n.startswith("_")}
    assert public == {"add", "copy_subset_to", "merge_from", "reconstruct_batch", "remove_ids", "replace_invlists", "search",
                      "search_defer_id_decoding", "train", "scan_device", "search_device"}, sorted(public)
    assert callable(ivf_range.range_scan_device) and callable(ivf_range.range_search_device)


def test_module_functions_without_a_gpu_raise():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(4, 2)
    xq = np.zeros((1, 4), np.float32)
    for call in (lambda: ivf_range.range_scan_device(idx, xq, 1.0), lambda: ivf_range.range_search_device(idx, xq, 1.0)):
        with pytest.raises(VidcError, match="no HIP device"):
            call()
