"""CPU: vidc_ivf_scan_dev is declared, listed, exported and loadable and the ABI version stays 100; every limit is VIDC_ERR_INVALID
before any device work, with "scan" in vidc_last_error; the plan header's S, slots, scratch and LDS against written-out tables; the
one-CU batches of the GPU test run the grid-stride loop past its first trip; IVFIndex gained exactly scan_device and search_device.

Items per slot.  The cut is the smallest S with nq * S >= the resident slots, so a call with S > 1 has nq * S / 2 below them: fewer
than two items per slot, whatever the batch.  Three items per slot with a ragged last trip are therefore asserted at S = 1; at S > 1
the batches are chosen so that some slots take two items and the others one (the loop still goes round, raggedly)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ivf_scan_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDC_ERR_INVALID = -1
# the one-CU batches (test_gpu_ivf_scan.py imports them): (d, M, nprobe, k) -> nq with S == 1, nq with S > 1
ONE_CU = {"flat": dict(d=4, M=0, nprobe=16, k=20, nq_whole=101, nq_cut=13),
          "pq": dict(d=128, M=16, nprobe=16, k=20, nq_whole=31, nq_cut=3)}


def test_symbol_declared_listed_exported_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    assert "vidc_ivf_scan_dev" in declared and "vidc_ivf_scan_dev" in _lib.EXPORTED_SYMBOLS and hasattr(dll, "vidc_ivf_scan_dev")
    fn = _lib.lib().vidc_ivf_scan_dev
    assert len(fn.argtypes) == 17 and fn.restype is ctypes.c_int
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    assert (_lib.VIDC_IVF_FLAT, _lib.VIDC_IVF_PQ8) == (0, 1)
    assert re.search(r"#define VIDC_IVF_FLAT 0\b", hdr) and re.search(r"#define VIDC_IVF_PQ8 1\b", hdr)
    sec = hdr[hdr.index("scan IVF lists"):hdr.index("vidc_ivf_scan_dev(")]
    for word in ("Inner product", "residual PQ", "return_codes", "coarse", "sharded", "segmented", "Faiss adapter", "Scratch", "2^32", "2^31"):
        assert word in sec, word  # the header says what is out of scope, and the limits


def test_limits_are_refused_before_any_device_work():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    p = 8  # (never dereferenced)
    ok = dict(ctx=p, nlist=16, off=p, ntotal=2000, codes=p, kind=1, d=128, M=16, cb=p, nq=5, xq=p, nprobe=4, probes=p, k=20, D=p, lab=p, stats=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vidc_ivf_scan_dev(a["ctx"], a["nlist"], a["off"], a["ntotal"], a["codes"], a["kind"], a["d"], a["M"], a["cb"], a["nq"], a["xq"],
                                   a["nprobe"], a["probes"], a["k"], a["D"], a["lab"], a["stats"])

    bad = [dict(ctx=None), dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(D=None), dict(lab=None),
           dict(k=0), dict(k=257), dict(k=2 ** 32 - 1), dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049), dict(d=2049, kind=0),
           dict(ntotal=2 ** 32), dict(ntotal=2 ** 40), dict(nlist=2 ** 31), dict(nlist=2 ** 40), dict(kind=2), dict(kind=-1), dict(kind=7),
           dict(M=0), dict(M=65, d=65), dict(M=3), dict(M=16, d=24), dict(cb=None), dict(ctx=None, nq=0)]
    for kw in bad:
        for stats in (None, p):
            assert call(stats=stats, **kw) == VIDC_ERR_INVALID, kw
            assert b"scan" in L.vidc_last_error(), kw
    # nq == 0 launches nothing and needs no array (and no device); the limits still hold
    assert call(nq=0, off=None, codes=None, xq=None, probes=None, D=None, lab=None) == 0
    assert call(nq=0) == 0 and call(nq=0, kind=0, M=0, cb=None) == 0
    assert call(nq=0, k=0) == VIDC_ERR_INVALID and call(nq=0, kind=5) == VIDC_ERR_INVALID


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path = str(tmp_path_factory.mktemp("ivf_scan_plan") / "ivf_scan_test")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-o", path, os.path.join(ROOT, "tests", "ivf_scan_test.cpp")])
    return path


def plan(exe, nq, num_cu, kind, d, M, nprobe, k):
    out = subprocess.run([exe, "plan", *map(str, (nq, num_cu, kind, d, M, nprobe, k))], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = ("lds", "resident", "S", "items", "nslots", "scratch", "lo", "hi", "G", "V", "W", "merge_lds")
    return dict(zip(names, map(int, out.stdout.split())))


# nq, num_cu, kind, d, M, nprobe, k -> lds, resident, S, nslots, scratch
PLAN_TABLE = [
    ((10, 256, 1, 128, 16, 16, 20), (17536, 2304, 16, 160, 10 * 16 * 21 * 8)),   # the reference shape, small batch
    ((10, 256, 1, 128, 16, 4, 20), (17488, 2304, 4, 40, 10 * 4 * 21 * 8)),       # S <= nprobe
    ((10, 256, 1, 128, 16, 1, 20), (17488, 2304, 1, 10, 0)),
    ((1000, 256, 1, 128, 16, 16, 20), (17536, 2304, 4, 2304, 1000 * 4 * 21 * 8)),
    ((10000, 256, 1, 128, 16, 16, 20), (17536, 2304, 1, 2304, 0)),
    ((10, 256, 0, 32, 0, 16, 20), (1280, 8192, 16, 160, 10 * 16 * 21 * 8)),       # Flat at d = 32
    ((1000, 256, 0, 32, 0, 16, 20), (1280, 8192, 16, 8192, 1000 * 16 * 21 * 8)),
    ((10000, 256, 0, 32, 0, 16, 20), (1280, 8192, 1, 8192, 0)),
    ((1, 256, 1, 2048, 64, 1024, 256), (77824, 512, 16, 16, 16 * 257 * 8)),      # the limits: two wavefronts per compute unit
    ((5, 256, 0, 2048, 0, 1024, 256), (17152, 2304, 16, 80, 5 * 16 * 257 * 8)),
    ((3, 1, 0, 4, 0, 3, 10), (960, 32, 2, 6, 3 * 2 * 11 * 8)),
]


@pytest.mark.parametrize("args,want", PLAN_TABLE)
def test_the_plan_against_written_out_tables(exe, args, want):
    p = plan(exe, *args)
    assert (p["lds"], p["resident"], p["S"], p["nslots"], p["scratch"]) == want, p
    nq, num_cu, kind, d, M, nprobe, k = args
    assert p["lds"] == ir.plan_lds(kind, k, nprobe, d, M) and p["resident"] == ir.plan_resident(num_cu, p["lds"])
    assert p["S"] == ir.plan_pieces(nq, nprobe, p["resident"]) and p["items"] == nq * p["S"] and p["merge_lds"] == p["S"] * k * 8
    assert p["lds"] * (p["resident"] // num_cu) <= 160 * 1024
    assert p["W"] == (0 if kind == 0 else max(w for w in (1, 2, 4, 8, 16) if M % w == 0))
    if kind == 0:
        assert (p["G"], p["V"]) == {32: (8, 4), 2048: (16, 4), 4: (1, 4)}[d]


@pytest.mark.parametrize("kind", sorted(ONE_CU))
def test_the_one_cu_batches_go_round_the_grid_stride_loop(exe, kind):
    b = ONE_CU[kind]
    args = (1, 1 if b["M"] else 0, b["d"], b["M"], b["nprobe"], b["k"])
    whole, cut = plan(exe, b["nq_whole"], *args), plan(exe, b["nq_cut"], *args)
    assert whole["resident"] == cut["resident"] == (9 if b["M"] else 32)
    assert whole["S"] == 1 and whole["nslots"] == whole["resident"] and whole["scratch"] == 0
    assert whole["lo"] >= 3 and whole["hi"] == whole["lo"] + 1  # every slot takes three items, some a fourth: the last trip is ragged
    assert cut["S"] == 4 and cut["nslots"] == cut["resident"] and cut["scratch"] == b["nq_cut"] * 4 * (b["k"] + 1) * 8
    assert (cut["lo"], cut["hi"]) == (1, 2)  # (see the module docstring) some slots go round, some do not
    assert [ir.plan_slot_items(cut["items"], cut["nslots"], s) for s in (0, cut["items"] - cut["nslots"] - 1, cut["items"] - cut["nslots"])] == [2, 2, 1]


def test_ivf_index_gained_exactly_two_methods():
    from vector_db_id_compression_amd.ivf import IVFIndex

    public = {n for n in dir(IVFIndex) if not n.startswith("_")}
    before = {"add", "copy_subset_to", "merge_from", "reconstruct_batch", "remove_ids", "replace_invlists", "search",
              "search_defer_id_decoding", "train"}
    assert public == before | {"scan_device", "search_device"}, sorted(public ^ before)


def test_scan_device_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(4, 2)
    for call in (lambda: idx.scan_device(np.zeros((1, 4), np.float32), 1), lambda: idx.search_device(np.zeros((1, 4), np.float32), 1)):
        with pytest.raises(VidcError, match="no HIP device"):
            call()
