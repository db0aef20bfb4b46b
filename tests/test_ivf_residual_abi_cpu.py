"""CPU: the three residual entry points are declared, listed, exported and loadable and the ABI version stays 100; every refusal is
VIDC_ERR_INVALID before any device work with the outputs untouched; the header section holds its "Not here" words;
IVFIndex(..., by_residual=True) constructs, Flat refuses, the class gained no public method; without a GPU the device paths raise."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDC_ERR_INVALID = -1
SYMBOLS = {"vidc_ivf_scan_residual_dev": 17, "vidc_ivf_range_count_residual_dev": 16, "vidc_ivf_range_fill_residual_dev": 18}


def test_symbols_declared_listed_exported_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym, nargs in SYMBOLS.items():
        assert sym in declared and sym in _lib.EXPORTED_SYMBOLS and hasattr(dll, sym), sym
        fn = getattr(_lib.lib(), sym)
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int, sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    assert len(_lib.lib().vidc_ivf_scan_dev.argtypes) == 17  # (the raw calls keep their signatures)
    sec = hdr[hdr.index("residual PQ in the IVF scan and range search"):hdr.index("int vidc_ivf_scan_residual_dev(")]
    assert hdr.index("range search over IVF lists") < hdr.index("residual PQ in the IVF scan and range search") < hdr.index("update rows (graph objects")
    for word in ("Not here", "Inner product", "precomputed table", "other than 8 bits", "er-query radii", "coarse quantiser", "harded containers",
                 "Faiss adapter", "LDS", "18560", "90880", "Scratch", "vidc_ctx_d2h_bytes", "count with total != NULL", "d_centroids",
                 "xq - centroids[l]", "bit for bit"):
        assert word in sec, word
    for old in ("scan IVF lists", "range search over IVF lists"):  # the raw sections still say that they do not do this
        assert "residual PQ" in hdr[hdr.index(old):hdr.index(old) + 6000]


def test_refusals_before_any_device_work():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    p = 8  # (never dereferenced)
    ok = dict(ctx=p, nlist=16, off=p, ntotal=2000, codes=p, d=128, M=16, cb=p, cent=p, nq=5, xq=p, nprobe=4, probes=p)
    total = ctypes.c_uint64(77)

    def head(a):
        return (a["ctx"], a["nlist"], a["off"], a["ntotal"], a["codes"], a["d"], a["M"], a["cb"], a["cent"], a["nq"], a["xq"], a["nprobe"], a["probes"])

    def scan(k=20, D=p, lab=p, stats=None, **kw):
        return L.vidc_ivf_scan_residual_dev(*head(dict(ok, **kw)), k, D, lab, stats)

    def count(lims=p, **kw):
        return L.vidc_ivf_range_count_residual_dev(*head(dict(ok, **kw)), 1.5, lims, ctypes.byref(total))

    def fill(lims=p, capacity=10, D=p, lab=p, **kw):
        return L.vidc_ivf_range_fill_residual_dev(*head(dict(ok, **kw)), 1.5, lims, capacity, D, lab)

    shared = [dict(ctx=None), dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(cent=None), dict(cb=None),
              dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049), dict(ntotal=2 ** 32), dict(ntotal=2 ** 40), dict(nlist=2 ** 31),
              dict(nlist=2 ** 40), dict(M=0), dict(M=65, d=65), dict(M=3), dict(M=16, d=24), dict(ctx=None, nq=0)]
    for kw in shared:
        for call, word in ((scan, b"residual scan"), (count, b"residual range count"), (fill, b"residual range fill")):
            assert call(**kw) == VIDC_ERR_INVALID, (kw, word)
            assert word in L.vidc_last_error(), (kw, L.vidc_last_error())
    for kw in (dict(k=0), dict(k=257), dict(k=2 ** 32 - 1), dict(D=None), dict(lab=None)):
        for stats in (None, p):
            assert scan(stats=stats, **kw) == VIDC_ERR_INVALID and b"residual scan" in L.vidc_last_error(), kw
    # the range calls: nq * nprobe, the slot limits, the capacity
    for kw in (dict(nq=2 ** 32 - 1, nprobe=1), dict(nq=2 ** 22, nprobe=1024), dict(lims=None)):
        assert count(**kw) == VIDC_ERR_INVALID and b"residual range count" in L.vidc_last_error(), kw
        assert fill(**kw) == VIDC_ERR_INVALID and b"residual range fill" in L.vidc_last_error(), kw
    assert fill(D=None) == VIDC_ERR_INVALID and fill(lab=None) == VIDC_ERR_INVALID
    assert total.value == 77  # (no refusal wrote the total)
    # nq == 0 launches nothing and needs no array (and no device); the limits still hold
    none = dict(nq=0, off=None, codes=None, xq=None, probes=None, cent=None)
    assert scan(D=None, lab=None, **none) == 0 and scan(nq=0) == 0
    assert scan(nq=0, k=0) == VIDC_ERR_INVALID and scan(nq=0, M=0) == VIDC_ERR_INVALID and scan(nq=0, cb=None) == VIDC_ERR_INVALID
    assert fill(lims=None, capacity=0, D=None, lab=None, **none) == 0 and fill(nq=0) == 0 and fill(nq=0, nprobe=0) == VIDC_ERR_INVALID
    assert L.vidc_ivf_range_count_residual_dev(*head(dict(ok, **none)), 1.5, None, ctypes.byref(total)) == 0 and total.value == 0
    assert L.vidc_ivf_range_count_residual_dev(*head(dict(ok, **none)), 1.5, None, None) == 0
    # the raw entry points still refuse a code kind of 2
    assert L.vidc_ivf_scan_dev(p, 16, p, 2000, p, 2, 128, 16, p, 5, p, 4, p, 20, p, p, None) == VIDC_ERR_INVALID


def test_ivf_index_takes_the_flag_and_gains_no_method():
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(8, 4, ("PQ", 2), by_residual=True)
    assert idx.by_residual is True and idx.M == 2 and idx.code_size == 2
    assert IVFIndex(8, 4, ("PQ", 2)).by_residual is False and IVFIndex(8, 4).by_residual is False
    with pytest.raises(ValueError, match="by_residual"):
        IVFIndex(8, 4, "Flat", by_residual=True)
    public = {n for n in dir(IVFIndex) if not n.startswith("_")}
    assert public == {"add", "copy_subset_to", "merge_from", "reconstruct_batch", "remove_ids", "replace_invlists", "search",
                      "search_defer_id_decoding", "train", "scan_device", "search_device"}, sorted(public)
    assert "by_residual" not in dir(IVFIndex)  # an instance attribute


def test_device_paths_without_a_gpu_raise():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, ivf_range
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(4, 2, ("PQ", 2), by_residual=True)
    xq = np.zeros((1, 4), np.float32)
    for call in (lambda: idx.scan_device(xq, 1), lambda: idx.search_device(xq, 1), lambda: ivf_range.range_scan_device(idx, xq, 1.0),
                 lambda: ivf_range.range_search_device(idx, xq, 1.0)):
        with pytest.raises(VidcError, match="no HIP device"):
            call()
