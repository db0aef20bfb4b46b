"""CPU: the three vidc_*_search_dev symbols are declared, listed, exported and loadable, there is no ROC form and the ABI version stays
100; every limit is VIDC_ERR_INVALID before any device work, with "search" in vidc_last_error; graph_search.search_device is a module
function that refuses ROCNSGGraph and everything else it cannot walk by class name, and says so when there is no GPU; the list classes
gained no public attribute."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDC_ERR_INVALID = -1
SYMS = ("vidc_rows_search_dev", "vidc_compact_search_dev", "vidc_ef_search_dev")


def test_symbols_declared_listed_exported_and_loadable():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTED_SYMBOLS and hasattr(dll, sym), sym
    for sym in ("vidc_roc_search_dev", "vidc_rocseg_search_dev", "vidc_shards_search_dev"):  # out of scope
        assert sym not in declared and sym not in _lib.EXPORTED_SYMBOLS and not hasattr(dll, sym) and sym not in hdr, sym
    L = _lib.lib()
    assert len(L.vidc_rows_search_dev.argtypes) == 15 and len(L.vidc_compact_search_dev.argtypes) == 13 == len(L.vidc_ef_search_dev.argtypes)
    assert all(getattr(L, s).restype is ctypes.c_int for s in SYMS)
    assert L.vidc_version() == 100  # the ABI grows, its version stays
    assert "search_batched" in hdr and "ROC" in hdr[hdr.index("search graph rows"):hdr.index("vidc_rows_search_dev(")]  # the header says where ROC goes


def test_limits_are_refused_before_any_device_work():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    p = 8  # (never dereferenced)
    ok = dict(ctx=p, N=100, K=8, rows=p, x=p, d=16, nq=5, xq=p, k=10, L=64, entry=0, rounds=0, D=p, I=p, stats=None)

    def rows_call(**kw):
        a = dict(ok, **kw)
        return L.vidc_rows_search_dev(a["ctx"], a["N"], a["K"], a["rows"], a["x"], a["d"], a["nq"], a["xq"], a["k"], a["L"], a["entry"],
                                      a["rounds"], a["D"], a["I"], a["stats"])

    bad = [dict(ctx=None), dict(rows=None), dict(x=None), dict(xq=None), dict(D=None), dict(I=None), dict(k=0), dict(k=65), dict(L=257, k=257),
           dict(L=257), dict(L=0, k=0), dict(d=0), dict(d=2049), dict(entry=100), dict(entry=2 ** 32 - 1), dict(N=2 ** 31), dict(N=2 ** 40),
           dict(N=0), dict(nq=2 ** 32 - 1), dict(nq=2 ** 40), dict(K=0)]
    for kw in bad:
        for stats in (None, p):
            assert rows_call(stats=stats, **kw) == VIDC_ERR_INVALID, kw
            assert b"search" in L.vidc_last_error(), kw
    # nq == 0 launches nothing and needs no array (and no device)
    assert rows_call(nq=0, rows=None, x=None, xq=None, D=None, I=None) == 0
    assert rows_call(nq=0) == 0
    # the object forms: a NULL context or object (the limits that need the object's N are checked on a live context, on the GPU)
    tail = (p, 16, 5, p, 10, 64, 0, 0, p, p, None)
    for fn in (L.vidc_compact_search_dev, L.vidc_ef_search_dev):
        for ctx, obj in ((None, None), (p, None)):
            assert fn(ctx, obj, *tail) == VIDC_ERR_INVALID
            assert b"search" in L.vidc_last_error()


def test_search_device_is_a_module_function_that_refuses_by_class():
    from vector_db_id_compression_amd import VidcError, altid, codecs, graph_search, sharding

    assert callable(graph_search.search_device)
    x, xq = np.zeros((4, 2), np.float32), np.zeros((1, 2), np.float32)
    for cls in (altid.ROCNSGGraph, codecs.RocLists, codecs.RocSegLists, codecs.PackedLists, codecs.WaveletTreeLists, sharding.DeviceShards):
        obj = cls.__new__(cls)  # (refused before the object is looked at)
        with pytest.raises(VidcError, match=rf"{cls.__name__}.*search_batched"):
            graph_search.search_device(obj, x, xq, 1)
    with pytest.raises(VidcError, match="object.*search_batched"):
        graph_search.search_device(object(), x, xq, 1)
    for cls in (altid.CompactBitNSGGraph, altid.EliasFanoNSGGraph, altid.ROCNSGGraph, altid._GraphBase, codecs.CompactRows, codecs.EfLists):
        assert not hasattr(cls, "search_device") and not hasattr(cls, "search"), cls.__name__


def test_search_device_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, altid, codecs, graph_search

    x, xq = np.zeros((4, 2), np.float32), np.zeros((1, 2), np.float32)
    raw = graph_search.RawGraph(np.full((4, 2), -1, np.int32))
    ef = object.__new__(altid.EliasFanoNSGGraph)
    ef._c = codecs.EfLists.__new__(codecs.EfLists)
    for g in (raw, codecs.CompactRows.__new__(codecs.CompactRows), ef):
        with pytest.raises(VidcError, match="no HIP device"):
            graph_search.search_device(g, x, xq, 1)


def test_the_list_classes_gained_no_public_attribute():
    from test_gpu_call_contract import SURFACE
    from vector_db_id_compression_amd import codecs

    for cname, want in SURFACE.items():
        got = {name for name in dir(getattr(codecs, cname)) if not name.startswith("_")}
        assert got == set(want), (cname, sorted(got ^ set(want)))
