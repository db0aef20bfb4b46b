"""CPU: the three update_rows entry points are declared, listed and exported; NULL arguments and impossible sizes are refused before
any device work; the Python methods exist and fail loudly without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE = ["vidc_compact_update_rows_dev", "vidc_ef_update_rows_dev", "vidc_roc_update_rows_dev"]


def test_update_rows_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in UPDATE:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    # the section sits between the remove and the sharded lists, and says what it leaves out
    sec = hdr[hdr.index("update rows (graph objects"):hdr.index("sharded lists (several contexts")]
    assert hdr.index("remove (batches of pairs") < hdr.index("update rows (graph objects")
    assert "K > 64" in sec and "VIDC_ERR_UNSUPPORTED" in sec and "last mention wins" in sec


def _calls():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    return L, (lambda c, o, m, nd, rw, n, out: L.vidc_compact_update_rows_dev(c, o, m, nd, rw, n, out, None),
               lambda c, o, m, nd, rw, n, out: L.vidc_ef_update_rows_dev(c, o, m, nd, rw, n, out, None),
               lambda c, o, m, nd, rw, n, out: L.vidc_roc_update_rows_dev(c, o, m, nd, rw, n, -1, out, None))


def test_null_arguments_are_rejected_before_any_device_work():
    """VIDC_ERR_INVALID for a NULL context / object / out needs no device (8: never dereferenced)"""
    L, calls = _calls()
    for call in calls:
        for c, o, with_out in ((None, None, True), (None, 8, True), (8, None, True), (8, 8, False)):
            out = ctypes.c_void_p(1)
            assert call(c, o, 0, None, None, 0, ctypes.byref(out) if with_out else None) == -1
            assert b"update_rows" in L.vidc_last_error()
            assert out.value is None or not with_out, "*out must be NULL after an error"


def test_python_layer_exists():
    from vector_db_id_compression_amd import altid, codecs

    assert callable(codecs.update_rows)
    for cls in (codecs.CompactRows, altid.CompactBitNSGGraph, altid.EliasFanoNSGGraph, altid.ROCNSGGraph):
        assert callable(getattr(cls, "update_rows")), cls.__name__
    # EfLists / RocLists are served by the function: their pinned method sets stay what they were
    assert not hasattr(codecs.EfLists, "update_rows") and not hasattr(codecs.RocLists, "update_rows")


def test_update_rows_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError
    from vector_db_id_compression_amd.codecs import CompactRows, EfLists, RocLists, update_rows

    nodes, rows = np.array([0], np.int64), np.array([[1, -1]], np.int32)
    for obj in (CompactRows(None, None, 2, 2), EfLists(None, None, None, nlist=2), RocLists(None, None, None)):
        obj.K = 2
        with pytest.raises(VidcError):
            update_rows(obj, nodes, rows)
    with pytest.raises(VidcError):
        update_rows(object(), nodes, rows)
