"""CPU: the three remove entry points are declared, listed and exported (and no wavelet-tree one exists); NULL arguments are refused
before any device work; without a GPU a remove fails loudly; the wavelet-tree container refuses, the other mutators still mirror the
reference's read-only virtuals."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REMOVE = ["vidc_packed_remove_dev", "vidc_ef_remove_dev", "vidc_roc_remove_dev"]


def test_remove_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in REMOVE:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    for sym in ("vidc_wt_remove_dev", "vidc_sharded_remove_dev"):
        assert sym not in declared and sym not in _lib.EXPORTED_SYMBOLS and not hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays


def test_null_arguments_are_rejected_before_any_device_work():
    """VIDC_ERR_INVALID for a NULL context / object / out needs no device"""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    calls = (lambda c, o, out: L.vidc_packed_remove_dev(c, o, 0, None, None, out, None, None, None),
             lambda c, o, out: L.vidc_ef_remove_dev(c, o, 0, None, None, 0, out, None, None, None),
             lambda c, o, out: L.vidc_roc_remove_dev(c, o, 0, None, None, -1, 0, out, None, None, None))
    for call in calls:
        for c, o, with_out in ((None, None, True), (None, 8, True), (8, None, True), (8, 8, False)):  # (8: never dereferenced)
            out = ctypes.c_void_p(1)
            assert call(c, o, ctypes.byref(out) if with_out else None) == -1
            assert b"remove" in L.vidc_last_error()
            assert out.value is None or not with_out, "*out must be NULL after an error"


def test_remove_is_a_module_of_the_package():
    import vector_db_id_compression_amd as pkg
    from vector_db_id_compression_amd import removal

    assert pkg.removal is removal and "removal" in pkg.__all__ and callable(removal.remove)


def test_remove_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, removal
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists

    off = np.array([0, 2], dtype=np.uint64)
    for cls in (RocLists, PackedLists, EfLists):
        obj = cls(None, None, off)
        for ln in (np.array([0], np.int64), None):
            with pytest.raises(VidcError):
                removal.remove(obj, ln, np.array([5], np.uint64))


def test_a_wavelet_tree_has_no_remove():
    from vector_db_id_compression_amd import VidcError, custom_invlists as ci, removal
    from vector_db_id_compression_amd.codecs import WaveletTreeLists

    with pytest.raises(VidcError, match="permutation"):
        removal.remove(WaveletTreeLists(None, None, np.array([0, 2], dtype=np.uint64)), None, np.array([1], np.uint64))
    with pytest.raises(VidcError):
        removal.remove(object(), None, np.array([1], np.uint64))
    il = ci.CompressedIDInvertedListsWaveletTree.__new__(ci.CompressedIDInvertedListsWaveletTree)
    with pytest.raises(RuntimeError, match="permutation"):
        il.remove_batch(np.array([0], np.int64), np.array([1], np.int64))


def test_other_mutators_still_raise():
    from vector_db_id_compression_amd import custom_invlists as ci

    for cls in (ci.CompressedIDInvertedListsPackedBits, ci.CompressedIDInvertedListsFenwickTree, ci.CompressedIDInvertedListsEliasFano):
        assert callable(getattr(cls, "remove_batch"))
        il = cls.__new__(cls)  # (the mutators do not look at the object)
        for name in ("add_entries", "update_entries", "resize"):
            with pytest.raises(RuntimeError, match="read-only"):
                getattr(il, name)(0, 1, None, None)


def test_array_inverted_lists_remove_ids_on_the_host():
    """IVFIndex.remove_ids on uncompressed lists is a numpy filter: no device"""
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(2, 3, ("PQ", 2))
    il = ArrayInvertedLists.from_assignment(np.array([0, 1, 1, 2, 0, 1]), 3, codes=np.arange(12, dtype=np.uint8).reshape(6, 2))
    idx.replace_invlists(il)
    idx.ntotal = idx._next_id = 6
    assert idx.remove_ids(np.array([1, 4, 99], np.int64)) == 2
    assert idx.ntotal == 4 and idx._next_id == 6  # ids handed out later continue from the number ever added
    assert [il.get_ids(l).tolist() for l in range(3)] == [[0], [2, 5], [3]]
    assert il.get_codes(1).tolist() == [[4, 5], [10, 11]]
    assert idx.remove_ids(np.zeros(0, np.int64)) == 0 and idx.ntotal == 4
