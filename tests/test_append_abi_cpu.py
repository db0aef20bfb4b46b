"""CPU: the four append entry points are declared, listed and exported; without a GPU an append fails loudly; the containers' other
mutators still mirror the reference's read-only virtuals."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPEND = ["vidc_packed_append_dev", "vidc_ef_append_dev", "vidc_wt_append_dev", "vidc_roc_append_dev"]


def test_append_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in APPEND:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays


def test_null_arguments_are_rejected_before_any_device_work():
    """VIDC_ERR_INVALID for a NULL context / object / out needs no device"""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    out = ctypes.c_void_p(1)
    assert L.vidc_packed_append_dev(None, None, 0, None, None, 0, ctypes.byref(out), None, None) == -1
    assert L.vidc_ef_append_dev(None, None, 0, None, None, 0, ctypes.byref(out), None, None) == -1
    assert L.vidc_wt_append_dev(None, None, 0, None, None, ctypes.byref(out), None, None) == -1
    assert L.vidc_roc_append_dev(None, None, 0, None, None, -1, 0, ctypes.byref(out), None, None) == -1
    assert b"append" in L.vidc_last_error()


def test_append_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists, WaveletTreeLists

    off = np.array([0, 2], dtype=np.uint64)
    for cls in (RocLists, PackedLists, EfLists, WaveletTreeLists):
        obj = cls(None, None, off)
        with pytest.raises(VidcError):
            obj.append(np.array([0], np.int64), np.array([5], np.uint64))


def test_other_mutators_still_raise():
    from vector_db_id_compression_amd import custom_invlists as ci

    for cls in (ci.CompressedIDInvertedListsPackedBits, ci.CompressedIDInvertedListsFenwickTree,
                ci.CompressedIDInvertedListsEliasFano, ci.CompressedIDInvertedListsWaveletTree):
        assert callable(getattr(cls, "add_batch"))
        il = cls.__new__(cls)  # (the mutators do not look at the object)
        for name in ("add_entries", "update_entries", "resize"):
            with pytest.raises(RuntimeError, match="read-only"):
                getattr(il, name)(0, 1, None, None)
