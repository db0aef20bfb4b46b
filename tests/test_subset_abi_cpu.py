"""CPU: the three subset entry points are declared, listed and exported, and the forms that are out of scope are absent; NULL arguments
and every violated argument condition are refused before any device work with *out == NULL; subset.subset is a module function that
needs a device and refuses the containers out of its scope by name; the four list classes gained no public attribute; the containers
have copy_subset_to and the wavelet-tree and segmented ones refuse; IVFIndex.copy_subset_to on uncompressed lists needs no device and
is the inverse of merge_from."""
import ctypes
import os
import re

import numpy as np
import pytest

import subset_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSET = ["vidc_packed_subset_dev", "vidc_ef_subset_dev", "vidc_roc_subset_dev"]
VIDC_ERR_INVALID = -1
BIG = 2 ** 64 - 1


def test_subset_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in SUBSET:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    for sym in ("vidc_wt_subset_dev", "vidc_rocseg_subset_dev", "vidc_shards_subset_dev"):  # out of scope
        assert sym not in declared and sym not in _lib.EXPORTED_SYMBOLS and not hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    merge_doc = hdr[hdr.index("merge (two objects over the same lists"):hdr.index("int vidc_packed_merge_dev")]
    assert "Out of scope" in merge_doc and "copy_subset_to." not in merge_doc.split("Out of scope")[1].split(".")[0]


def _call(fn, sym, ctx, obj, subset_type, a1, a2, out, prec=-1):
    extra = {"vidc_packed_subset_dev": (), "vidc_ef_subset_dev": (0,), "vidc_roc_subset_dev": (prec, 0)}[sym]
    return fn(ctx, obj, subset_type, a1, a2, *extra, out, None, None)


@pytest.mark.parametrize("sym", SUBSET)
def test_null_arguments_are_rejected_before_any_device_work(sym):
    """VIDC_ERR_INVALID for a NULL context / object / out needs no device, and *out is NULL afterwards wherever out was given"""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    fn = getattr(L, sym)
    p = 8  # (never dereferenced)
    for ctx, obj, has_out in ((None, None, False), (None, p, True), (p, None, True), (None, None, True)):
        out = ctypes.c_void_p(12345)
        assert _call(fn, sym, ctx, obj, 0, 0, 5, ctypes.byref(out) if has_out else None) == VIDC_ERR_INVALID, (ctx, obj, has_out)
        assert b"subset" in L.vidc_last_error()
        assert not has_out or out.value is None


@pytest.mark.parametrize("sym", SUBSET)
def test_violated_argument_conditions_are_rejected_before_any_device_work(sym):
    """a subset_type outside 0 .. 4 and every argument condition of the table: VIDC_ERR_INVALID and *out == NULL without a device.
    The checks run on the numbers and the object's ntotal alone, in front of everything else: the object here is a block of zeros
    (ntotal reads 0), the context a pointer that is never followed."""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    fn = getattr(L, sym)
    zeros = (ctypes.c_uint64 * 8192)()
    obj, ctx = ctypes.cast(zeros, ctypes.c_void_p), 8
    bad = [(-1, 1, 0), (5, 1, 0), (1 << 20, 1, 0),                    # the type
           (1, 0, 0), (1, 3, 3), (1, 3, 4), (1, BIG, BIG),              # ID_MOD: a1 >= 1, a2 < a1
           (2, 5, 4), (2, 0, 1), (2, 1, 1), (2, BIG, BIG),              # ELEMENT_RANGE: a1 <= a2 <= T (T = 0 here)
           (3, 0, 0), (3, 2 ** 32, 1), (3, 4, 4), (3, 4, BIG)]          # INVLIST_FRACTION: 1 <= a1 < 2^32, a2 < a1
    for t, a1, a2 in bad:
        assert sr.refusal(False, t, a1, a2, 0) in (sr.ERR_TYPE, sr.ERR_ARGS)
        out = ctypes.c_void_p(12345)
        assert _call(fn, sym, ctx, obj, t, a1, a2, ctypes.byref(out)) == VIDC_ERR_INVALID, (t, a1, a2)
        assert out.value is None and b"subset" in L.vidc_last_error()
    assert not any(zeros)


def test_every_violated_argument_condition_is_a_refusal_of_the_model():
    """the table of include/vidc.h, condition by condition"""
    T = 100
    bad = [(1, 0, 0), (1, 3, 3), (1, 3, 4), (2, 5, 4), (2, 0, T + 1), (2, T + 1, T + 1), (3, 0, 0), (3, 2 ** 32, 1), (3, 4, 4), (3, 4, BIG),
           (5, 0, 0), (-1, 0, 0)]
    for t, a1, a2 in bad:
        assert sr.refusal(False, t, a1, a2, T) in (sr.ERR_ARGS, sr.ERR_TYPE), (t, a1, a2)
    good = [(0, 0, 0), (0, BIG, 0), (1, 1, 0), (1, BIG, BIG - 1), (2, 0, 0), (2, 0, T), (2, T, T), (3, 1, 0), (3, 2 ** 32 - 1, 0), (4, 0, 0),
            (4, BIG, BIG), (4, 9, 2)]
    for t, a1, a2 in good:
        assert sr.refusal(False, t, a1, a2, T) == sr.OK, (t, a1, a2)


def test_subset_is_a_module_function_and_refuses_by_class():
    import vector_db_id_compression_amd as pkg
    from vector_db_id_compression_amd import VidcError, codecs, sharding, subset

    assert pkg.subset is subset and "subset" in pkg.__all__ and callable(subset.subset)
    assert (subset.ID_RANGE, subset.ID_MOD, subset.ELEMENT_RANGE, subset.INVLIST_FRACTION, subset.INVLIST) == (0, 1, 2, 3, 4)
    for cls in (codecs.WaveletTreeLists, codecs.RocSegLists, codecs.CompactRows, sharding.DeviceShards):
        obj = cls.__new__(cls)  # (refused before the object is looked at)
        with pytest.raises(VidcError, match=cls.__name__):
            subset.subset(obj, subset.ID_MOD, 2, 0)
    graph = codecs.RocLists(None, None, None)
    graph.K = 8
    with pytest.raises(VidcError, match="graph-row"):
        subset.subset(graph, subset.INVLIST, 0, 1)
    with pytest.raises(VidcError, match="object"):
        subset.subset(object(), 0, 0, 1)
    off = np.array([0, 2], dtype=np.uint64)
    for a1, a2 in ((-1, 0), (0, 2 ** 64)):
        with pytest.raises(ValueError, match="2\\^64"):
            subset.subset(codecs.PackedLists(None, None, off), 0, a1, a2)


def test_subset_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, subset
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists

    off = np.array([0, 2], dtype=np.uint64)
    for cls in (RocLists, PackedLists, EfLists):
        with pytest.raises(VidcError, match="no HIP device"):
            subset.subset(cls(None, None, off), subset.ID_MOD, 2, 1)


def test_the_list_classes_gained_no_public_attribute():
    from test_gpu_call_contract import SURFACE
    from vector_db_id_compression_amd import codecs

    for cname, want in SURFACE.items():
        got = {name for name in dir(getattr(codecs, cname)) if not name.startswith("_")}
        assert got == set(want), (cname, sorted(got ^ set(want)))


def test_containers_have_copy_subset_to_and_two_of_them_refuse():
    from vector_db_id_compression_amd import custom_invlists as ci

    for cls in (ci.CompressedIDInvertedListsPackedBits, ci.CompressedIDInvertedListsFenwickTree, ci.CompressedIDInvertedListsEliasFano):
        assert cls.copy_subset_to is ci.InvertedListsArrayCodes.copy_subset_to
    for cls in (ci.CompressedIDInvertedListsWaveletTree, ci.CompressedIDInvertedListsROCSegmented):
        with pytest.raises(RuntimeError, match="no copy_subset_to"):
            cls.__new__(cls).copy_subset_to(cls.__new__(cls), 1, 2, 0)
    a = ci.CompressedIDInvertedListsPackedBits.__new__(ci.CompressedIDInvertedListsPackedBits)
    with pytest.raises(TypeError, match="FenwickTree"):
        a.copy_subset_to(ci.CompressedIDInvertedListsFenwickTree.__new__(ci.CompressedIDInvertedListsFenwickTree), 1, 2, 0)
    a.nlist, a.code_size = 4, 8
    for nlist, cs in ((5, 8), (4, 4)):
        b = ci.CompressedIDInvertedListsPackedBits.__new__(ci.CompressedIDInvertedListsPackedBits)
        b.nlist, b.code_size = nlist, cs
        with pytest.raises(ValueError, match="differ"):
            a.copy_subset_to(b, 1, 2, 0)


def _index(lists, nlist=5):
    from vector_db_id_compression_amd import ivf
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    ix = ivf.IVFIndex(1, nlist)  # (Flat: code_size 4; never trained: no centroids on either side)
    ix.invlists = ArrayInvertedLists(nlist, 4)
    n = 0
    for l, ids in lists.items():
        ids = np.array(ids, np.uint64).view(np.int64)
        ix.invlists.add_entries(l, ids, (ids % 1000).astype(np.float32).view(np.uint8).reshape(-1, 4))  # a payload computed from the id
        n += len(ids)
    ix.ntotal = ix._next_id = n
    return ix


def _lists(ix):
    return [sorted(zip(ix.invlists.get_ids(l).view(np.uint64).tolist(), ix.invlists.get_codes(l).view(np.float32).reshape(-1).tolist()))
            for l in range(ix.nlist)]


SPLITS = {  # subset type -> the (a1, a2) of parts that together take every entry once
    0: [(0, 7), (7, 7), (7, 2 ** 33), (2 ** 33, BIG)],
    1: [(3, 0), (3, 1), (3, 2)],
    2: [(0, 4), (4, 4), (4, 9), (9, 16)],
    3: [(3, 0), (3, 1), (3, 2)],
    4: [(0, 2), (2, 2), (2, 900)],
}


@pytest.mark.parametrize("subset_type", sorted(SPLITS))
def test_ivf_copy_subset_to_on_array_inverted_lists_needs_no_device(subset_type):
    """an index split into parts by each of the five rules and merged back holds every list again as a multiset, codes attached; the
    parts are the model's"""
    src = _index({0: [0, 9, 2 ** 33 + 1, 4], 1: [], 2: [5], 3: [7, 6, 2 ** 63 + 2, 1, 12, 13, 14, 15], 4: [8, 3, 10]})
    assert src.ntotal == 16
    off, ids, _ = src.invlists.to_csr()
    want = _lists(src)
    whole = _index({})
    for a1, a2 in SPLITS[subset_type]:
        part = _index({})
        n = src.copy_subset_to(part, subset_type, a1, a2)
        m = sr.subset(subset_type, a1, a2, off, ids)
        assert n == m.n_taken == part.ntotal and part._next_id == src._next_id
        assert np.array_equal(part.invlists.to_csr()[0], m.offsets) and np.array_equal(part.invlists.to_csr()[1], m.ids)
        whole.merge_from(part, add_id=0)
    assert _lists(whole) == want and whole.ntotal == 16
    assert _lists(src) == want and src.ntotal == 16  # the source is unchanged


def test_ivf_copy_subset_to_refuses_what_merge_from_refuses():
    from vector_db_id_compression_amd import ivf

    a = _index({0: [1, 2]})
    with pytest.raises(ValueError, match="differ"):
        a.copy_subset_to(ivf.IVFIndex(1, 4), 1, 2, 0)
    with pytest.raises(TypeError):
        a.copy_subset_to(object(), 1, 2, 0)
    c = _index({})
    c.centroids = np.zeros(1)
    with pytest.raises(ValueError, match="centroids"):
        a.copy_subset_to(c, 1, 2, 0)
    for t, a1, a2 in ((1, 0, 0), (1, 3, 3), (2, 2, 1), (2, 0, 3), (3, 0, 0), (3, 2 ** 32, 0), (5, 0, 0), (-1, 0, 0), (0, -1, 0)):
        with pytest.raises(ValueError, match="copy_subset_to"):
            a.copy_subset_to(_index({}), t, a1, a2)
