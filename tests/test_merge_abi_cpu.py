"""CPU: the four merge entry points are declared, listed and exported; NULL arguments are refused before any device work, and the
refusals that read the objects (nlist mismatch, another device, 2^32 - 1 ids) together with the ROC list classes and the shift check
are csrc/merge_plan.h, built with g++ into a stand-alone program and held to the numpy model (merge_ref.py), plain and under
-fsanitize=address,undefined; merge.merge is a module function that refuses the containers out of its scope and mixed classes by
name; the four list classes gained no public attribute; the containers have merge_from and the segmented one refuses;
IVFIndex.merge_from on uncompressed lists needs no device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import merge_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE = ["vidc_packed_merge_dev", "vidc_ef_merge_dev", "vidc_wt_merge_dev", "vidc_roc_merge_dev"]
VIDC_ERR_INVALID = -1


def test_merge_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in MERGE:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    for sym in ("vidc_rocseg_merge_dev", "vidc_shards_merge_dev", "vidc_compact_merge_dev"):  # out of scope
        assert sym not in declared and sym not in _lib.EXPORTED_SYMBOLS and not hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays


def _call(fn, sym, ctx, a, b, out):
    extra = {"vidc_packed_merge_dev": (0,), "vidc_ef_merge_dev": (0,), "vidc_wt_merge_dev": (), "vidc_roc_merge_dev": (-1, 0)}[sym]
    return fn(ctx, a, b, 0, *extra, out, None)


@pytest.mark.parametrize("sym", MERGE)
def test_null_arguments_are_rejected_before_any_device_work(sym):
    """VIDC_ERR_INVALID for a NULL context / a / b / out needs no device, and *out is NULL afterwards wherever out was given"""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    fn = getattr(L, sym)
    p = 8  # (never dereferenced)
    for ctx, a, b, has_out in ((None, None, None, False), (None, p, p, True), (p, None, p, True), (p, p, None, True), (p, p, p, False)):
        out = ctypes.c_void_p(12345)
        assert _call(fn, sym, ctx, a, b, ctypes.byref(out) if has_out else None) == VIDC_ERR_INVALID, (ctx, a, b, has_out)
        assert b"merge" in L.vidc_last_error()
        assert not has_out or out.value is None


def _plan_cases():
    rng = np.random.default_rng(77)
    cases = []
    for a_n in (0, 1, 5):
        for b_n in (0, 1, 7):
            for add_id in (0, 3):
                off = lambda n: np.array([0, n], np.uint64)
                m = mr.merge(off(a_n), np.zeros(a_n, np.uint64), off(b_n), np.zeros(b_n, np.uint64), add_id)
                cases.append(["CLASS", a_n, b_n, int(add_id != 0), int(mr.roc_classes(m, add_id)[0])])
    big = 2 ** 32 - 1
    for args in ((1, 1, 2, 0, 1, 1, big, big), (0, 1, 2, 0, 1, 1, big, big), (0, 2, 2, 0, 0, 1, big, big), (0, 2, 2, 0, 1, 0, 0, 0),
                 (0, 2, 2, 1, 1, 1, big - 1, 1), (0, 2, 2, 1, 1, 1, big - 2, 1), (0, 2, 2, 1, 1, 1, big, 0), (0, 2, 2, 1, 1, 1, 0, big),
                 (0, 0, 0, 3, 3, 3, 0, 0), (0, 7, 7, 0, 0, 0, 2 ** 31, 2 ** 31), (0, 7, 7, 0, 0, 0, 2 ** 63, 2 ** 63)):
        cases.append(["REFUSE", *args, mr.refusal(bool(args[0]), *args[1:])])
    for max_b, add_id, bits in ((2 ** 64 - 1, 1, 64), (2 ** 64 - 2, 1, 64), (2 ** 31 - 1, 1, 31), (2 ** 31 - 2, 1, 31), (255, 1, 8), (254, 1, 8),
                                (0, 0, 0), (0, 1, 0), (2 ** 63, 2 ** 63, 64), (5, 2 ** 64 - 1, 64), (0, 2 ** 64 - 1, 64), (0, 2 ** 64 - 1, 63)):
        cases.append(["SHIFT", max_b, add_id, bits, int(mr.shift_overflows(max_b, add_id, bits))])
    for _ in range(200):
        max_b, add_id, bits = int(rng.integers(0, 2 ** 63)) >> int(rng.integers(0, 63)), int(rng.integers(0, 2 ** 63)) >> int(rng.integers(0, 63)), int(rng.integers(0, 65))
        cases.append(["SHIFT", max_b, add_id, bits, int(mr.shift_overflows(max_b, add_id, bits))])
    return cases


@pytest.mark.parametrize("sanitize", [False, True])
def test_merge_plan_program(tmp_path, sanitize):
    """the classification rule and the refusals the library runs (csrc/merge_plan.h) are the model's"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    cases = _plan_cases()
    kinds = {(c[0], c[-1]) for c in cases}
    assert {("CLASS", 0), ("CLASS", 1), ("CLASS", 2), ("SHIFT", 0), ("SHIFT", 1)} <= kinds
    assert {("REFUSE", r) for r in (mr.OK, mr.ERR_NULL, mr.ERR_NLIST, mr.ERR_DEVICE, mr.ERR_NTOTAL)} <= kinds
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(v) for v in c) for c in cases) + "\n")
    exe = str(tmp_path / "merge_plan_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "merge_plan_test.cpp")])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and f"merge plan ok: {len(cases)} cases" in out.stdout, out.stdout + out.stderr


def test_merge_is_a_module_function_and_refuses_by_class():
    import vector_db_id_compression_amd as pkg
    from vector_db_id_compression_amd import VidcError, codecs, merge, sharding

    assert pkg.merge is merge and "merge" in pkg.__all__ and callable(merge.merge)
    off = np.array([0, 2], dtype=np.uint64)
    lists = [cls(None, None, off) for cls in (codecs.PackedLists, codecs.EfLists, codecs.WaveletTreeLists, codecs.RocLists)]
    for cls in (codecs.RocSegLists, codecs.CompactRows, sharding.DeviceShards):
        obj = cls.__new__(cls)  # (refused before the object is looked at)
        for a, b in ((obj, obj), (obj, lists[0]), (lists[3], obj)):
            with pytest.raises(VidcError, match=cls.__name__):
                merge.merge(a, b)
    with pytest.raises(VidcError, match="object"):
        merge.merge(object(), lists[0])
    for a in lists:
        for b in lists:
            if a is not b:
                with pytest.raises(VidcError, match=f"{type(a).__name__} and {type(b).__name__}"):
                    merge.merge(a, b, 5)
    with pytest.raises(TypeError, match="precision_mode"):
        merge.merge(lists[0], lists[0], precision_mode=3)
    with pytest.raises(TypeError, match="bits"):
        merge.merge(lists[3], lists[3], bits=3)


def test_merge_without_a_gpu_raises():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from vector_db_id_compression_amd import VidcError, merge
    from vector_db_id_compression_amd.codecs import EfLists, PackedLists, RocLists, WaveletTreeLists

    off = np.array([0, 2], dtype=np.uint64)
    for cls in (RocLists, PackedLists, EfLists, WaveletTreeLists):
        with pytest.raises(VidcError, match="no HIP device"):
            merge.merge(cls(None, None, off), cls(None, None, off), 2)


def test_the_list_classes_gained_no_public_attribute():
    from test_gpu_call_contract import SURFACE
    from vector_db_id_compression_amd import codecs

    for cname, want in SURFACE.items():
        got = {name for name in dir(getattr(codecs, cname)) if not name.startswith("_")}
        assert got == set(want), (cname, sorted(got ^ set(want)))


def test_containers_have_merge_from_and_the_segmented_one_refuses():
    from vector_db_id_compression_amd import custom_invlists as ci

    for cls in (ci.CompressedIDInvertedListsPackedBits, ci.CompressedIDInvertedListsFenwickTree, ci.CompressedIDInvertedListsEliasFano,
                ci.CompressedIDInvertedListsWaveletTree):
        assert cls.merge_from is ci.InvertedListsArrayCodes.merge_from
    cls = ci.CompressedIDInvertedListsROCSegmented
    with pytest.raises(RuntimeError, match="no merge"):
        cls.__new__(cls).merge_from(cls.__new__(cls))
    a = ci.CompressedIDInvertedListsPackedBits.__new__(ci.CompressedIDInvertedListsPackedBits)
    with pytest.raises(TypeError, match="FenwickTree"):
        a.merge_from(ci.CompressedIDInvertedListsFenwickTree.__new__(ci.CompressedIDInvertedListsFenwickTree))


def test_ivf_merge_from_on_array_inverted_lists_needs_no_device():
    """two halves built on the host become the index that holds all of it: lists, ids shifted by add_id, codes, ntotal, _next_id"""
    from vector_db_id_compression_amd import ivf
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    def index(lists):
        ix = ivf.IVFIndex(1, 3)  # (Flat: code_size 4; never trained: no centroids on either side)
        ix.invlists = ArrayInvertedLists(3, 4)
        n = 0
        for l, ids in lists.items():
            ix.invlists.add_entries(l, np.array(ids, np.int64), np.array(ids, np.float32).view(np.uint8).reshape(-1, 4))
            n += len(ids)
        ix.ntotal = ix._next_id = n
        return ix

    a, b = index({0: [0, 2], 2: [1]}), index({0: [1], 1: [0, 2]})
    a.merge_from(b)  # add_id = 3
    assert a.ntotal == 6 and a._next_id == 6 and b.ntotal == 3
    assert [a.invlists.get_ids(l).tolist() for l in range(3)] == [[0, 2, 4], [3, 5], [1]]
    assert a.invlists.get_codes(1).view(np.float32).reshape(-1).tolist() == [0.0, 2.0]  # (b's codes travel unchanged)
    assert [b.invlists.get_ids(l).tolist() for l in range(3)] == [[1], [0, 2], []]
    a.merge_from(b, add_id=100)
    assert a.ntotal == 9 and a._next_id == 103 and a.invlists.get_ids(1).tolist() == [3, 5, 100, 102]
    a.merge_from(a, add_id=1000)  # other may be the index itself
    assert a.ntotal == 18 and a.invlists.get_ids(2).tolist() == [1, 1001] and a._next_id == 1103
    with pytest.raises(ValueError, match="differ"):
        a.merge_from(ivf.IVFIndex(1, 4))
    with pytest.raises(TypeError):
        a.merge_from(object())
    c = index({})
    c.centroids = np.zeros(1)
    with pytest.raises(ValueError, match="centroids"):
        a.merge_from(c)
