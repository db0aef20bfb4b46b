"""Subsets of compressed lists on the device (vidc_*_subset_dev, Faiss's copy_subset_to): the new object is the one the ordinary encoder
builds from the taken entries, word for word; the mask names the taken positions and nothing around it is written; the source is
untouched; ROC copies the streams of the lists that keep everything, empties the ones that keep nothing and re-encodes only the rest;
nothing moves id payload over PCIe.  copy_subset_to of the containers and of IVFIndex is the inverse of merge_from.

The subset S comes from tests/subset_ref.py and the source's own decode_all.  ROC inputs are lists the reference codec round-trips
(distinct ids, no power-of-two maximum, at most 65 536 ids; include/vidc.h says why): ids here are 6 * k + 3, so no list and no part
of a list has a power-of-two maximum."""
import ctypes as C

import numpy as np
import pytest

import churn_ref as ch
import subset_ref as sr
from test_gpu_append import dev_i64, encode
from test_gpu_dev_offsets import dev, same, sorted_lists, zipf
from test_gpu_remove import check_roundtrips, img, spread

pytestmark = pytest.mark.gpu

KINDS = ["packed", "ef", "roc"]
BITS = 24  # packed width of the ordinary cases: ids below 2^24
SG_BITS = 28  # ... and of the shapes of test_gpu_small_grid.py
BIG = 2 ** 64 - 1
GUARD = 64


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _subset():
    from vector_db_id_compression_amd import subset

    return subset


def check_subset(kind, old, t, a1, a2, want_perm=True, ctx=None):
    """take the subset of `old`; compare with the from-scratch encode of S, the mask between its guard bands, the size, the d2h
    counter and the source's image -> (new, model)"""
    torch = _torch()
    ctx = _lib().default_context() if ctx is None else ctx
    dec = old.decode_all().cpu().numpy().view(np.uint64)
    m = sr.subset(t, a1, a2, old.offsets, dec)
    before = img(kind, old, want_perm)
    T = old.ntotal
    buf = torch.full((T + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    d2h = ctx.d2h_bytes()
    new, mask = _subset().subset(old, t, a1, a2, want_perm=want_perm, taken=buf[GUARD:GUARD + T])
    what = f"{kind} subset type {t} ({a1}, {a2})"
    assert ctx.d2h_bytes() == d2h, f"{what}: id payload moved to the host"
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0xAB).all() and (got[GUARD + T:] == 0xAB).all(), f"{what}: a byte outside the mask was written"
    assert np.array_equal(got[GUARD:GUARD + T], m.mask), f"{what}: the taken mask differs from the model"
    assert np.array_equal(mask.cpu().numpy(), m.mask)
    scratch = encode(kind, m.offsets, m.ids, want_perm, old.bits if kind == "packed" else None)
    same(img(kind, new, want_perm), img(kind, scratch, want_perm), what)
    assert new.ntotal == m.n_taken, what
    same(img(kind, old, want_perm), before, f"{what}: the source changed")
    return new, m


# ------------------------------------------------------------------------------------------------------------- list sizes on the seams
SEAM_SIZES = np.array([0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097, 4100, 70, 1, 0, 300], np.int64)
TOP = 6 * (1 << 19)  # every non-empty list's largest id is above it, every other id below


@pytest.fixture(scope="module")
def seams():
    """the sizes around the wavefront, the 1024-id chunk and the ROC classes (64 / 1024 / 2048 / 4096); ids ascending in every list,
    the largest of list l = 6 (2^19 + l) + 3: ID_RANGE [0, TOP) takes all but the last entry, so 65 -> 64, 1025 -> 1024, 2049 -> 2048,
    4097 -> 4096 and 1 -> 0"""
    rng = np.random.default_rng(33)
    off = np.concatenate([[0], np.cumsum(SEAM_SIZES)]).astype(np.uint64)
    ids = spread(rng.choice(1 << 18, int(off[-1]), replace=False))
    for l in range(SEAM_SIZES.size):
        a, b = int(off[l]), int(off[l + 1])
        ids[a:b].sort()
        if b > a:
            ids[b - 1] = 6 * ((1 << 19) + l) + 3
    return off, ids


def seam_cases(family, off, dec):
    o = off.astype(np.int64)
    T, nlist = int(o[-1]), o.size - 1
    big = np.sort(dec[o[8]:o[9]])  # the list of 2049 ids
    if family == "id_range":
        return [(0, 0, TOP), (0, TOP, BIG), (0, 0, BIG), (0, 5, 5), (0, BIG, 0), (0, int(big[7]), int(big[1500]))] + \
               [(0, 0, int(big[k])) for k in (1023, 1024, 1025)]  # (ascending lists: the range ends before, on and behind a chunk end)
    if family == "id_mod":
        x = int(dec[o[9] + 100])
        return [(1, 1, 0), (1, 2, 1), (1, 2, 0), (1, 3, 0), (1, 3, 1), (1, 4, 1), (1, 4, 3), (1, 8, 5), (1, 5, 2), (1, 7, 0), (1, 1 << 20, x % (1 << 20)),
                (1, 2 ** 32 - 1, x), (1, 2 ** 32 + 5, x), (1, 2 ** 40, x), (1, 2 ** 63 + 1, x), (1, BIG, 5)]
    if family == "element_range":
        return [(2, 0, T), (2, 0, 0), (2, T, T), (2, 777, 777), (2, 0, T // 2), (2, T // 3, 2 * T // 3), (2, 1, T - 1), (2, T - 300, T),
                (2, 4100, 4100 + 2049), (2, 0, 1024), (2, 1023, T - 1025)]
    if family == "fraction":
        return [(3, 1, 0), (3, 2, 0), (3, 2, 1), (3, 3, 1), (3, 4, 3), (3, 2049, 1023), (3, 2049, 1024), (3, 2049, 1025), (3, 4100, 4099),
                (3, 2 ** 32 - 1, 0), (3, 2 ** 32 - 1, 2 ** 32 - 2)]
    assert family == "invlist"
    return [(4, 0, nlist), (4, 0, BIG), (4, 3, 3), (4, 9, 2), (4, 0, 7), (4, 7, 900), (4, nlist, nlist + 5), (4, 8, 9), (4, BIG, BIG)]


FAMILIES = ["id_range", "id_mod", "element_range", "fraction", "invlist"]


def run_seams(kind, family, seams, oracle):
    off, ids = seams
    if kind == "roc":
        check_roundtrips(oracle, off, ids)
    old = encode(kind, off, ids, True, BITS)
    dec = old.decode_all().cpu().numpy().view(np.uint64)
    taken = []
    for t, a1, a2 in seam_cases(family, off, dec):
        new, m = check_subset(kind, old, t, a1, a2)
        taken.append(m.n_taken)
        if m.n_taken == old.ntotal:  # (ROC's permutation is over the input of the last call: the source's own order)
            same(img(kind, new, kind != "roc"), img(kind, old, kind != "roc"), f"{kind}: everything taken must give the source")
        if m.n_taken == 0:
            assert not new.offsets.any() and new.compressed_bytes == 0
    assert old.ntotal in taken and 0 in taken and any(0 < n < old.ntotal for n in taken)
    return old


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_list_sizes_on_the_chunk_and_class_seams(kind, family, seams, oracle):
    old = run_seams(kind, family, seams, oracle)
    if family == "id_range":  # the class seams crossed downward by one entry
        _, m = check_subset(kind, old, 0, 0, TOP)
        assert np.diff(m.offsets.astype(np.int64)).tolist() == [max(0, n - 1) for n in SEAM_SIZES]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("hook", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
def test_roc_on_the_other_kernel_families(hook, family, seams, oracle, monkeypatch):
    monkeypatch.setenv(hook, "1")
    run_seams("roc", family, seams, oracle)


def test_element_range_bounds_that_cross(oracle):
    """offsets 0, 3, 4, 10 with a1 = 3, a2 = 4: list 1 gets i1 = 1 > i2 = 0 and gives nothing"""
    off = np.array([0, 3, 4, 10], np.uint64)
    ids = spread(np.array([5, 9, 11, 2, 1, 3, 4, 6, 7, 8]))
    for kind in KINDS:
        old = encode(kind, off, ids, True, BITS)
        _, m = check_subset(kind, old, sr.ELEMENT_RANGE, 3, 4)
        assert np.diff(m.offsets.astype(np.int64)).tolist() == [1, 0, 1]
        for a1 in (0, 3, 7, 10):
            for a2 in range(a1, 11, 3):
                check_subset(kind, old, sr.ELEMENT_RANGE, a1, a2)


# ------------------------------------------------------------------------------------------------------------- ROC: what is re-encoded
def test_roc_invlist_copies_streams_and_encodes_nothing(seams, oracle):
    off, ids = seams
    ctx = _lib().default_context()
    old = encode("roc", off, ids, True, BITS)
    info = old.info()
    for a1, a2 in ((0, 7), (7, 900), (3, 3), (9, 2), (0, BIG)):
        _subset().subset(old, sr.INVLIST, a1, a2, want_perm=True)
        for which in (0, 1):  # (read before anything else encodes or decodes)
            assert ctx.chain_info(which)["longest"] == 0, f"INVLIST ({a1}, {a2}): a list went through an ANS chain"
        new, m = check_subset("roc", old, sr.INVLIST, a1, a2)
        assert not (m.classes == sr.PARTIAL).any()
        ninfo = new.info()
        for l in range(off.size - 1):
            if a1 <= l < a2:
                nw = int(info["nwords"][l])
                assert int(ninfo["nwords"][l]) == nw and int(ninfo["heads"][l]) == int(info["heads"][l])
                assert np.array_equal(new.words(l, nw), old.words(l, nw)), f"list {l}: the kept stream is not the source's"
            else:
                assert int(ninfo["nwords"][l]) == 0 and int(ninfo["sizes"][l]) == 0


def test_roc_positional_types_decode_only_the_partial_lists(oracle):
    """ELEMENT_RANGE hands every list its share of the range: a short range leaves most lists empty and a part of a few; nothing
    longer than the longest of those goes through a chain, and a range that takes nothing decodes nothing"""
    from vector_db_id_compression_amd.codecs import RocLists

    ctx = _lib().default_context()
    off, ids = zipf(200_000, 300, seed=61)
    ids = spread(ids)
    sizes = np.diff(off.astype(np.int64))
    old = RocLists.encode(off, dev(ids))
    dec = old.decode_all().cpu().numpy().view(np.uint64)
    for a1, a2 in ((0, 20), (777, 777), (100_000, 100_007)):
        m = sr.subset(sr.ELEMENT_RANGE, a1, a2, off, dec)
        partial = np.flatnonzero(m.classes == sr.PARTIAL)
        longest = int(sizes[partial].max()) if partial.size else 0
        # (the shares are differences of running totals: more lists than a2 - a1 may get one, see the crossing bounds)
        assert (m.classes == sr.EMPTY).sum() >= 200 and (partial.size > 0) == (a2 > a1)
        _subset().subset(old, sr.ELEMENT_RANGE, a1, a2, taken=False)
        for which in (0, 1):  # (read before anything else encodes or decodes)
            info = ctx.chain_info(which)
            assert info["longest"] <= longest, (which, info, longest)
        check_subset("roc", old, sr.ELEMENT_RANGE, a1, a2, want_perm=False)


def test_roc_twenty_bit_list_cut_in_half(oracle):
    """the sparse scheme of churn_ref.py: L_WIDE holds 4090 ids of 19 - 20 bits, L_PREC 499 ids below 2^15 and one of 20 bits"""
    init, _ = ch.schedule("sparse")
    m0 = ch.Model(init)
    off, ids = m0.offsets(), m0.ids()
    check_roundtrips(oracle, off, ids)
    old = encode("roc", off, ids, True, BITS)
    prec = old.info()["precision"]
    assert int(prec[ch.L_WIDE]) >= 20 and int(prec[ch.L_PREC]) >= 20
    for t, a1, a2 in ((3, 2, 0), (3, 2, 1), (0, 0, int(np.median(init[ch.L_WIDE]))), (0, int(np.median(init[ch.L_WIDE])), BIG), (1, 4, 1),
                      (0, 0, int(init[ch.L_PREC].max()))):  # (the last one drops L_PREC's 20-bit id: its precision falls)
        new, m = check_subset("roc", old, t, a1, a2)
    assert int(new.info()["precision"][ch.L_PREC]) < int(prec[ch.L_PREC])


# ------------------------------------------------------------------------------------------------------------- many lists, wide ids
@pytest.fixture(scope="module")
def zipf9000():
    """9000 lists: the scans over the lists pass one tile; most lists hold a handful of ids, many none"""
    off, ids = zipf(60_000, 9000, seed=63)
    return off, spread(ids)


@pytest.mark.parametrize("kind", KINDS)
def test_nine_thousand_lists(kind, zipf9000, oracle):
    off, ids = zipf9000
    if kind == "roc":
        check_roundtrips(oracle, off, ids)
    old = encode(kind, off, ids, True, BITS)
    T = int(off[-1])
    for t, a1, a2 in ((0, 6 * 10_000, 6 * 40_000), (1, 4, 3), (2, T // 5, T // 2), (3, 3, 1), (4, 1000, 5000)):
        _, m = check_subset(kind, old, t, a1, a2)
        assert 0 < m.n_taken < T and (m.classes == sr.PARTIAL).any() == (t != 4)


@pytest.mark.parametrize("kind", ["packed", "ef"])
def test_ids_above_32_bits(kind):
    """packed bits at width 40 and Elias-Fano over a 2^40 universe: the predicates compare and reduce all 64 bits"""
    off, ids = sorted_lists(np.array([700, 0, 1500, 40, 1025], np.uint64), universe=1 << 40, seed=65)
    assert (ids >> 32).max() > 0
    old = encode(kind, off, ids, True, 40)
    x = int(ids[1000])
    cases = [(0, 1 << 32, 1 << 39), (0, x, x + 1), (0, (1 << 39) + 12345, BIG), (0, 0, 1 << 32)]
    cases += [(1, a1, x % a1) for a1 in (1, 2, 3, 7, 1 << 33, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 10 ** 12 + 39, 1 << 40)]
    cases += [(1, 3, (x + 1) % 3), (1, 2 ** 32 - 1, (x + 1) % (2 ** 32 - 1))]
    hit = 0
    for t, a1, a2 in cases:
        _, m = check_subset(kind, old, t, a1, a2)
        hit += m.n_taken > 0
    assert hit >= len(cases) - 2


# ------------------------------------------------------------------------------------------------------------- one compute unit
@pytest.fixture(scope="module")
def one_cu():
    """a context created under VIDC_NUM_CU=1 with pool poison on, running on torch's stream"""
    L, torch = _lib(), _torch()
    torch.cuda.set_device(0)
    mp = pytest.MonkeyPatch()
    mp.setenv("VIDC_NUM_CU", "1")
    ctx = L.Context(0)
    mp.undo()
    assert ctx.num_cu() == 1
    ctx.set_pool_poison(True)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx
    torch.cuda.synchronize()
    ctx.synchronize()
    ctx.close()


def _encode_on(kind, off, ids, ctx):
    from vector_db_id_compression_amd import codecs as cd

    d = dev(ids)
    _torch().cuda.synchronize()
    if kind == "packed":
        return cd.PackedLists.encode(off, d, bits=SG_BITS, ctx=ctx)
    if kind == "ef":
        return cd.EfLists.encode(off, d, want_perm=True, ctx=ctx)
    return cd.RocLists.encode(off, d, want_perm=True, ctx=ctx)


@pytest.mark.parametrize("name", ["chunky", "short"])
@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_loops_on_one_compute_unit(kind, name, one_cu, monkeypatch):
    """one CU: a chunk kernel runs 64 wavefronts a trip, a per-list kernel 8192 threads.  `chunky` (600 lists, about 700 chunks of
    1024 ids) gives the mark, the slice and the compaction more than three trips, `short` (17 001 lists) the bounds and the slots"""
    from test_gpu_small_grid import HOOKS, shape

    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    sh = shape(name)
    off, ids = sh["off"], sh["ids"]
    assert (name == "chunky" and sh["offers"]["chunk1024"] > 3 * 64) or (name == "short" and off.size - 1 > 2 * 8192)
    old = _encode_on(kind, off, ids, one_cu)
    T = int(off[-1])
    for t, a1, a2 in ((0, int(np.median(ids)), BIG), (1, 4, 3), (2, T // 7, T - T // 3), (3, 3, 1), (4, 100, (off.size - 1) - 50)):
        new, m = check_subset(kind, old, t, a1, a2, ctx=one_cu)
        assert 0 < m.n_taken < T
        twin, _ = _subset().subset(encode(kind, off, ids, True, SG_BITS), t, a1, a2, want_perm=True)
        same(img(kind, new), img(kind, twin), f"{kind} {name} type {t}: one CU against the default context")


# ------------------------------------------------------------------------------------------------------------- derived objects
@pytest.mark.parametrize("kind", KINDS)
def test_subsets_of_appended_shrunk_merged_and_loaded_objects(kind, tmp_path, oracle):
    from vector_db_id_compression_amd import merge, persist, removal

    rng = np.random.default_rng(67)
    off, ids = zipf(20_000, 120, seed=68)
    ids = spread(ids)
    base = encode(kind, off, ids, True, BITS)
    ln = rng.integers(0, 120, 3000)
    add = spread(30_000 + np.arange(3000))
    appended, _ = base.append(dev_i64(ln), dev(add), **({} if kind == "packed" else {"want_perm": True}))
    shrunk, _ = removal.remove(appended, None, dev(ids[::3]), want_perm=True)
    off_b, ids_b = zipf(5000, 120, seed=69)
    other = encode(kind, off_b, spread(50_000 + ids_b), True, BITS)
    merged = merge.merge(shrunk, other, 0, **({} if kind == "packed" else {"want_perm": True}))
    loaded = persist.load(persist.save(merged, str(tmp_path / f"{kind}.npz")))
    for name, obj in (("appended", appended), ("shrunk", shrunk), ("merged", merged), ("loaded", loaded)):
        T = obj.ntotal
        for t, a1, a2 in ((1, 4, 1), (3, 3, 2), (2, T // 4, T // 2), (4, 10, 60), (0, 6 * 5000, 6 * 31_000)):
            _, m = check_subset(kind, obj, t, a1, a2, want_perm=name != "loaded")  # (a loaded object carries no permutation)
            assert 0 < m.n_taken < T, name


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "pool_poison"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_same_call_twice_gives_identical_objects(kind, poison, seams):
    L = _lib()
    ctx = L.default_context()
    off, ids = seams
    L.check(L.lib().vidc_ctx_debug_pool_poison(ctx.h, 1 if poison else 0))
    try:
        old = encode(kind, off, ids, True, BITS)
        for t, a1, a2 in ((1, 4, 1), (2, 3000, 9000), (3, 3, 1)):
            first, m = check_subset(kind, old, t, a1, a2)
            want = img(kind, first)
            second, mask = _subset().subset(old, t, a1, a2, want_perm=True)
            same(img(kind, second), want, f"{kind}: the second run differs")
            assert np.array_equal(mask.cpu().numpy(), m.mask)
        keep = second.decode_all().cpu().numpy().copy()
        del first, old
        junk = encode(kind, off, ids, True, BITS)
        assert np.array_equal(second.decode_all().cpu().numpy(), keep)  # the new object owns all of its memory
        del junk
        _torch().cuda.synchronize()
    finally:
        L.check(L.lib().vidc_ctx_debug_pool_poison(ctx.h, 0))


@pytest.mark.parametrize("kind", KINDS)
def test_empty_objects_and_objects_without_lists(kind):
    for nlist in (1, 6):
        off0 = np.zeros(nlist + 1, np.uint64)
        old = encode(kind, off0, np.zeros(0, np.uint64), True, BITS)
        for t, a1, a2 in ((0, 0, BIG), (1, 3, 1), (2, 0, 0), (3, 4, 2), (4, 0, 3)):
            new, mask = _subset().subset(old, t, a1, a2, want_perm=True)
            assert new.ntotal == 0 and mask.numel() == 0 and new.offsets.size == nlist + 1 and not new.offsets.any()
            same(img(kind, new), img(kind, old), f"{kind}: the subset of an empty object")


# ------------------------------------------------------------------------------------------------------------- status
def _raw(kind, ctx_h, obj_h, t, a1, a2, out, taken=None, n_taken=None, prec=-1):
    L = _lib().lib()
    p = _lib().ptr
    if kind == "packed":
        return L.vidc_packed_subset_dev(ctx_h, obj_h, t, a1, a2, out, p(taken), n_taken)
    if kind == "ef":
        return L.vidc_ef_subset_dev(ctx_h, obj_h, t, a1, a2, 0, out, p(taken), n_taken)
    return L.vidc_roc_subset_dev(ctx_h, obj_h, t, a1, a2, prec, 0, out, p(taken), n_taken)


@pytest.mark.parametrize("kind", KINDS)
def test_invalid_arguments(kind):
    L = _lib()
    ctx = L.default_context()
    off, ids = zipf(2000, 50, seed=71)
    ids = spread(ids)
    obj = encode(kind, off, ids, True, BITS)
    T = obj.ntotal
    bad = [(None, obj.h, 1, 2, 0), (ctx.h, None, 1, 2, 0), (ctx.h, obj.h, -1, 0, 0), (ctx.h, obj.h, 5, 0, 0),
           (ctx.h, obj.h, 1, 0, 0), (ctx.h, obj.h, 1, 3, 3), (ctx.h, obj.h, 2, 5, 4), (ctx.h, obj.h, 2, 0, T + 1), (ctx.h, obj.h, 3, 0, 0),
           (ctx.h, obj.h, 3, 2 ** 32, 0), (ctx.h, obj.h, 3, 4, 4)]
    for args in bad:
        out = C.c_void_p(12345)
        assert sr.refusal(args[0] is None or args[1] is None, args[2], args[3], args[4], T) != sr.OK
        assert _raw(kind, *args, C.byref(out)) == -1, args
        assert out.value is None, "*out must be NULL after an error"
        assert b"subset" in L.lib().vidc_last_error()
    assert _raw(kind, ctx.h, obj.h, 1, 2, 0, None) == -1
    if kind == "roc":
        for prec in (33, -3):
            out = C.c_void_p(12345)
            assert _raw(kind, ctx.h, obj.h, 1, 2, 1, C.byref(out), prec=prec) == -1 and out.value is None
    # the largest accepted arguments, the host count, and a NULL mask: the context is still usable, the object untouched
    out, n = C.c_void_p(), C.c_uint64(77)
    assert _raw(kind, ctx.h, obj.h, 2, 0, T, C.byref(out), None, C.byref(n)) == 0 and n.value == T
    getattr(L.lib(), {"packed": "vidc_packed_destroy", "ef": "vidc_ef_destroy", "roc": "vidc_roc_destroy"}[kind])(out)
    new, mask = _subset().subset(obj, 1, 4, 1, taken=False)
    assert mask is None and new.ntotal == int(sr.taken_mask(1, 4, 1, off, obj.decode_all().cpu().numpy().view(np.uint64)).sum())
    check_subset(kind, obj, 3, 2 ** 32 - 1, 2 ** 32 - 2)


def _status(fn):
    try:
        fn()
    except _lib().VidcError as ex:
        return int(str(ex).split("vidc status ")[1].split(":")[0])
    return 0


def test_graph_objects_are_unsupported():
    torch = _torch()
    from vector_db_id_compression_amd.codecs import EfLists, RocLists

    rng = np.random.default_rng(73)
    rows = np.full((300, 8), -1, np.int32)
    for i in range(300):
        k = int(rng.integers(1, 9))
        rows[i, :k] = np.sort(rng.choice(300, k, replace=False))
    d_rows = torch.from_numpy(rows).cuda()
    for kind, obj in (("roc", RocLists.encode_rows(d_rows)), ("ef", EfLists.encode_rows(d_rows))):
        before = obj.decode_rows(None, 8)[0].cpu().numpy()
        with pytest.raises(_lib().VidcError, match="graph"):
            _subset().subset(obj, 1, 2, 0)
        out = C.c_void_p(12345)
        assert _raw(kind, obj.ctx.h, obj.h, 4, 0, 5, C.byref(out)) == -6 and out.value is None  # VIDC_ERR_UNSUPPORTED through the C call
        assert np.array_equal(obj.decode_rows(None, 8)[0].cpu().numpy(), before)  # untouched and still usable


# ------------------------------------------------------------------------------------------------------------- the round trip
CONTAINERS = {"packed-bits": "dense", "elias-fano": "sparse", "roc": "sparse"}
GOLDEN_I64 = ch.GOLDEN - (1 << 64)


def _container(name, lists):
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    il = ArrayInvertedLists(len(lists), ch.CODE_SIZE)
    for l, li in enumerate(lists):
        if li.size:
            il.add_entries(l, li.view(np.int64), ch.code(li).view(np.uint8).reshape(-1, ch.CODE_SIZE))
    return ci.AVAILABLE_COMPRESSED_IVFS[name](il)


def _entries(il):
    """every list as a sorted array of ids, after checking that every row of codes_all is the payload of the id at its position"""
    torch = _torch()
    ids = il.get_ids_all()
    codes = il.codes_all.view(torch.int64).reshape(-1) if il.ntotal else ids
    assert torch.equal(codes, ids * GOLDEN_I64), "a code is attached to another id"
    host, o = ids.cpu().numpy().view(np.uint64), il._offsets.astype(np.int64)
    return [np.sort(host[o[l]:o[l + 1]]) for l in range(il.nlist)]


@pytest.mark.parametrize("split", [(sr.ID_MOD, 3), (sr.ID_MOD, 5), (sr.INVLIST_FRACTION, 3)], ids=["id_mod_3", "id_mod_5", "fraction_3"])
@pytest.mark.parametrize("name", list(CONTAINERS))
def test_a_container_split_in_three_and_merged_back(name, split):
    """copy_subset_to into three empty containers, merge_from of the three: every list is the original as a multiset, every entry with
    the payload computed from its id"""
    t, parts = split
    init, _ = ch.schedule(CONTAINERS[name])
    src = _container(name, init)
    want = _entries(src)
    empty = [np.zeros(0, np.uint64)] * ch.NLIST
    shards = [_container(name, empty) for _ in range(parts)]
    n = [src.copy_subset_to(shards[r], t, parts, r) for r in range(parts)]
    assert sum(n) == src.ntotal and [s.ntotal for s in shards] == n
    assert all(x > 0 for x in n) or (t, parts, CONTAINERS[name]) == (sr.ID_MOD, 3, "sparse")  # (the sparse ids 6 k + 3 are all 0 mod 3)
    m0 = ch.Model(init)
    for r, s in enumerate(shards):
        got = _entries(s)
        if t == sr.ID_MOD:
            for l in range(ch.NLIST):
                assert np.array_equal(got[l], np.sort(init[l][init[l] % np.uint64(parts) == r])), (name, r, l)
        else:
            sizes = m0.sizes()
            assert [g.size for g in got] == [int(k * (r + 1) // parts - k * r // parts) for k in sizes]
    whole = _container(name, empty)
    for s in shards:
        whole.merge_from(s, 0)
    assert whole.ntotal == src.ntotal and np.array_equal(whole._offsets, src._offsets)
    for a, b in zip(_entries(whole), want):
        assert np.array_equal(a, b)
    for a, b in zip(_entries(src), want):  # the source is unchanged
        assert np.array_equal(a, b)
    for attr in ("compressed_ids_size_in_bytes",):
        assert getattr(whole, attr) > 0


@pytest.mark.parametrize("name", ["packed-bits", "elias-fano", "roc"])
def test_index_copy_subset_to_in_step_with_a_twin(name):
    """IVFIndex.copy_subset_to on a compressed container and on a twin over ArrayInvertedLists: the same parts list by list, and the
    parts merged back are the index"""
    from test_gpu_churn import _index_data, _new_index
    from vector_db_id_compression_amd import custom_invlists as ci

    torch = _torch()
    cent, batches, _ = _index_data()
    a, twin = _new_index(cent), _new_index(cent)
    a.add(batches[0])
    twin.add(batches[0])
    ci.apply_id_compression(a, name)
    rows = batches[0]

    def fresh(compressed):
        ix = _new_index(cent)
        if compressed:
            ci.apply_id_compression(ix, name)
        return ix

    def lists(ix):
        il = ix.invlists
        if hasattr(il, "get_ids_all"):
            ids, o = il.get_ids_all().cpu().numpy(), il._offsets.astype(np.int64)
            return [np.sort(ids[o[l]:o[l + 1]]) for l in range(il.nlist)]
        return [np.sort(il.get_ids(l)) for l in range(il.nlist)]

    whole, whole_twin = fresh(True), fresh(False)
    T = a.ntotal
    for t, splits in ((sr.ID_MOD, [(3, 0), (3, 1), (3, 2)]), (sr.INVLIST_FRACTION, [(3, 0), (3, 1), (3, 2)]),
                      (sr.ID_RANGE, [(0, T // 3), (T // 3, BIG)]), (sr.ELEMENT_RANGE, [(0, T // 2)]), (sr.INVLIST, [(0, 4), (4, 900)])):
        for a1, a2 in splits:
            part, part_twin = fresh(True), fresh(False)
            n = a.copy_subset_to(part, t, a1, a2)
            assert n == twin.copy_subset_to(part_twin, t, a1, a2) == part.ntotal == part_twin.ntotal == part.invlists.ntotal
            by_position = t in (sr.ELEMENT_RANGE, sr.INVLIST_FRACTION) and name == "roc"
            for x, y, z in zip(lists(part), lists(part_twin), lists(a)):
                if by_position:  # (positions are those of the container's own order -- ROC: sampling order, the twin: add order)
                    assert x.size == y.size and np.isin(x, z).all(), (name, t, a1, a2)
                else:
                    assert np.array_equal(x, y), (name, t, a1, a2)
            if n:  # Flat codes: the stored vector of every id of the part, bit for bit
                some = np.concatenate(lists(part))[:200]
                got = part.reconstruct_batch(torch.from_numpy(some).cuda()).cpu().numpy()
                assert np.array_equal(got.view(np.int32), rows[some].view(np.int32))
            if t == sr.ID_MOD:
                whole.merge_from(part, add_id=0)
                whole_twin.merge_from(part_twin, add_id=0)
    assert whole.ntotal == whole_twin.ntotal == T and a.ntotal == T
    for x, y, z in zip(lists(whole), lists(whole_twin), lists(a)):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    live = np.arange(T)
    got = whole.reconstruct_batch(torch.from_numpy(live).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.int32), rows.view(np.int32))
