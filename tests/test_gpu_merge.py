"""Merge two compressed list objects on the device (vidc_*_merge_dev): the new object is the one the ordinary encoder builds from
M_l = a_l ++ [x + add_id for x in b_l], word for word; `src` says where every entry came from; both sources stay untouched; ROC
re-encodes only the lists that hold ids of both sides (or shifted ids of b); no id payload moves over PCIe.

M and src come from tests/merge_ref.py and the sources' own decode_all.  Ids are distinct inside every merged list (the IVF case)."""
import numpy as np
import pytest

import merge_ref as mr
from test_gpu_dev_offsets import dev, ef_image, packed_image, roc_image, same

pytestmark = pytest.mark.gpu

KINDS = ["packed", "ef", "wt", "wt1", "roc"]
U = 1 << 19        # ids of either side are below U; add_id = U keeps the merged lists distinct, and below 2^20 (ROC's 20-bit list class)
GUARD = 64
SENTINEL = -0x5A5A5A5A5A5A5A5B
EDGE = (0, 1, 1023, 1024, 1025)
# every pair of edge lengths (b's destination takes every offset mod 2 elements against its source), lists that end a chunk exactly,
# merged ROC lists that cross the 64 / 1024 / 2048 / 4096 class seams from below, a 20-bit chain list made of both sides, and lists
# of the chain class that are one-sided on either side
SIZES_A = [a for a in EDGE for _ in EDGE] + [2048, 1024, 60, 1000, 2000, 4000, 3000, 0, 5000]
SIZES_B = [b for _ in EDGE for b in EDGE] + [1024, 2048, 10, 100, 100, 200, 3000, 5000, 0]


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def _merge():
    from vector_db_id_compression_amd import merge

    return merge


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def make_ids(kind, sizes, seed, lo=0, hi=U):
    """distinct ids per list in [lo, hi), in random order (ascending for Elias-Fano's sake nowhere: the codecs sort or keep as they
    like); wavelet tree: a permutation of 0 .. ntotal - 1, ascending inside every list"""
    rng = np.random.default_rng(seed)
    off = offsets(sizes)
    if kind.startswith("wt"):
        lst = np.repeat(np.arange(len(sizes)), np.asarray(sizes, dtype=np.int64))
        rng.shuffle(lst)
        return off, np.argsort(lst, kind="stable").astype(np.uint64)
    ids = np.empty(int(off[-1]), np.uint64)
    for l, n in enumerate(sizes):
        if n:
            # no 0 and no power of two, before or after a shift by U: a list whose maximum is one is a lossy case of the reference
            # codec (include/vidc.h, "append"), where even the from-scratch object does not decode to its input -- with thousands of
            # one-id lists that is no rare draw (id 0 of b shifted to 2^19 was one)
            u = np.unique(rng.integers(lo + 1, hi - 1, 2 * n + 24, dtype=np.uint64))
            u = u[(u & (u - np.uint64(1))) != 0]
            ids[int(off[l]):int(off[l + 1])] = u[rng.permutation(u.size)[:n]]
    return off, ids


def encode(kind, off, ids, want_perm=True, bits=None, ctx=None):
    cd, torch = _codecs(), _torch()
    d = dev(ids) if int(off[-1]) else torch.zeros(0, dtype=torch.int64, device="cuda")
    if kind == "packed":
        return cd.PackedLists.encode(off, d, bits=bits, ctx=ctx)
    if kind == "ef":
        return cd.EfLists.encode(off, d, want_perm=want_perm, ctx=ctx)
    if kind == "roc":
        return cd.RocLists.encode(off, d, want_perm=want_perm, ctx=ctx)
    return cd.WaveletTreeLists.build(off, d, wt_type=1 if kind == "wt1" else 0, ctx=ctx)


def image(kind, obj, want_perm=True):
    if kind == "packed":
        return dict(offsets=obj.offsets, **packed_image(obj))
    if kind == "ef":
        d = dict(offsets=obj.offsets, **ef_image(obj, want_perm))
        if not np.any(d["sizes"].astype(np.uint64) * d["low_bits"]):
            d.pop("low")  # no list has a low bit: the export is one padding word, which the device-offsets encoder leaves unwritten
        return d
    if kind == "roc":
        return dict(offsets=obj.offsets, ntotal=obj.ntotal, **roc_image(obj, want_perm))
    # the wavelet tree has no per-list export: its geometry, sizes and every id it answers
    return dict(offsets=obj.offsets, size=obj.size_in_bytes, levels=obj.levels, ids=obj.decode_all().cpu().numpy())


def decoded(obj):
    return obj.decode_all().cpu().numpy().view(np.uint64).copy()


def merge_args(kind, want_perm, bits):
    return dict(bits=bits) if kind == "packed" else dict(want_perm=want_perm) if kind in ("ef", "roc") else {}


def status_of(fn):
    from vector_db_id_compression_amd import VidcError

    try:
        fn()
    except VidcError as e:
        import re

        return int(re.search(r"vidc status (-?\d+)", str(e)).group(1))
    return 0


def check_merge(kind, a, b, add_id, want_perm=True, bits=None, src_perm=(True, True)):
    """merge a and b; compare with the from-scratch encode of M, src with the model, translate_labels of every position, both
    sources before and after, the d2h counter -> (new, m)"""
    torch = _torch()
    ctx = a.ctx
    dec_a, dec_b = decoded(a), decoded(b)
    m = mr.merge(a.offsets, dec_a, b.offsets, dec_b, add_id)
    n = int(m.offsets[-1])
    before = (image(kind, a, src_perm[0]), image(kind, b, src_perm[1]))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    src = buf[GUARD:GUARD + n]
    d2h = ctx.d2h_bytes()
    new = _merge().merge(a, b, add_id, src=src, **merge_args(kind, want_perm, bits))
    assert ctx.d2h_bytes() == d2h, f"{kind}: a merge moved id payload to the host"
    assert ctx.last_kernel_ms() > 0 or n == 0
    scratch = encode(kind, m.offsets, m.ids, want_perm, (bits or a.bits) if kind == "packed" else None, ctx=ctx)
    same(image(kind, new, want_perm), image(kind, scratch, want_perm), f"{kind} merge")
    new_dec = decoded(new)
    assert np.array_equal(new_dec, decoded(scratch))
    # src: the model's, guard bands intact, and the gather through it rebuilds what the new object decodes to
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + n:] == SENTINEL), f"{kind}: src was written outside its {n} entries"
    s = host[GUARD:GUARD + n]
    if kind == "ef":
        want = mr.src("ascending", m)
    elif kind == "roc":
        want = mr.src("perm", m, new.perm()) if want_perm else None
    else:
        want = mr.src("plain", m)
    if want is not None:
        assert np.array_equal(s, want), f"{kind}: src differs from the model"
    assert np.array_equal(np.sort(s[s >= 0]), np.arange(dec_a.size)) and np.array_equal(np.sort(~s[s < 0]), np.arange(dec_b.size))
    with np.errstate(over="ignore"):
        both = np.concatenate([dec_a, dec_b + np.uint64(add_id)])
    assert np.array_equal(both[np.where(s >= 0, s, dec_a.size + ~s)], new_dec), f"{kind}: the gather through src is not the new object"
    # translate_labels of every position
    if n:
        off = m.offsets.astype(np.int64)
        lists = np.repeat(np.arange(m.nlist), off[1:] - off[:-1])
        lab = torch.from_numpy((lists << 32) | (np.arange(n) - off[lists])).cuda()
        assert np.array_equal(new.translate_labels(lab).cpu().numpy().view(np.uint64), new_dec)
    same(image(kind, a, src_perm[0]), before[0], f"{kind}: a changed")
    same(image(kind, b, src_perm[1]), before[1], f"{kind}: b changed")
    return new, m


def pair(kind, sizes_a, sizes_b, seed=1, want_perm=True, bits=None, ctx=None, disjoint=False):
    """two objects; disjoint: b's ids lie above a's (for merges with add_id 0)"""
    a_off, a_ids = make_ids(kind, sizes_a, seed)
    b_off, b_ids = make_ids(kind, sizes_b, seed + 1000, *((U, 2 * U) if disjoint and not kind.startswith("wt") else (0, U)))
    return encode(kind, a_off, a_ids, want_perm, bits, ctx), encode(kind, b_off, b_ids, want_perm, bits, ctx)


def shift_for(kind, a):
    return a.ntotal if kind.startswith("wt") else U


# ------------------------------------------------------------------------------------------------------------- equality
@pytest.mark.parametrize("kind", KINDS)
def test_every_alignment_chunk_edge_and_class_seam(kind):
    a, b = pair(kind, SIZES_A, SIZES_B, bits=21 if kind == "packed" else None)
    ctx = a.ctx
    new, m = check_merge(kind, a, b, shift_for(kind, a))
    if kind == "roc":
        # an upper bound only: at most the three re-encoded lists of the chain class (4200, 6000 and b's shifted 5000) went through
        # the chain launch, and none longer than 6000 (a kernel family without a chain class reports 0).  That a kept list runs no
        # chain at all is what test_one_sided_lists asserts; a list wrongly kept here is caught by the word-for-word compare above
        new2 = _merge().merge(a, b, U)
        for which in (0, 1):
            info = ctx.chain_info(which)
            assert info["lists"] <= 3 and info["longest"] <= 6000, (which, info)
        assert np.array_equal(new2.all_words(), new.all_words())  # the same on every run
        assert np.array_equal(mr.roc_classes(m, U) == mr.ENCODE, (m.a_n + m.b_n > 0) & (m.b_n > 0))


@pytest.mark.parametrize("kind", ["packed", "ef", "roc"])
def test_one_sided_lists(kind):
    """lists cut by list parity: every list holds ids of one side only.  With add_id 0 ROC keeps every stream -- no ANS chain runs,
    on either side of the codec --, with a shift b's lists are re-encoded"""
    sizes = np.array([5000, 4500, 0, 700, 64, 65, 1, 1024, 1025, 4097, 0, 3], np.int64)
    sa, sb = np.where(np.arange(sizes.size) % 2 == 0, sizes, 0), np.where(np.arange(sizes.size) % 2 == 1, sizes, 0)
    a, b = pair(kind, sa.tolist(), sb.tolist(), seed=3, disjoint=True, bits=22 if kind == "packed" else None)
    ctx = a.ctx
    new, m = check_merge(kind, a, b, 0)
    if kind == "roc":
        _merge().merge(a, b, 0)
        for which in (0, 1):
            assert ctx.chain_info(which)["lists"] == 0 and ctx.chain_info(which)["ids"] == 0, "a kept list went through an ANS chain"
        assert not np.any(mr.roc_classes(m, 0) == mr.ENCODE)
        assert np.array_equal(new.perm(), mr.identity_perm(m))
    check_merge(kind, a, b, 7)
    check_merge(kind, b, a, 7)


@pytest.mark.parametrize("kind", KINDS)
def test_small_and_empty_objects(kind):
    for sa, sb in (([9], [4]), ([0], [4]), ([9], [0]), ([0, 0, 0], [0, 0, 0]), ([3, 0, 2], [0, 0, 0]), ([0, 0], [1, 5])):
        a, b = pair(kind, sa, sb, seed=5, bits=21 if kind == "packed" else None)
        new, m = check_merge(kind, a, b, shift_for(kind, a))
        if not sum(sb):  # (the permutation aside: a derived object's is over what a decodes to)
            same(image(kind, new, False), image(kind, a, False), f"{kind}: an empty b must give an object equal to a")
    a, _ = pair(kind, [40, 0, 1025, 7], [0, 0, 0, 0], seed=6, bits=21 if kind == "packed" else None)
    check_merge(kind, a, a, shift_for(kind, a))  # a is b: the halves are told apart by the sign of src


def test_elias_fano_ids_above_2_32():
    a, b = pair("ef", [100, 0, 1025, 3], [7, 1024, 2000, 0], seed=7)
    new, _ = check_merge("ef", a, b, (1 << 33) + 5)
    assert int(decoded(new).max()) > 1 << 33
    check_merge("ef", a, b, 1 << 62, want_perm=False)
    assert status_of(lambda: _merge().merge(a, b, (1 << 64) - 1)) == -4  # the shifted id leaves 64 bits


def test_packed_width_kept_widened_and_too_narrow():
    a, b = pair("packed", [100, 0, 1025, 3], [7, 1024, 2000, 0], seed=8, bits=20)
    new, _ = check_merge("packed", a, b, U)  # kept: ids below 2^20 fit
    assert new.bits == 20
    new, _ = check_merge("packed", a, b, U, bits=40)
    assert new.bits == 40
    before = (image("packed", a), image("packed", b))
    assert status_of(lambda: _merge().merge(a, b, 1 << 20)) == -4
    assert status_of(lambda: _merge().merge(a, b, U, bits=19)) == -4
    same(image("packed", a), before[0], "a after a refusal")
    same(image("packed", b), before[1], "b after a refusal")
    check_merge("packed", a, b, 1 << 20, bits=21)  # a following merge succeeds


def test_roc_domain_refusals():
    cd = _codecs()
    big = mr.ROC_MAX_LIST
    a_off = offsets([big, 3])
    a = cd.RocLists.encode(a_off, dev(np.concatenate([np.arange(big), [5, 6, 9]]).astype(np.uint64)))
    b = encode("roc", offsets([1, 2]), np.array([big + 7, 100, 200], np.uint64))
    before = (roc_image(a, False), roc_image(b, False))
    assert status_of(lambda: _merge().merge(a, b, 0)) == -4  # list 0 would hold VIDC_ROC_MAX_LIST + 1 ids
    same(roc_image(a, False), before[0], "a after a refusal")
    c = encode("roc", offsets([0, 2]), np.array([101, (1 << 31) - 11], np.uint64))
    assert status_of(lambda: _merge().merge(a, c, 11)) == -4  # a shifted id of 2^31
    same(roc_image(a, False), before[0], "a after a refusal")
    new = _merge().merge(a, c, 10)  # 2^31 - 1 is inside the domain, and the long list keeps its stream
    assert int(new.decode_lists([1])[0].max().item()) == (1 << 31) - 1 and new.ntotal == big + 5
    assert np.array_equal(new.words(0), a.words(0))
    assert status_of(lambda: _merge().merge(a, b, 0, precision_mode=33)) == -1
    g = cd.RocLists.encode_rows(np.array([[1, 2, -1], [0, -1, -1]], np.int32))
    assert status_of(lambda: _merge().merge(g, g, 0)) == -6
    other = encode("roc", offsets([1, 2, 3]), np.arange(6, dtype=np.uint64))
    assert status_of(lambda: _merge().merge(a, other, 0)) == -1  # nlist differs
    check_merge("roc", b, c, 0)  # the context stays usable


def raw_merge(kind, a, b, add_id, bits=0, precision_mode=-1):
    """the C call itself, *out preset to a non-NULL value -> (status, *out afterwards)"""
    import ctypes as C

    L = _lib().lib()
    out = C.c_void_p(0xDEAD)
    head = (a.ctx.h, a.h, b.h, int(add_id))
    if kind == "packed":
        st = L.vidc_packed_merge_dev(*head, int(bits), C.byref(out), None)
    elif kind == "ef":
        st = L.vidc_ef_merge_dev(*head, 0, C.byref(out), None)
    elif kind == "roc":
        st = L.vidc_roc_merge_dev(*head, int(precision_mode), 0, C.byref(out), None)
    else:
        st = L.vidc_wt_merge_dev(*head, C.byref(out), None)
    return st, out.value


@pytest.mark.parametrize("kind", KINDS)
def test_every_refusal_leaves_out_null_and_the_context_usable(kind):
    """the refusals that look into the objects -- another list count for every codec, and each codec's own: a width that is too
    narrow, a graph object, a list above VIDC_ROC_MAX_LIST, a shifted id of 2^31 or past 64 bits, a bad precision mode, a broken
    permutation -- set *out to NULL, leave both sources as they were, and a merge that follows succeeds.  (ntotal(a) + ntotal(b) >=
    2^32 - 1 needs objects of four billion ids: that refusal is held to the model through csrc/merge_plan.h alone.)"""
    cd = _codecs()
    a, b = pair(kind, [40, 0, 700, 3], [7, 1024, 0, 2], seed=21, bits=20 if kind == "packed" else None)
    other, _ = pair(kind, [5, 5, 5], [0, 0, 0], seed=22, bits=20 if kind == "packed" else None)
    before = (image(kind, a), image(kind, b))
    cases = [(a, other, 0, {}, -1), (other, a, 0, {}, -1)]
    if kind == "packed":
        cases += [(a, b, 1 << 20, {}, -4), (a, b, U, dict(bits=19), -4), (a, b, U, dict(bits=65), -1)]
    elif kind == "ef":
        g = cd.EfLists.encode_rows(np.array([[1, 2, -1], [0, -1, -1], [1, -1, -1], [0, 2, -1]], np.int32))
        cases += [(a, b, (1 << 64) - 1, {}, -4), (a, g, 0, {}, -6), (g, a, 0, {}, -6)]
    elif kind == "roc":
        g = cd.RocLists.encode_rows(np.array([[1, 2, -1], [0, -1, -1], [1, -1, -1], [0, 2, -1]], np.int32))
        cases += [(a, b, 1 << 31, {}, -4), (a, b, U, dict(precision_mode=33), -1), (a, b, U, dict(precision_mode=-3), -1),
                  (a, g, 0, {}, -6), (g, a, 0, {}, -6)]
    else:
        m = mr.merge(a.offsets, decoded(a), b.offsets, decoded(b), a.ntotal + 1)
        cases += [(a, b, a.ntotal + 1, {}, status_of(lambda: encode(kind, m.offsets, m.ids)))]
    for x, y, add_id, kw, want in cases:
        st, out = raw_merge(kind, x, y, add_id, **kw)
        assert st == want and st != 0 and out is None, (kind, add_id, kw, st, want, out)
        assert status_of(lambda: _merge().merge(x, y, add_id, **kw)) == want
    same(image(kind, a), before[0], f"{kind}: a after the refusals")
    same(image(kind, b), before[1], f"{kind}: b after the refusals")
    check_merge(kind, a, b, shift_for(kind, a))


def test_a_subclass_instance_merges_into_an_object_of_the_list_class():
    """the inner object of a segmented container is a RocLists subclass that borrows its handle and constructs differently: the merge
    takes it and returns a plain RocLists that owns the new handle"""
    cd = _codecs()
    off, ids = make_ids("roc", [3000, 10, 0], 26)
    seg = cd.RocSegLists.encode(off, dev(ids))
    inner = seg.inner
    assert type(inner) is not cd.RocLists and isinstance(inner, cd.RocLists)
    new = _merge().merge(inner, inner, U)
    assert type(new) is cd.RocLists and new.ntotal == 2 * inner.ntotal
    d = decoded(inner)
    m = mr.merge(inner.offsets, d, inner.offsets, d, U)
    assert np.array_equal(np.sort(decoded(new)), np.sort(m.ids)) and np.array_equal(new.offsets, m.offsets)


@pytest.mark.parametrize("kind", KINDS)
def test_more_lists_than_one_scan_tile(kind):
    """9000 short lists (the scans of the offsets, of the ROC classes and of the chunk tables leave their one-workgroup form above
    8192 entries): empty, one-sided and two-sided lists mixed, so ROC reads back a few thousand (list, size) pairs"""
    rng = np.random.default_rng(23)
    nlist = 9000
    sa, sb = rng.integers(0, 7, nlist), rng.integers(0, 7, nlist)
    sa[rng.random(nlist) < 0.3] = 0
    sb[rng.random(nlist) < 0.3] = 0
    a, b = pair(kind, sa.tolist(), sb.tolist(), seed=24, bits=21 if kind == "packed" else None)
    new, m = check_merge(kind, a, b, shift_for(kind, a))
    if kind == "roc":
        cls = mr.roc_classes(m, U)
        assert np.count_nonzero(cls == mr.ENCODE) > 2000 and np.count_nonzero(cls == mr.KEEP_A) > 2000
        a0, b0 = pair(kind, sa.tolist(), sb.tolist(), seed=25, disjoint=True)
        _, m0 = check_merge(kind, a0, b0, 0)
        assert np.count_nonzero(mr.roc_classes(m0, 0) == mr.KEEP_B) > 1000


@pytest.mark.parametrize("kind", ["wt", "wt1"])
def test_wavelet_tree_add_id_that_breaks_the_permutation(kind):
    a, b = pair(kind, [30, 0, 600, 5], [100, 40, 0, 2], seed=9)
    for bad in (a.ntotal + 1, 0, a.ntotal - 1):
        m = mr.merge(a.offsets, decoded(a), b.offsets, decoded(b), bad)
        st = status_of(lambda: encode(kind, m.offsets, m.ids))
        assert st != 0 and status_of(lambda: _merge().merge(a, b, bad)) == st
    check_merge(kind, a, b, a.ntotal)


# ------------------------------------------------------------------------------------------------------------- modes
@pytest.mark.parametrize("hook", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
def test_roc_kernel_families(hook, monkeypatch):
    for h in ("VIDC_FORCE_GENERAL", "VIDC_NO_LANE"):
        monkeypatch.delenv(h, raising=False)
    a, b = pair("roc", SIZES_A, SIZES_B, seed=11)
    plain = _merge().merge(a, b, U, want_perm=True)
    monkeypatch.setenv(hook, "1")
    new, _ = check_merge("roc", a, b, U)
    same(roc_image(new, True), roc_image(plain, True), f"{hook}: another stream than the default families'")


@pytest.fixture(scope="module")
def small_ctx():
    """a context created under VIDC_NUM_CU=1 with the pool poison on: the chunk loops of a 16-workgroup grid take 64 chunks a trip"""
    L, torch = _lib(), _torch()
    torch.cuda.set_device(0)
    mp = pytest.MonkeyPatch()
    mp.setenv("VIDC_NUM_CU", "1")
    c = L.Context(0)
    mp.undo()
    assert c.num_cu() == 1
    c.set_pool_poison(True)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.synchronize()
    c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_one_compute_unit_and_poisoned_pool(kind, small_ctx):
    """150 lists of about 1500 ids a side: 300 chunks of a, 300 of b, 450 of the new object -- five to eight trips of 64, the last
    one ragged"""
    rng = np.random.default_rng(13)
    sa, sb = (1400 + rng.integers(0, 200, 150)).tolist(), (1400 + rng.integers(0, 200, 150)).tolist()
    for s in (sa, sb):
        chunks = sum((n + 1023) // 1024 for n in s)
        assert chunks > 192 and chunks % 64
    a, b = pair(kind, sa, sb, seed=14, ctx=small_ctx, bits=21 if kind == "packed" else None)
    check_merge(kind, a, b, shift_for(kind, a))


# ------------------------------------------------------------------------------------------------------------- compositions
@pytest.mark.parametrize("kind", ["packed", "ef", "roc", "wt"])
def test_merges_of_merged_appended_shrunk_and_loaded_objects(kind, tmp_path):
    from vector_db_id_compression_amd import locate, persist, removal

    torch = _torch()
    sizes_a, sizes_b = [100, 0, 1025, 3, 70], [7, 1024, 200, 0, 64]
    a, b = pair(kind, sizes_a, sizes_b, seed=15, bits=24 if kind == "packed" else None)
    shift = shift_for(kind, a)
    ab, m = check_merge(kind, a, b, shift)                                   # merged
    top = int(m.ids.max()) + 1
    # appended: ids above everything, one per list
    ln = torch.arange(5, dtype=torch.int64, device="cuda")
    more, _ = ab.append(ln, top + ln)
    loaded = persist.load(persist.save(more, str(tmp_path / f"{kind}.npz")))  # loaded (no permutation of its own)
    c_off, c_ids = make_ids(kind, [5, 5, 0, 900, 1], 16)
    c = encode(kind, c_off, c_ids, bits=24 if kind == "packed" else None)
    shift2 = loaded.ntotal if kind == "wt" else 4 * U
    new, m2 = check_merge(kind, loaded, c, shift2, src_perm=(False, True))   # merged + appended + loaded, with a fresh one
    if kind == "wt":
        return
    # shrunk: drop every third entry of the merge, then merge the rest with c again (other ids: another shift)
    def lists_of(off):
        off = np.asarray(off, dtype=np.int64)
        return torch.from_numpy(np.repeat(np.arange(off.size - 1), off[1:] - off[:-1])).cuda()

    dec = torch.from_numpy(decoded(new).view(np.int64)).cuda()
    shrunk, mask = removal.remove(new, lists_of(new.offsets)[::3].contiguous(), dec[::3].contiguous(), want_perm=True)
    assert int(mask.sum().item()) == (dec.numel() + 2) // 3
    again, m3 = check_merge(kind, shrunk, c, 8 * U)
    # a merge followed by a remove and a locate: the survivors are found where translate_labels reads them
    ln3 = lists_of(m3.offsets)
    gone, ln_gone = torch.from_numpy(m3.ids[1::2].view(np.int64).copy()).cuda(), ln3[1::2].contiguous()
    left, _ = removal.remove(again, ln_gone, gone, want_perm=True)
    stay, ln_stay = torch.from_numpy(m3.ids[0::2].view(np.int64).copy()).cuda(), ln3[0::2].contiguous()
    lab = locate.locate(left, ln_stay, stay)
    assert int((lab < 0).sum().item()) == 0 and torch.equal(left.translate_labels(lab), stay)
    assert torch.equal(lab >> 32, ln_stay)
    assert int((locate.locate(left, ln_gone, gone) >= 0).sum().item()) == 0


def _containers():
    from vector_db_id_compression_amd import custom_invlists as ci

    return {"packed": ci.CompressedIDInvertedListsPackedBits, "roc": ci.CompressedIDInvertedListsFenwickTree,
            "ef": ci.CompressedIDInvertedListsEliasFano, "wt": ci.CompressedIDInvertedListsWaveletTree}


@pytest.mark.parametrize("kind", ["packed", "roc", "ef", "wt"])
def test_containers_merge_from(kind):
    """merge_from on every container with codes: ids, codes, offsets and the size attributes of a fresh container over the merged
    lists; `other` unchanged"""
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    rng = np.random.default_rng(17)
    nlist, na, nb, cs = 12, 3000, 2000, 6
    asg_a, asg_b = rng.integers(0, nlist, na), rng.integers(0, nlist - 2, nb)  # (b leaves two lists empty)
    codes_a, codes_b = rng.integers(0, 256, (na, cs), dtype=np.uint8), rng.integers(0, 256, (nb, cs), dtype=np.uint8)
    il_a, il_b = ArrayInvertedLists.from_assignment(asg_a, nlist, codes_a), ArrayInvertedLists.from_assignment(asg_b, nlist, codes_b)
    il_all = ArrayInvertedLists.from_assignment(asg_a, nlist, codes_a)
    for l in range(nlist):
        il_all.add_entries(l, il_b.get_ids(l) + na, il_b.get_codes(l))
    cls = _containers()[kind]
    A, B, want = cls(il_a), cls(il_b), cls(il_all)
    b_ids, b_codes = B.get_ids_all().clone(), B.codes_all.clone()
    A.merge_from(B, na)
    assert A.ntotal == na + nb and np.array_equal(A._offsets, want._offsets) and A.compute_ntotal() == want.ntotal
    assert _torch().equal(A.get_ids_all(), want.get_ids_all())
    assert _torch().equal(A.codes_all, want.codes_all)
    for attr in ("compressed_ids_size_in_bytes", "codes_size_in_bytes", "bits"):
        if hasattr(want, attr):
            assert getattr(A, attr) == getattr(want, attr), attr
    if kind == "roc":
        assert np.array_equal(A.id_symbol_precision, want.id_symbol_precision)
    assert B.ntotal == nb and _torch().equal(B.get_ids_all(), b_ids) and _torch().equal(B.codes_all, b_codes)
    odd = cls.__new__(cls)
    odd.nlist, odd.code_size = nlist + 1, cs
    with pytest.raises(ValueError, match="nlist"):
        A.merge_from(odd, 0)


@pytest.mark.parametrize("kind", ["none", "packed", "roc", "ef", "wt"])
def test_ivf_merge_from_two_halves(kind):
    """two halves of 4096 Flat vectors against an index that added all of them: the same search results and reconstructions"""
    from vector_db_id_compression_amd import ivf

    rng = np.random.default_rng(19)
    n, d, nlist = 4096, 8, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    full = ivf.IVFIndex(d, nlist)
    full.train(x)

    def index(rows):
        ix = ivf.IVFIndex(d, nlist)
        ix.centroids = full.centroids
        ix.add(x[rows])
        if kind != "none":
            ix.replace_invlists(_containers()[kind](ix.invlists))
        return ix

    full.add(x)
    a, b = index(slice(0, n // 2)), index(slice(n // 2, n))
    a.merge_from(b)
    assert a.ntotal == n and a._next_id == n and b.ntotal == n // 2
    for ix in (a, full):
        ix.nprobe = 4
    xq = x[::64] + 0.01
    D0, I0 = full.search(xq, 10)
    D1, I1 = a.search(xq, 10)
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    ids = rng.permutation(n)[:300]
    assert np.array_equal(a.reconstruct_batch(ids).cpu().numpy(), x[ids])
    other = ivf.IVFIndex(d, nlist)
    other.centroids = full.centroids + 1
    with pytest.raises(ValueError, match="centroids"):
        a.merge_from(other)
