"""Remove (list, id) batches from compressed lists on the device (vidc_*_remove_dev): the new object is the one the ordinary encoder
builds from the surviving lists, word for word; the mask names the removed positions; missing and invalid pairs are counted; the old
object is untouched; ROC decodes the candidates and re-encodes only the lists that lose an entry; nothing moves id payload over PCIe.

The surviving CSR S comes from tests/remove_ref.py and the old object's own decode_all.  ROC inputs are lists the reference codec
round-trips (distinct ids, no power-of-two maximum, at most 65 536 ids; include/vidc.h says why): ids here are 6 * k + 3, odd multiples
of three, so no list and no surviving list has a power-of-two maximum; check_roundtrips holds that against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import remove_ref as rr
from test_gpu_append import dev_i64, encode, image
from test_gpu_dev_offsets import dev, same, sorted_lists, zipf

pytestmark = pytest.mark.gpu

KINDS = ["packed", "ef", "roc"]
MODES = ["pairs", "any"]
BITS = 24  # packed width of the ordinary cases: ids below 2^24


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _removal():
    from vector_db_id_compression_amd import removal

    return removal


def spread(ids):
    """k -> 6 k + 3: distinct stays distinct, ascending stays ascending, nothing is a power of two"""
    return (6 * np.asarray(ids, dtype=np.uint64) + 3).astype(np.uint64)


def check_roundtrips(oracle, off, ids):
    """the lists are ones the reference ROC codec reproduces under VIDC_PREC_REFERENCE"""
    off = np.asarray(off).astype(np.int64)
    for l in range(off.size - 1):
        li = ids[off[l]:off[l + 1]]
        if li.size:
            assert li.size <= 65536 and np.unique(li).size == li.size and int(li.max()) < (1 << 31)
            assert int(li.max()) == 0 or int(li.max()) < (1 << oracle.list_precision(li)), f"list {l}: the reference codec is lossy here"


def img(kind, obj, want_perm=True):
    """image() of test_gpu_append.  An Elias-Fano object without ids has no stream, but reports and exports one padding word per
    stream that no encoder writes: those two words are not part of the object and stay out of the comparison."""
    d = image(kind, obj, want_perm)
    if kind == "ef" and obj.ntotal == 0:
        assert d["low"].size == 1 and d["high"].size == 1 and d["bytes"] == 0
        d["low"], d["high"] = d["low"][:0], d["high"][:0]
    return d


def zeros1():
    return _torch().zeros(1, dtype=_torch().int64, device="cuda")


def remove(old, ln, rm, want_perm=True, **kw):
    torch = _torch()
    d_ln = None if ln is None else dev_i64(ln)
    d_rm = dev(rm) if np.asarray(rm).size else torch.zeros(0, dtype=torch.int64, device="cuda")
    return _removal().remove(old, d_ln, d_rm, want_perm=want_perm, **kw)


def check_remove(kind, off, ids, ln, rm, want_perm=True, bits=BITS, old=None, oracle=None):
    """remove from `old` (default: a fresh encode of (off, ids)); compare with the from-scratch encode of S, the mask, the counts and
    the old object's image -> (old, new, model)"""
    ctx = _lib().default_context()
    if old is None:
        if kind == "roc" and oracle is not None:
            check_roundtrips(oracle, off, ids)
        old = encode(kind, off, ids, want_perm, bits)
    ln = None if ln is None else np.asarray(ln, dtype=np.int64)
    rm = np.asarray(rm, dtype=np.uint64)
    old_dec = old.decode_all().cpu().numpy().view(np.uint64)
    m = rr.remove(old.offsets, old_dec, ln, rm)
    before = img(kind, old, want_perm)
    mis, inv = zeros1(), zeros1()
    d2h = ctx.d2h_bytes()
    new, mask = remove(old, ln, rm, want_perm, missing=mis, invalid=inv)
    assert ctx.d2h_bytes() == d2h, f"{kind}: a remove moved id payload to the host"
    scratch = encode(kind, m.offsets, m.ids, want_perm, old.bits if kind == "packed" else None)
    same(img(kind, new, want_perm), img(kind, scratch, want_perm), f"{kind} remove")
    assert np.array_equal(mask.cpu().numpy(), m.mask), f"{kind}: the removed mask differs from the model"
    assert (int(mis.item()), int(inv.item())) == (m.missing, m.invalid), f"{kind}: (missing, invalid)"
    assert new.ntotal == old.ntotal - m.removed
    same(img(kind, old, want_perm), before, f"{kind}: the old object changed")
    return old, new, m


def lists_of(pos, off):
    return (np.searchsorted(np.asarray(off).astype(np.int64), pos, side="right") - 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- the batch
@pytest.fixture(scope="module")
def zipf300():
    """300 lists (the list key takes two radix passes), 30 000 ids"""
    off, ids = zipf(30_000, 300, seed=31)
    return off, spread(ids)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_rm", [1, 64, 65, 1023, 1024, 1025, 5000])
def test_batch_sizes_on_the_sorter_rounds_and_tiles(kind, mode, n_rm, zipf300, oracle):
    """half the pairs hit; the rest name an absent id or a present id under the wrong list, a negative or too large list number, or
    repeat an earlier pair"""
    off, ids = zipf300
    rng = np.random.default_rng(200 + n_rm)
    nlist = off.size - 1
    pos = rng.choice(ids.size, n_rm, replace=n_rm > ids.size // 2)
    rm, ln = ids[pos].copy(), lists_of(pos, off)
    what = rng.integers(0, 10, n_rm) if n_rm > 1 else np.zeros(1, np.int64)  # 0-4 hit
    rm[what == 5] += 1                                                            # an id no list holds (6 k + 4)
    wrong = what == 6                                                             # a present id under another list
    ln[wrong] = (ln[wrong] + 1 + rng.integers(0, nlist - 1, int(wrong.sum()))) % nlist
    ln[what == 7] = -1 - rng.integers(0, 5, int((what == 7).sum()))
    ln[what == 8] = nlist + rng.integers(0, 3, int((what == 8).sum()))
    rep = np.flatnonzero(what == 9)
    if rep.size:
        src = rng.integers(0, n_rm, rep.size)
        rm[rep], ln[rep] = rm[src], ln[src]
    _, _, m = check_remove(kind, off, ids, ln if mode == "pairs" else None, rm, oracle=oracle)
    assert m.removed > 0
    if n_rm >= 1023:
        assert m.missing > 0 and (mode == "any" or m.invalid > 0)


# ------------------------------------------------------------------------------------------------------------- list sizes
SEAM_SIZES = np.array([0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097, 4100, 70, 1, 0, 300], np.uint64)


@pytest.fixture(scope="module")
def seams():
    rng = np.random.default_rng(33)
    off = np.concatenate([[0], np.cumsum(SEAM_SIZES)]).astype(np.uint64)
    ids = spread(rng.choice(1 << 18, int(off[-1]), replace=False))  # distinct over the whole object: any-list mode removes one entry each
    for l in range(SEAM_SIZES.size):
        ids[int(off[l]):int(off[l + 1])].sort()
    ids[int(off[-1]) - 1] = 6 * (1 << 19) + 3  # the last list's largest id stands alone above 2^21: without it the precision drops
    return off, ids


def seam_positions(off, which):
    """positions (in the old object's decode_all order) a variant removes"""
    off = off.astype(np.int64)
    out = []
    for l in range(off.size - 1):
        n = int(off[l + 1] - off[l])
        if which == "edges":  # the first entry, the last, both neighbours of every 1024 seam
            p = {0, n - 1} | {s + d for s in range(1024, n + 1, 1024) for d in (-1, 0)}
        elif which == "all":
            p = set(range(n))
        elif which == "classes":  # 4100 -> 4090, 70 -> 60, 1 -> 0, and the last list loses its largest id
            p = {4100: set(range(5, 4100, 410)), 70: set(range(3, 70, 7)), 1: {0} if l == 12 else set(), 300: {"max"}}.get(n, set())
        else:
            p = set()
        out += [(l, q) for q in sorted(x for x in p if x == "max" or 0 <= x < n)]
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["edges", "all", "classes", "none"])
def test_list_sizes_on_the_chunk_and_class_seams(kind, mode, which, seams, oracle):
    off, ids = seams
    old = encode(kind, off, ids, True, BITS)
    if kind == "roc":
        check_roundtrips(oracle, off, ids)
    dec = old.decode_all().cpu().numpy().view(np.uint64)
    o = off.astype(np.int64)
    pairs = seam_positions(off, which)
    ln = np.array([l for l, _ in pairs], np.int64)
    rm = np.array([dec[o[l]:o[l + 1]].max() if q == "max" else dec[o[l] + q] for l, q in pairs], np.uint64)
    _, new, m = check_remove(kind, None, None, ln if mode == "pairs" else None, rm, old=old)
    assert m.missing == 0 and m.removed == len(pairs)
    if which == "all":
        assert new.ntotal == 0 and not new.offsets.any()
    if which == "none":
        same(img(kind, new, kind != "roc"), img(kind, old, kind != "roc"), f"{kind}: nothing removed")
    if which == "classes":
        sizes = (m.offsets[1:] - m.offsets[:-1]).astype(np.int64)
        assert sizes[10] == 4090 and sizes[11] == 60 and sizes[12] == 0 and sizes[14] == 299
        if kind == "roc":
            assert new.info()["precision"][14] < old.info()["precision"][14]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_one_list_no_list_and_lists_that_are_all_empty(kind, mode, oracle):
    pairs = mode == "pairs"
    # nlist == 1
    ids = spread(np.arange(1500))
    check_remove(kind, np.array([0, 1500], np.uint64), ids, np.zeros(3, np.int64) if pairs else None, ids[[0, 1024, 1499]], oracle=oracle)
    # every list empty: each valid pair is missing
    off0 = np.zeros(6, np.uint64)
    _, new, m = check_remove(kind, off0, np.zeros(0, np.uint64), np.array([0, 4, 5, -1]) if pairs else None, np.array([3, 9, 3, 3], np.uint64))
    assert (m.missing, m.invalid) == ((2, 1) if pairs else (4, 0)) and new.ntotal == 0
    # an empty batch
    _, new, m = check_remove(kind, off0, np.zeros(0, np.uint64), np.zeros(0, np.int64) if pairs else None, np.zeros(0, np.uint64))
    assert m.removed == 0


# ------------------------------------------------------------------------------------------------------------- membership
@pytest.mark.parametrize("kind", KINDS)
def test_the_same_id_in_two_lists(kind, oracle):
    off = np.array([0, 3, 3, 7], np.uint64)
    ids = np.array([9, 21, 33, 15, 21, 27, 39], np.uint64)
    _, _, m = check_remove(kind, off, ids, [2], [21], oracle=oracle)
    assert m.removed == 1 and m.mask[3:].sum() == 1
    _, _, m = check_remove(kind, off, ids, None, [21], oracle=oracle)
    assert m.removed == 2
    _, _, m = check_remove(kind, off, ids, [1, 0], [21, 15], oracle=oracle)  # an empty list, and an id of another list
    assert (m.removed, m.missing) == (0, 2)


def test_a_packed_list_with_a_repeated_id_loses_every_copy():
    off = np.array([0, 6, 9], np.uint64)
    ids = np.array([4, 8, 4, 1, 4, 2, 4, 8, 5], np.uint64)
    _, _, m = check_remove("packed", off, ids, [0], [4], bits=8)
    assert m.removed == 3 and np.array_equal(m.ids, [8, 1, 2, 4, 8, 5])
    _, _, m = check_remove("packed", off, ids, None, [4, 8], bits=8)
    assert m.removed == 6


@pytest.mark.parametrize("kind", ["packed", "ef"])
@pytest.mark.parametrize("mode", MODES)
def test_ids_above_32_bits_compare_on_all_64(kind, mode):
    """packed bits at width 40 and Elias-Fano over a 2^40 universe: a batch id that differs from a present one only in its high half,
    or only in its low half, does not match"""
    rng = np.random.default_rng(35)
    sizes = np.array([700, 0, 1500, 40], np.uint64)
    off, ids = sorted_lists(sizes, universe=1 << 40, seed=36)
    assert (ids >> 32).max() > 0
    pos = rng.choice(ids.size, 300, replace=False)
    hit = ids[pos[:100]]
    hi_only = ids[pos[100:200]] ^ np.uint64(1 << 35)   # the low half of a present id, another high half
    lo_only = ids[pos[200:]] ^ np.uint64(1 << 7)       # the high half of a present id, another low half
    miss = np.setdiff1d(np.concatenate([hi_only, lo_only]), ids)
    rm = np.concatenate([hit, miss])
    # (ids that share their low half sit next to each other after the first sort phase: a present id and its high-half twin)
    rm = np.concatenate([rm, ids[pos[100:110]]])
    ln = np.concatenate([lists_of(pos[:100], off), rng.integers(0, 4, miss.size), lists_of(pos[100:110], off)])
    order = rng.permutation(rm.size)
    _, _, m = check_remove(kind, off, ids, ln[order] if mode == "pairs" else None, rm[order], bits=40)
    assert m.removed == 110 and m.missing == miss.size


@pytest.mark.parametrize("mode", MODES)
def test_batch_ids_wider_than_the_object_count_as_missing(mode, oracle):
    off, ids = zipf(3000, 20, seed=37)
    ids = spread(ids)
    sel = ids[[5, 900, 2999]]
    wide = np.concatenate([sel + np.uint64(1 << 32), sel + np.uint64(1 << 20), [np.uint64(1 << 63)]]).astype(np.uint64)
    rm = np.concatenate([sel[:2], wide])
    ln = np.concatenate([lists_of(np.array([5, 900]), off), lists_of(np.array([5, 900, 2999, 5, 900, 2999, 5]), off)])
    ln_arg = ln if mode == "pairs" else None
    _, _, m = check_remove("packed", off, ids, ln_arg, rm, bits=20)
    assert (m.removed, m.missing) == (2, 7)
    _, _, m = check_remove("roc", off, ids, ln_arg, rm, oracle=oracle)
    assert (m.removed, m.missing) == (2, 7)


# ------------------------------------------------------------------------------------------------------------- ROC: touched lists only
def test_roc_works_only_on_touched_lists():
    from vector_db_id_compression_amd import synth
    from vector_db_id_compression_amd.codecs import RocLists

    ctx = _lib().default_context()
    w = synth.workload("s1")
    off, ids = w["offsets"], w["ids"]
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    assert sizes.max() > 50_000
    rng = np.random.default_rng(39)
    o = off.astype(np.int64)
    short = np.flatnonzero((sizes < 1000) & (sizes > 0))
    ln = rng.choice(short, 2000).astype(np.int64)
    old = RocLists.encode(off, dev(ids))
    dec = old.decode_all().cpu().numpy().view(np.uint64)
    rm = dec[o[ln] + (rng.random(2000) * sizes[ln]).astype(np.int64)]
    m = rr.remove(off, dec, ln, rm)
    d2h = ctx.d2h_bytes()
    new, mask = remove(old, ln, rm, want_perm=False)
    assert ctx.d2h_bytes() == d2h
    longest_touched = int(sizes[np.unique(ln)].max())
    for which in (0, 1):
        info = ctx.chain_info(which)
        assert info["longest"] <= longest_touched, (which, info, longest_touched)
    from test_gpu_dev_offsets import roc_image
    same(dict(offsets=new.offsets, **roc_image(new, False)),
         dict(offsets=m.offsets, **roc_image(RocLists.encode(m.offsets, dev(m.ids)), False)), "roc S1 remove")
    assert np.array_equal(mask.cpu().numpy(), m.mask)


# ------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_two_removes_equal_one_remove_of_the_union(kind, mode, zipf300, oracle):
    off, ids = zipf300
    rng = np.random.default_rng(41)
    pos = rng.choice(ids.size, 3000, replace=False)
    ln, rm = lists_of(pos, off), ids[pos]
    pick = (lambda a: a) if mode == "pairs" else (lambda a: None)
    old, mid, _ = check_remove(kind, off, ids, pick(ln[:1800]), rm[:1800], oracle=oracle)
    _, two, _ = check_remove(kind, None, None, pick(ln[1500:]), rm[1500:], old=mid)  # (the overlap is missing the second time)
    _, one, _ = check_remove(kind, None, None, pick(ln), rm, old=old)
    # (ROC's permutation is over the input of the last call: `two` saw the first batch's lists already in object order)
    same(img(kind, two, kind != "roc"), img(kind, one, kind != "roc"), f"{kind}: two removes against one")


@pytest.mark.parametrize("kind", KINDS)
def test_remove_then_append_gives_the_ids_back(kind, zipf300, oracle):
    off, ids = zipf300
    rng = np.random.default_rng(43)
    pos = rng.choice(ids.size, 700, replace=False)
    ln, rm = lists_of(pos, off), ids[pos]
    old, new, m = check_remove(kind, off, ids, ln, rm, oracle=oracle)
    back, lab = new.append(dev_i64(ln), dev(rm))
    assert back.ntotal == old.ntotal
    assert np.array_equal(back.translate_labels(lab).cpu().numpy().view(np.uint64), rm)
    a, b = old.decode_all().cpu().numpy(), back.decode_all().cpu().numpy()
    o = off.astype(np.int64)
    assert np.array_equal(back.offsets, old.offsets)
    for l in np.unique(ln):
        assert np.array_equal(np.sort(a[o[l]:o[l + 1]]), np.sort(b[o[l]:o[l + 1]]))


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "pool_poison"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_the_same_call_twice_gives_identical_objects(kind, mode, poison, zipf300, oracle):
    L = _lib()
    ctx = L.default_context()
    off, ids = zipf300
    rng = np.random.default_rng(45)
    pos = rng.choice(ids.size, 4000, replace=False)
    ln, rm = lists_of(pos, off), ids[pos]
    rm[::7] += 1
    ln_arg = ln if mode == "pairs" else None
    L.check(L.lib().vidc_ctx_debug_pool_poison(ctx.h, 1 if poison else 0))
    try:
        old, first, m = check_remove(kind, off, ids, ln_arg, rm, oracle=oracle)
        want = img(kind, first)
        mis = zeros1()
        second, mask = remove(old, ln_arg, rm, missing=mis)
        same(img(kind, second), want, f"{kind}: the second run differs")
        assert np.array_equal(mask.cpu().numpy(), m.mask) and int(mis.item()) == m.missing
        # either object may go first: the blocks of the one that went are handed out again (poisoned) by the next calls
        keep = second.decode_all().cpu().numpy().copy()
        del first, old
        junk = encode(kind, off, ids, True, BITS)
        assert np.array_equal(second.decode_all().cpu().numpy(), keep)
        del junk
        _torch().cuda.synchronize()
    finally:
        L.check(L.lib().vidc_ctx_debug_pool_poison(ctx.h, 0))


# ------------------------------------------------------------------------------------------------------------- status
def _raw_remove(kind, ctx_h, obj_h, n, ln, ids, out, prec=-1):
    L = _lib().lib()
    p = _lib().ptr
    if kind == "packed":
        return L.vidc_packed_remove_dev(ctx_h, obj_h, n, p(ln), p(ids), out, None, None, None)
    if kind == "ef":
        return L.vidc_ef_remove_dev(ctx_h, obj_h, n, p(ln), p(ids), 0, out, None, None, None)
    return L.vidc_roc_remove_dev(ctx_h, obj_h, n, p(ln), p(ids), prec, 0, out, None, None, None)


@pytest.mark.parametrize("kind", KINDS)
def test_invalid_arguments(kind, oracle):
    L = _lib()
    ctx = L.default_context()
    off, ids = zipf(2000, 50, seed=47)
    ids = spread(ids)
    obj = encode(kind, off, ids, True, BITS)
    ln, rm = dev_i64(np.arange(10) % 50), dev(ids[:10])
    for args in ((None, obj.h, 10, ln, rm), (ctx.h, None, 10, ln, rm), (ctx.h, obj.h, 10, ln, None), (ctx.h, obj.h, 10, None, None),
                 (ctx.h, obj.h, (1 << 32) - 1, ln, rm), (ctx.h, obj.h, 1 << 40, None, rm)):
        out = C.c_void_p(12345)
        assert _raw_remove(kind, *args, C.byref(out)) == -1, args
        assert out.value is None, "*out must be NULL after an error"
        assert b"remove" in L.lib().vidc_last_error()
    assert _raw_remove(kind, ctx.h, obj.h, 10, ln, rm, None) == -1
    if kind == "roc":
        for prec in (33, -3):
            out = C.c_void_p(12345)
            assert _raw_remove(kind, ctx.h, obj.h, 10, ln, rm, C.byref(out), prec=prec) == -1 and out.value is None
    # the context is still usable, the object untouched
    check_remove(kind, None, None, lists_of(np.arange(10), off), ids[:10], old=obj)


def _status(fn):
    try:
        fn()
    except _lib().VidcError as ex:
        return int(str(ex).split("vidc status ")[1].split(":")[0])
    return 0


def test_graph_objects_are_unsupported(oracle):
    torch = _torch()
    from vector_db_id_compression_amd.codecs import EfLists, RocLists

    rng = np.random.default_rng(49)
    rows = np.full((300, 8), -1, np.int32)
    for i in range(300):
        k = int(rng.integers(1, 9))
        rows[i, :k] = np.sort(rng.choice(300, k, replace=False))
    d_rows = torch.from_numpy(rows).cuda()
    for obj in (RocLists.encode_rows(d_rows), EfLists.encode_rows(d_rows)):
        before = obj.decode_rows(None, 8)[0].cpu().numpy()
        for ln in (np.array([1, 2]), None):
            assert _status(lambda: remove(obj, ln, np.array([int(rows[1, 0]), int(rows[2, 0])], np.uint64), removed=False)) == -6
        assert np.array_equal(obj.decode_rows(None, 8)[0].cpu().numpy(), before)  # untouched and still usable
    off, ids = zipf(2000, 50, seed=51)
    check_remove("roc", off, spread(ids), None, spread(ids)[:2], oracle=oracle)


# ------------------------------------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_stream_order(kind, mode, zipf300):
    """list numbers and ids made by torch kernels on the current stream right before the call, no synchronisation in between"""
    torch = _torch()
    off, ids = zipf300
    rng = np.random.default_rng(53)
    old = encode(kind, off, ids, True, BITS)
    pos = rng.choice(ids.size, 6000, replace=False)
    ln, rm = lists_of(pos, off), ids[pos]
    m = rr.remove(old.offsets, old.decode_all().cpu().numpy().view(np.uint64), ln if mode == "pairs" else None, rm)
    want = img(kind, encode(kind, m.offsets, m.ids, True, BITS))
    src_ln, src_rm = dev_i64(ln), dev(rm)
    torch.cuda.synchronize()
    big = torch.randn(4096, 4096, device="cuda")  # keep the stream busy in front of the batch
    for _ in range(4):
        big = big @ big
        big = big / big.norm()
    zero = (big[0, 0] * 0).to(torch.int64)
    d_ln, d_rm = src_ln + zero, src_rm + zero
    new, mask = _removal().remove(old, d_ln if mode == "pairs" else None, d_rm, want_perm=True)
    d_rm.fill_(-1)
    same(img(kind, new), want, f"{kind}: stream order")
    assert np.array_equal(mask.cpu().numpy(), m.mask)


# ------------------------------------------------------------------------------------------------------------- Python containers
def _index(xt, xb, centroids=None):
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(xt.shape[1], 24, "Flat")
    if centroids is None:
        idx.train(xt)
    else:
        idx.centroids = centroids
    idx.add(xb)
    idx.nprobe = 6
    idx.parallel_mode = 3
    return idx


@pytest.mark.parametrize("kind", ["packed-bits", "elias-fano", "roc", "none"])
def test_index_remove_ids(kind):
    """remove_ids of a few hundred ids, then the deferred search: the results are those of an index built from the surviving vectors
    alone (ids renumbered), up to ties; no removed id comes back; a later add hands out fresh ids"""
    from vector_db_id_compression_amd import custom_invlists as ci

    torch = _torch()
    rng = np.random.default_rng(55)
    d = 8
    xt = rng.standard_normal((900, d)).astype(np.float32)
    xb, xb2, xq = xt[:700], rng.standard_normal((60, d)).astype(np.float32), rng.standard_normal((40, d)).astype(np.float32)
    gone = rng.choice(700, 250, replace=False).astype(np.int64)
    a = _index(xt, xb)
    il_a, _ = ci.apply_id_compression(a, kind)
    ids_arg = torch.from_numpy(np.concatenate([gone, [5000, 700]])).cuda() if kind != "none" else np.concatenate([gone, [5000, 700]])
    assert a.remove_ids(ids_arg) == 250
    assert a.ntotal == 450 and (kind == "none" or il_a.ntotal == 450)
    keep = np.setdiff1d(np.arange(700), gone)
    b = _index(xt, xb[keep], a.centroids)  # ids 0 .. 449 stand for keep[0] .. keep[449]
    il_b, _ = ci.apply_id_compression(b, kind)
    if kind != "none":
        assert np.array_equal(il_a._offsets, il_b._offsets)
        assert np.array_equal(np.sort(il_a.get_ids_all().cpu().numpy()), keep)
        for name in ("codes_size_in_bytes", "overhead_in_bytes"):
            assert getattr(il_a, name, None) == getattr(il_b, name, None), name
    searches = (lambda i: i.search(xq, 10), lambda i: i.search_defer_id_decoding(xq, 10),
                lambda i: i.search_defer_id_decoding(xq, 10, decode_1by1=True))
    for search in searches:
        Da, Ia = search(a)
        Db, Ib = search(b)
        assert np.array_equal(Da, Db)
        assert not np.isin(Ia, gone).any()
        Ib = np.where(Ib >= 0, keep[np.maximum(Ib, 0)], -1)
        for q in range(xq.shape[0]):  # equal-distance ties may come back in another order: compare (distance, id) pairs as sets
            assert sorted(zip(Da[q].tolist(), Ia[q].tolist())) == sorted(zip(Db[q].tolist(), Ib[q].tolist())), (kind, q)
    a.add(xb2)  # fresh ids: 700 .. 759, never one that was handed out before
    assert a.ntotal == 510
    all_ids = (il_a.get_ids_all().cpu().numpy() if kind != "none" else np.concatenate([a.invlists.get_ids(l) for l in range(24)]))
    assert np.array_equal(np.sort(all_ids), np.concatenate([keep, np.arange(700, 760)]))
    D, I = a.search_defer_id_decoding(xb2[:20], 1)
    assert np.array_equal(I[:, 0], np.arange(700, 720)) and not np.isin(I, gone).any()
    if kind != "none":
        with pytest.raises(RuntimeError, match="read-only"):
            il_a.add_entries(0, 1, None, None)


def test_wavelet_tree_container_refuses():
    from vector_db_id_compression_amd import custom_invlists as ci

    rng = np.random.default_rng(57)
    xt = rng.standard_normal((300, 8)).astype(np.float32)
    a = _index(xt, xt[:200])
    il, _ = ci.apply_id_compression(a, "wavelet-tree")
    with pytest.raises(RuntimeError, match="permutation"):
        a.remove_ids(np.array([1, 2], np.int64))
    assert a.ntotal == 200 and il.ntotal == 200
