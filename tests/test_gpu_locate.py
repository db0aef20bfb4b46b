"""Locate (list, id) batches in compressed lists on the device (vidc_*_locate_dev): labels, missing and invalid are those of the numpy
model (tests/locate_ref.py) run on the object's own decode_all; translate_labels maps every label >= 0 back to its id; the object's
image does not change; nothing moves id payload over PCIe; the labels are written into guarded, poisoned buffers.  Every comparison
is exact.  ROC inputs are the 6 k + 3 ids of test_gpu_remove.py (lists the reference codec round-trips)."""
import numpy as np
import pytest

import contract_ref as cr
import locate_ref
from test_gpu_append import append, dev_i64, encode, image
from test_gpu_dev_offsets import dev, same, zipf
from test_gpu_remove import lists_of, spread, zeros1

pytestmark = pytest.mark.gpu

KINDS = ["packed", "ef", "roc"]
MODES = ["pairs", "any"]
BITS = 24  # packed width of the ordinary cases: ids below 2^24
VIDC_ERR_UNSUPPORTED = -6


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _locate():
    from vector_db_id_compression_amd import locate

    return locate


def id_bits_of(kind, obj):
    """the width of the ids the object can hold (a wavelet tree holds 0 .. ntotal - 1: a larger id is simply not in it)"""
    return {"packed": lambda: obj.bits, "roc": lambda: 32}.get(kind, lambda: 64)()


def csr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def check_locate(kind, obj, ln, ids, want_perm=True, misalign=0):
    """locate on `obj`; compare with the model on obj.decode_all(), the defining property, the counters, the guards, the object's
    image and the d2h counter -> (labels, missing, invalid) of the model"""
    torch = _torch()
    ctx = _lib().default_context()
    ln = None if ln is None else np.asarray(ln, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.uint64)
    dec = obj.decode_all().cpu().numpy().view(np.uint64)
    labels, missing, invalid = locate_ref.locate(obj.offsets, dec, ln, ids, id_bits_of(kind, obj))
    before = image(kind, obj, want_perm)
    d_ln = None if ln is None else dev_i64(ln)
    d_ids = dev(ids) if ids.size else torch.zeros(0, dtype=torch.int64, device="cuda")
    mis, inv = zeros1(), zeros1()
    d2h = ctx.d2h_bytes()
    if ids.size:
        whole, view = cr.guarded(ids.size, np.int64, device="cuda", misalign_elems=misalign)
        out = _locate().locate(obj, d_ln, d_ids, out=view, missing=mis, invalid=inv)
        torch.cuda.synchronize()
        assert out is view
        cr.assert_guards_intact(whole, view, f"{kind} locate")
        cr.assert_view_equals(view, labels, f"{kind} locate")
    else:  # (an empty view has no address of its own to guard)
        assert _locate().locate(obj, d_ln, d_ids, missing=mis, invalid=inv).numel() == 0
    assert ctx.d2h_bytes() == d2h, f"{kind}: a locate moved id payload to the host"
    assert (int(mis.item()), int(inv.item())) == (missing, invalid), f"{kind}: (missing, invalid)"
    hit = labels >= 0
    if hit.any():
        back = obj.translate_labels(dev_i64(labels[hit])).cpu().numpy().view(np.uint64)
        assert np.array_equal(back, ids[hit]), f"{kind}: translate_labels does not map the labels back to the ids"
    same(image(kind, obj, want_perm), before, f"{kind}: the object changed")
    return labels, missing, invalid


# ------------------------------------------------------------------------------------------------------------- the batch
@pytest.fixture(scope="module")
def zipf300():
    """300 lists (the list key takes two radix passes), 30 000 ids; one object per kind, shared and never changed"""
    off, ids = zipf(30_000, 300, seed=31)
    ids = spread(ids)
    return off, ids, {k: encode(k, off, ids, True, BITS) for k in KINDS}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 64, 65, 1023, 1024, 1025, 5000])
def test_batch_sizes_on_the_sorter_rounds_and_tiles(kind, mode, n, zipf300):
    """half the pairs hit; the rest name an absent id or a present id under the wrong list, a negative or too large list number, or
    repeat an earlier pair"""
    off, ids, objs = zipf300
    rng = np.random.default_rng(300 + n)
    nlist = off.size - 1
    pos = rng.choice(ids.size, n, replace=False)
    want, ln = ids[pos].copy(), lists_of(pos, off)
    what = rng.integers(0, 10, n) if n > 1 else np.zeros(1, np.int64)  # 0-4 hit
    want[what == 5] += 1                                                # an id no list holds (6 k + 4)
    wrong = what == 6                                                   # a present id under another list
    ln[wrong] = (ln[wrong] + 1 + rng.integers(0, nlist - 1, int(wrong.sum()))) % nlist
    ln[what == 7] = -1 - rng.integers(0, 5, int((what == 7).sum()))
    ln[what == 8] = nlist + rng.integers(0, 3, int((what == 8).sum()))
    rep = np.flatnonzero(what == 9)
    if rep.size:
        src = rng.integers(0, n, rep.size)
        want[rep], ln[rep] = want[src], ln[src]
    labels, missing, invalid = check_locate(kind, objs[kind], ln if mode == "pairs" else None, want, misalign=n % 2)
    assert (labels[what < 5] >= 0).all()
    if n >= 1023:
        assert missing > 0 and (mode == "any" or invalid > 0)


# ------------------------------------------------------------------------------------------------------------- list sizes
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_every_position_of_lists_on_the_1024_element_chunk(kind, mode):
    sizes = [0, 1, 1023, 1024, 1025, 2049, 0]
    off = csr(sizes)
    rng = np.random.default_rng(41)
    ids = spread(rng.choice(1 << 18, int(off[-1]), replace=False))  # distinct over the whole object: one label per id in any-list mode
    for l in range(len(sizes)):
        ids[int(off[l]):int(off[l + 1])].sort()
    obj = encode(kind, off, ids, True, BITS)
    dec = obj.decode_all().cpu().numpy().view(np.uint64)
    order = rng.permutation(dec.size)
    labels, missing, invalid = check_locate(kind, obj, lists_of(order, off) if mode == "pairs" else None, dec[order])
    o = off.astype(np.int64)
    assert np.array_equal(o[labels >> 32] + (labels & 0xFFFFFFFF), order) and (missing, invalid) == (0, 0)


# ------------------------------------------------------------------------------------------------------------- duplicates
@pytest.mark.parametrize("kind", ["packed", "ef"])
def test_duplicates_take_the_smallest_label(kind):
    """equal ids at offsets 1023 and 1024 of list 0 (two wavefronts, one atomic minimum); equal ids in lists 0 and 2"""
    sizes = [2049, 5, 1500]
    off = csr(sizes)
    ids = np.concatenate([3 * np.arange(s, dtype=np.uint64) + 7 for s in sizes])  # ascending; lists 0 and 2 share their first 1500 ids
    ids[1024] = ids[1023]
    ids[int(off[1]):int(off[2])] = 3 * np.arange(5, dtype=np.uint64) + 8  # list 1 shares nothing
    obj = encode(kind, off, ids, True, BITS)
    for _ in range(3):  # (the same on every run)
        labels, _, _ = check_locate(kind, obj, None, ids)
        assert labels[1023] == 1023 and labels[1024] == 1023
        # list 0 wins over list 2 -- but for the id that list 0 lost to the duplicate
        assert np.array_equal(labels[int(off[2]):], np.where(np.arange(1500) == 1024, (2 << 32) | 1024, np.arange(1500)))
    labels, missing, _ = check_locate(kind, obj, np.full(ids.size, 2, np.int64), ids)
    assert (labels[int(off[2]):] >> 32 == 2).all() and missing == int((labels < 0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------- wide ids
@pytest.mark.parametrize("kind", ["packed", "ef"])
@pytest.mark.parametrize("mode", MODES)
def test_ids_above_2_to_32_and_ids_too_wide_for_the_object(kind, mode):
    rng = np.random.default_rng(43)
    sizes = [70, 0, 1300, 3]
    off = csr(sizes)
    top = 40 if kind == "packed" else 45
    ids = np.unique(rng.integers(0, 1 << top, 3 * int(off[-1]), dtype=np.uint64))[: int(off[-1])]
    ids = ids[rng.permutation(ids.size)]
    low = ids & np.uint64(0xFFFFFFFF)
    ids[5], ids[100] = low[6] | np.uint64(1 << 33), low[101] | np.uint64(1 << 35)  # equal low halves: the high-half pass decides
    for l in range(len(sizes)):
        ids[int(off[l]):int(off[l + 1])].sort()
    obj = encode(kind, off, ids, True, 40)
    pos = rng.permutation(ids.size)[:900]
    dec = obj.decode_all().cpu().numpy().view(np.uint64)
    want = np.concatenate([dec[pos], dec[pos[:50]] ^ np.uint64(1 << 34), np.array([1 << 40, (1 << 63) + 5, 2 ** 64 - 1], np.uint64)])
    ln = np.concatenate([lists_of(pos, off), lists_of(pos[:50], off), [0, 2, 3]])
    labels, missing, _ = check_locate(kind, obj, ln if mode == "pairs" else None, want)
    assert (labels[:900] >= 0).all() and (labels[-3:] == -1).all() and missing >= 3


# ------------------------------------------------------------------------------------------------------------- ROC
ROC_SIZES = [1, 17, 0, 64, 65, 300, 5000, 0]  # lane, row and chain classes among the candidates; empty lists


@pytest.fixture(scope="module")
def roc_classes():
    off = csr(ROC_SIZES)
    rng = np.random.default_rng(47)
    ids = spread(rng.choice(1 << 20, int(off[-1]), replace=False))
    for l in range(len(ROC_SIZES)):
        ids[int(off[l]):int(off[l + 1])].sort()
    return off, ids


@pytest.mark.parametrize("hook", [None, "VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
@pytest.mark.parametrize("mode", ["pairs", "any", "one-list"])
def test_roc_labels_follow_sampling_order_in_every_decoder_class(hook, mode, roc_classes, monkeypatch):
    off, ids = roc_classes
    for h in ("VIDC_FORCE_GENERAL", "VIDC_NO_LANE"):
        monkeypatch.delenv(h, raising=False)
    if hook:
        monkeypatch.setenv(hook, "1")
    obj = encode("roc", off, ids, True)
    rng = np.random.default_rng(48)
    if mode == "one-list":  # a batch that names list 5 only: one candidate
        pos = int(off[5]) + rng.permutation(300)[:200]
    else:
        pos = np.concatenate([rng.permutation(ids.size)[:2000], np.arange(int(off[5]))])  # every id of the short lists among them
    want = np.concatenate([ids[pos], ids[pos[:40]] + 1])
    ln = np.concatenate([lists_of(pos, off), lists_of(pos[:40], off)])
    labels, missing, invalid = check_locate("roc", obj, None if mode == "any" else ln, want)
    assert (labels[: pos.size] >= 0).all() and (missing, invalid) == (40, 0)


# ------------------------------------------------------------------------------------------------------------- wavelet tree
def wt_lists(nlist, ntotal, seed):
    """a permutation of 0 .. ntotal - 1, ascending inside every list; list 1 of three or more lists is empty"""
    rng = np.random.default_rng(seed)
    lst = rng.integers(0, nlist, ntotal)
    if nlist >= 3:
        lst[lst == 1] = nlist - 1
    order = np.argsort(lst, kind="stable").astype(np.uint64)
    return csr(np.bincount(lst, minlength=nlist)), order, lst


@pytest.mark.parametrize("kind", ["wt", "wt1"])
@pytest.mark.parametrize("ntotal", [1, 63, 64, 65, 511, 512, 513, 2017])
def test_wavelet_tree_walks_every_id_down(kind, ntotal):
    """the 63-bit RRR block, the 512-bit rank block, one id beyond a 32-block sample; 1 .. 9 levels"""
    for nlist in (1, 2, 3, 5, 256, 257):
        off, ids, lst = wt_lists(nlist, ntotal, 100 * nlist + ntotal)
        obj = encode(kind, off, ids)
        every = np.concatenate([np.arange(ntotal, dtype=np.uint64), np.array([ntotal, 1 << 40], np.uint64)])
        labels, missing, invalid = check_locate(kind, obj, None, every)
        assert (labels[:ntotal] >> 32 == lst).all() and (labels[ntotal:] == -1).all() and (missing, invalid) == (2, 0)
        right = np.concatenate([lst, [0, 0]]).astype(np.int64)
        labels2, missing, invalid = check_locate(kind, obj, right, every)
        assert np.array_equal(labels2, labels) and (missing, invalid) == (2, 0)
        wrong = np.concatenate([(lst + 1) % nlist, [-1, nlist]]).astype(np.int64)
        labels3, missing, invalid = check_locate(kind, obj, wrong, every)
        if nlist > 1:
            assert (labels3 == -1).all() and (missing, invalid) == (ntotal, 1)


# ------------------------------------------------------------------------------------------------------------- edges
@pytest.fixture(scope="module")
def small():
    sizes = [0, 40, 513, 0, 70]
    off = csr(sizes)
    ids = np.arange(int(off[-1]), dtype=np.uint64)  # a permutation, ascending per list: every codec takes it
    return off, ids


@pytest.mark.parametrize("kind", KINDS + ["wt", "wt1"])
def test_empty_batch_and_a_batch_without_a_valid_pair(kind, small):
    off, ids = small
    obj = encode(kind, off, ids if kind.startswith("wt") else spread(ids), True, BITS)
    for ln in (None, np.zeros(0, np.int64)):
        check_locate(kind, obj, ln, np.zeros(0, np.uint64))
    fn = getattr(_lib().lib(), f"vidc_{kind[:2] if kind.startswith('wt') else kind}_locate_dev")
    assert fn(obj.ctx.h, obj.h, 0, None, None, None, None, None) == 0  # n == 0: VIDC_OK whatever the arrays are
    labels, missing, invalid = check_locate(kind, obj, np.array([-1, 5, -3, 99], np.int64), np.array([3, 9, 15, 21], np.uint64))
    assert (labels == -1).all() and (missing, invalid) == (0, 2)
    if kind.startswith("wt"):  # (a wavelet tree over no ids is not built)
        return
    empty = encode(kind, csr([0, 0, 0]), np.zeros(0, np.uint64), True, BITS)
    for ln in (None, np.array([0, 2, 3], np.int64)):
        _, missing, invalid = check_locate(kind, empty, ln, np.array([0, 1, 2], np.uint64))
        assert (missing, invalid) == ((3, 0) if ln is None else (2, 1))


@pytest.mark.parametrize("kind", KINDS + ["wt"])
def test_objects_built_by_append_remove_and_load(kind, small, tmp_path):
    from vector_db_id_compression_amd import persist, removal

    off, ids = small
    wt = kind.startswith("wt")
    base = ids if wt else spread(ids)
    obj = encode(kind, off, base, True, BITS)
    add_ln = np.array([4, 0, 2, 2, -1, 0], np.int64)
    add = (ids.size + np.cumsum(add_ln >= 0) - 1).astype(np.uint64)  # fresh ids, ascending in add order
    grown, _ = append(kind, obj, dev_i64(add_ln), dev(add if wt else spread(add)), True, BITS)
    dec = grown.decode_all().cpu().numpy().view(np.uint64)
    labels, missing, _ = check_locate(kind, grown, None, np.concatenate([dec, [6 * 4000 + 4]]))
    assert (labels[:-1] >= 0).all() and missing == 1
    if not wt:
        shrunk, _ = removal.remove(grown, None, dev(dec[::3]), want_perm=True)
        labels, missing, _ = check_locate(kind, shrunk, None, dec)
        assert np.array_equal(labels >= 0, np.arange(dec.size) % 3 != 0) and missing == len(dec[::3])
    loaded = persist.load(persist.save(grown, str(tmp_path / "obj")))
    check_locate(kind, loaded, lists_of(np.arange(dec.size), grown.offsets), dec, want_perm=False)


def test_graph_objects_are_unsupported():
    from vector_db_id_compression_amd import VidcError, codecs

    torch = _torch()
    L = _lib()
    rows = np.full((5, 8), -1, np.int32)
    rows[:, :3] = np.arange(15).reshape(5, 3)
    d_ids, d_out = dev(np.array([1, 2], np.uint64)), torch.full((2,), 7, dtype=torch.int64, device="cuda")
    for obj, fn in ((codecs.EfLists.encode_rows(rows), L.lib().vidc_ef_locate_dev), (codecs.RocLists.encode_rows(rows), L.lib().vidc_roc_locate_dev)):
        assert fn(obj.ctx.h, obj.h, 2, None, L.ptr(d_ids), L.ptr(d_out), None, None) == VIDC_ERR_UNSUPPORTED
        assert b"graph" in L.lib().vidc_last_error() and d_out.tolist() == [7, 7]
        with pytest.raises(VidcError, match=type(obj).__name__):
            _locate().locate(obj, None, d_ids)
    ok = encode("ef", csr([2]), np.array([1, 2], np.uint64))  # the context stays usable
    assert _locate().locate(ok, None, d_ids).tolist() == [0, 1]


# ------------------------------------------------------------------------------------------------------------- containers
CONTAINERS = ["packed-bits", "elias-fano", "roc", "wavelet-tree", "wavelet-tree-1"]


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(53)
    return rng.standard_normal((2300, 8)).astype(np.float32)


def _index(xb):
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(xb.shape[1], 16, "Flat")
    idx.train(xb)
    idx.add(xb)
    return idx


@pytest.mark.parametrize("name", CONTAINERS)
def test_container_locate_batch_and_reconstruct_batch(name, vectors):
    from vector_db_id_compression_amd import custom_invlists as ci

    torch = _torch()
    xb, more = vectors[:2000], vectors[2000:]
    idx = _index(xb)
    il, _ = ci.apply_id_compression(idx, name)
    every = torch.arange(2000, dtype=torch.int64, device="cuda")
    labels = il.locate_batch(None, every)
    assert (labels >= 0).all() and torch.equal(il.translate_labels(labels), every)
    lists = labels >> 32
    assert torch.equal(il.locate_batch(lists, every), labels)
    assert (il.locate_batch((lists + 1) % 16, every) == -1).all()
    assert np.array_equal(idx.reconstruct_batch(every).cpu().numpy(), xb)
    assert np.array_equal(idx.reconstruct_batch(np.array([1999, 0, 7, 7], np.int64)).cpu().numpy(), xb[[1999, 0, 7, 7]])
    with pytest.raises(RuntimeError, match="not in the index"):
        idx.reconstruct_batch(np.array([5, 2000], np.int64))
    idx.add(more)  # ids 2000 .. 2299
    stored = vectors.copy()
    alive = np.arange(2300)
    if not name.startswith("wavelet"):
        gone = np.arange(3, 2300, 7)
        assert idx.remove_ids(torch.from_numpy(gone).cuda()) == gone.size
        alive = np.setdiff1d(alive, gone)
        with pytest.raises(RuntimeError, match="not in the index"):
            idx.reconstruct_batch(gone[:2])
    assert np.array_equal(idx.reconstruct_batch(alive).cpu().numpy(), stored[alive])


def test_reconstruct_batch_on_uncompressed_lists(vectors):
    idx = _index(vectors[:500])
    assert np.array_equal(idx.reconstruct_batch(np.arange(499, -1, -1)).cpu().numpy(), vectors[:500][::-1])
    with pytest.raises(RuntimeError, match="not in the index"):
        idx.reconstruct_batch(np.array([500], np.int64))
