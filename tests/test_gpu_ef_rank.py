"""Rank inside compressed Elias-Fano lists and graph rows on the device (vidc_ef_rank_dev).  Every call's ranks, found flags and invalid
count are those of the numpy statement (tests/ef_rank_ref.py: np.searchsorted on the object's own decoded lists); both outputs are
written into guarded, poisoned buffers; the d2h counter does not move; the object's exported image is the same word for word before
and after.  For list objects, wherever found, list << 32 | rank is the label vidc_ef_locate_dev answers in pairs mode and
translate_labels maps it back to the id; where not found, locate says -1.  Every comparison is exact.  The queries are the ones the
contract allows, against objects the encoder built."""
import ctypes as C

import numpy as np
import pytest

import contract_ref as cr
import ef_rank_ref as er
import lists_ref as lr

pytestmark = pytest.mark.gpu

POISON8 = 0xA5
GUARD8 = 256
M64 = er.M64


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def _rank():
    from vector_db_id_compression_amd import rank

    return rank


def sync():
    _torch().cuda.synchronize()


def dev_u64(a):
    t = _torch()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return t.from_numpy(a.view(np.int64)).cuda() if a.size else t.zeros(0, dtype=t.int64, device="cuda")


def dev_i64(a):
    t = _torch()
    a = np.ascontiguousarray(a, dtype=np.int64)
    return t.from_numpy(a).cuda() if a.size else t.zeros(0, dtype=t.int64, device="cuda")


def zeros1():
    return _torch().zeros(1, dtype=_torch().int64, device="cuda")


def encode(lists, ctx=None, dev_offsets=False):
    off = lr.offsets_of(lists)
    ids = lr.concat(lists)
    sync()
    return _codecs().EfLists.encode(dev_u64(off) if dev_offsets else off, dev_u64(ids), ctx=ctx)


def ef_words(obj):
    """the exported image (vidc_ef_export_all) with the per-list geometry"""
    L = _lib()
    lw, hw = C.c_uint64(), C.c_uint64()
    L.check(L.lib().vidc_ef_stream_words(obj.h, C.byref(lw), C.byref(hw)))
    low, high = np.zeros(max(lw.value, 1), np.uint64), np.zeros(max(hw.value, 1), np.uint64)
    L.check(L.lib().vidc_ef_export_all(obj.ctx.h, obj.h, L.ptr(low), low.size, L.ptr(high), high.size))
    return dict(low=low, high=high, **obj.info())


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs"


def lists_of_obj(obj):
    """the object's own lists (decode_lists of every list) as uint64 arrays"""
    nlist = obj.offsets.size - 1
    if nlist == 0:
        return []
    dec, off = obj.decode_lists(np.arange(nlist, dtype=np.uint64))
    sync()
    dec = dec.cpu().numpy().view(np.uint64)
    off = np.asarray(off).astype(np.int64)
    return [dec[off[l]:off[l + 1]].copy() for l in range(nlist)]


def guarded_u8(n):
    t = _torch()
    whole = t.full((n + 2 * GUARD8,), POISON8, dtype=t.uint8, device="cuda")
    return whole, whole[GUARD8:GUARD8 + n]


def call_rank(obj, ln, ids, what, want_found=True):
    """the call through rank.rank into guarded buffers -> (ranks, found, invalid) as numpy; the guards and the d2h counter are checked"""
    torch = _torch()
    ln = np.asarray(ln, dtype=np.int64)
    ids = lr.u64(ids)
    n = ids.size
    d_ln, d_ids, inv = dev_i64(ln), dev_u64(ids), zeros1()
    d2h = obj.ctx.d2h_bytes()
    if n == 0:
        out = _rank().rank(obj, d_ln, d_ids, invalid=inv)
        sync()
        assert out.numel() == 0 and int(inv.item()) == 0 and obj.ctx.d2h_bytes() == d2h
        return np.zeros(0, np.int64), (np.zeros(0, np.uint8) if want_found else None), 0
    whole, view = cr.guarded(n, np.int64, device="cuda", misalign_elems=n % 2)
    fwhole, fview = guarded_u8(n) if want_found else (None, None)
    sync()
    out = _rank().rank(obj, d_ln, d_ids, out=view, found=fview, invalid=inv)
    sync()
    assert out is view
    assert obj.ctx.d2h_bytes() == d2h, f"{what}: a rank moved id payload to the host"
    cr.assert_guards_intact(whole, view, f"{what}: ranks")
    assert np.array_equal(d_ln.cpu().numpy(), ln) and np.array_equal(d_ids.cpu().numpy().view(np.uint64), ids), f"{what}: the inputs changed"
    found = None
    if want_found:
        fw = fwhole.cpu().numpy()
        assert (fw[:GUARD8] == POISON8).all() and (fw[GUARD8 + n:] == POISON8).all(), f"{what}: found guards"
        found = fw[GUARD8:GUARD8 + n].copy()
    return view.cpu().numpy().copy(), found, int(inv.item())


def check_rank(obj, lists, ln, ids, what, locate=True, image=True):
    """call_rank against the statement; for list objects the labels against vidc_ef_locate_dev and translate_labels; the image"""
    ln = np.asarray(ln, dtype=np.int64)
    ids = lr.u64(ids)
    before = ef_words(obj) if image else None
    want_r, want_f, want_inv = er.statement(lists, ln, ids)
    ranks, found, inv = call_rank(obj, ln, ids, what)
    bad = np.flatnonzero(ranks != want_r)
    assert bad.size == 0, f"{what}: {bad.size} ranks differ, first pair {int(bad[0])}: list {ln[bad[0]]} id {ids[bad[0]]} got {ranks[bad[0]]} want {want_r[bad[0]]}"
    bad = np.flatnonzero(found != want_f)
    assert bad.size == 0, f"{what}: {bad.size} found flags differ, first pair {int(bad[0])}: list {ln[bad[0]]} id {ids[bad[0]]}"
    assert inv == want_inv, f"{what}: invalid {inv}, the statement says {want_inv}"
    only_r, none, _ = call_rank(obj, ln, ids, what + " (no found array)", want_found=False)
    assert none is None and np.array_equal(only_r, want_r)
    if locate and ids.size:
        from vector_db_id_compression_amd import locate as loc

        labels = loc.locate(obj, dev_i64(ln), dev_u64(ids))
        sync()
        labels = labels.cpu().numpy()
        want_lab = np.where(want_f == 1, (np.maximum(ln, 0) << 32) | np.maximum(want_r, 0), -1)
        assert np.array_equal(labels, want_lab), f"{what}: list << 32 | rank is not locate's label"
        hit = want_f == 1
        if hit.any():
            back = obj.translate_labels(dev_i64(want_lab[hit]))
            sync()
            assert np.array_equal(back.cpu().numpy().view(np.uint64), ids[hit]), f"{what}: translate_labels does not lead back to the id"
        succ = (want_r >= 0) & (want_f == 0)  # the successor: the first entry >= the id, where there is one
        sizes = np.array([len(li) for li in lists], np.int64)
        succ[succ] = want_r[succ] < sizes[ln[succ]]
        if succ.any():
            nxt = obj.translate_labels(dev_i64((ln[succ] << 32) | want_r[succ]))
            sync()
            assert (nxt.cpu().numpy().view(np.uint64) > ids[succ]).all(), f"{what}: the label of a rank is not the successor"
    if image:
        same(ef_words(obj), before, f"{what}: the object changed")
    return want_r, want_f, want_inv


# ----------------------------------------------------------------------------------------------------------------- the designed object
_DESIGNED = {}


def designed_object():
    """-> (lists, pairs): the designed lists of tests/ef_rank_ref.py between empty lists, and every query of every list (the empty lists
    are asked the extremes).  Built once, never changed."""
    if not _DESIGNED:
        d = er.designed()
        er.check_designed(d)
        lists = [np.zeros(0, np.uint64)]
        for i, k in enumerate(sorted(d)):
            lists.append(d[k])
            if i % 5 == 4:
                lists.append(np.zeros(0, np.uint64))
        lists.append(np.zeros(0, np.uint64))
        ln, ids = [], []
        for l, li in enumerate(lists):
            q = er.queries(li)
            ln.append(np.full(q.size, l, np.int64))
            ids.append(q)
        _DESIGNED.update(lists=lists, ln=np.concatenate(ln), ids=np.concatenate(ids))
    return _DESIGNED["lists"], _DESIGNED["ln"], _DESIGNED["ids"]


@pytest.mark.parametrize("dev_offsets", [False, True])
def test_designed_lists_every_query(dev_offsets):
    """sizes 0 .. 65, l = 0 and l = 29, ids above 2^32, buckets and duplicate runs across batch boundaries, zeros on word and batch
    boundaries, two random lists: every entry, every entry +- 1, 0, u, u + 1, 2^32, 2^63, 2^64 - 1 -- in list order and shuffled"""
    lists, ln, ids = designed_object()
    obj = encode(lists, dev_offsets=dev_offsets)
    assert [np.array_equal(a, b) for a, b in zip(lists_of_obj(obj), lists)].count(False) == 0
    check_rank(obj, lists, ln, ids, "designed")
    p = np.random.default_rng(1).permutation(ln.size)
    check_rank(obj, lists, ln[p], ids[p], "designed, shuffled", image=False)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257])
def test_batch_forms(n):
    """batch sizes around the four-pairs-per-wavefront grouping; negative and too large list numbers and repeated pairs mixed in"""
    lists, ln, ids = designed_object()
    obj = encode(lists)
    rng = np.random.default_rng(100 + n)
    pick = rng.choice(ln.size, n, replace=False)
    bl, bi = ln[pick].copy(), ids[pick].copy()
    if n >= 5:
        what = rng.integers(0, 8, n)
        what[:5] = [0, 5, 6, 7, 0]
        bl[what == 5] = -1 - rng.integers(0, 5, int((what == 5).sum()))
        bl[what == 6] = len(lists) + rng.integers(0, 3, int((what == 6).sum()))
        rep = np.flatnonzero(what == 7)
        src = rng.integers(0, n, rep.size)
        bl[rep], bi[rep] = bl[src], bi[src]
    r, f, inv = check_rank(obj, lists, bl, bi, f"batch of {n}", image=n in (0, 257))
    if n >= 5:
        assert (r == -1).sum() >= 2 and inv >= 1
    L = _lib()
    assert L.lib().vidc_ef_rank_dev(obj.ctx.h, obj.h, 0, None, None, None, None, None) == 0  # n == 0: VIDC_OK whatever the arrays are


def test_all_pairs_skipped_or_invalid_and_an_object_without_ids():
    lists, _, _ = designed_object()
    obj = encode(lists)
    r, f, inv = check_rank(obj, lists, [-1, len(lists), -3, len(lists) + 9], [3, 9, 15, 21], "no valid pair")
    assert (r == -1).all() and (f == 0).all() and inv == 2
    empty = [np.zeros(0, np.uint64)] * 3
    r, f, inv = check_rank(encode(empty), empty, [0, 2, 3, 1, -1], [0, 1, 2, M64, 5], "empty object", image=False)
    assert r.tolist() == [0, 0, -1, 0, -1] and inv == 1


# ------------------------------------------------------------------------------------------------------------------------- grid-stride
@pytest.fixture(scope="module")
def small():
    """a context created under VIDC_NUM_CU=1, pool poison on, running on torch's stream (the idiom of tests/test_gpu_small_grid.py)"""
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
    sync()
    ctx.synchronize()
    ctx.close()


#: pairs one trip of the grid-stride loops covers at one CU (requests.h req_grid: 32 workgroups; k_ef_rank_g16 takes 16 pairs per
#: workgroup of 256 threads, k_ef_rank_arena 256)
TRIP_G16, TRIP_ARENA = 32 * 16, 32 * 256


def test_nine_thousand_lists_named_once_each(small):
    rng = np.random.default_rng(9000)
    sizes = rng.integers(0, 12, 9000)
    sizes[::97] = 0
    lists = [np.sort(rng.integers(0, 1 << 20, int(n), dtype=np.uint64)) for n in sizes]
    ln = rng.permutation(9000).astype(np.int64)
    ids = np.array([int(li[rng.integers(0, li.size)]) + int(rng.integers(0, 2)) if li.size else 7 for li in (lists[l] for l in ln)], np.uint64)
    assert ln.size > 3 * TRIP_G16 and ln.size % TRIP_G16
    want = check_rank(encode(lists), lists, ln, ids, "9000 lists")
    got = check_rank(encode(lists, ctx=small), lists, ln, ids, "9000 lists, one CU")
    assert all(np.array_equal(a, b) for a, b in zip(want[:2], got[:2])) and want[2] == got[2]


def test_designed_object_on_one_cu_equals_the_default_context(small):
    lists, ln, ids = designed_object()
    assert ln.size > 3 * TRIP_G16
    n = 2 * TRIP_G16 + 301  # three trips, the last one ragged (and ending inside a wavefront: 301 = 4 * 75 + 1)
    p = np.random.default_rng(2).permutation(ln.size)
    default, one = encode(lists), encode(lists, ctx=small)
    same(ef_words(one), ef_words(default), "one CU against the default context")
    for tag, sel in (("every query", p), ("three trips", p[:n])):
        a = call_rank(default, ln[sel], ids[sel], tag)
        b = check_rank(one, lists, ln[sel], ids[sel], f"one CU, {tag}")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], tag


# -------------------------------------------------------------------------------------------------------------------------- graph rows
def graph_rows(N, K, seed):
    """int32 [N, K], -1 padded, ids below N in random order: empty rows, full rows (K ids, or all N where N < K), a one-edge row"""
    rng = np.random.default_rng([seed, N, K])
    rows = np.full((N, K), -1, np.int32)
    deg = rng.integers(0, min(K, N) + 1, N)
    deg[:6] = [0, min(K, N), 1, 0, min(K, N), 1]
    for i in range(N):
        rows[i, : deg[i]] = rng.choice(N, int(deg[i]), replace=False)
    rows[2, 0] = N - 1
    rows[5, 0] = 0
    return rows


def row_lists(rows):
    return [np.sort(r[r >= 0]).astype(np.uint64) for r in rows]


def edge_queries(rows):
    """every (u, v in row u), v +- 1, v = 0, v = N - 1, and nodes outside 0 .. N-1 -> (u int64, v int64; v = -1 is a legal question)"""
    N = rows.shape[0]
    u, v = [], []
    for i in range(N):
        r = rows[i][rows[i] >= 0].astype(np.int64)
        q = np.unique(np.concatenate([r, r - 1, r + 1, [0, N - 1]]))
        u.append(np.full(q.size, i, np.int64))
        v.append(q)
    for bad in (-1, -5, N, N + 5):
        u.append(np.full(3, bad, np.int64))
        v.append(np.array([0, 1, N - 1], np.int64))
    return np.concatenate(u), np.concatenate(v)


def check_graph(c, rows, u, v, what):
    """the C call on the codec object against the statement; no locate (graph objects hold no lists to locate in)"""
    lists = row_lists(rows)
    return check_rank(c, lists, u, v.view(np.uint64), what, locate=False, image=False)


@pytest.mark.parametrize("K,N", [(7, 63), (7, 64), (7, 65), (16, 64), (16, 65), (64, 63), (64, 64), (64, 65), (64, 300), (80, 130)])
def test_graph_rows_has_edges(K, N):
    """K <= 64: the arena, read in place; K = 80: the CSR form.  The arena object answers the same before and after a call that builds
    its CSR streams (export), and its image is then the same before and after a rank."""
    from vector_db_id_compression_amd import altid

    torch = _torch()
    rows = graph_rows(N, K, seed=40)
    g = altid.EliasFanoNSGGraph(rows)
    u, v = edge_queries(rows)
    what = f"rows K={K} N={N}"
    first = check_graph(g._c, rows, u, v, what)
    want = er.has_edges(rows, u, v)
    assert want.sum() == (rows >= 0).sum() and np.array_equal(first[1].astype(bool), want)
    for args in ((u, v), (dev_i64(u), dev_i64(v)), (u.tolist(), v.tolist())):
        got = g.has_edges(*args)
        sync()
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), f"{what}: has_edges"
    g._c.export(1)  # (builds the per-list streams of an arena object)
    before = ef_words(g._c)
    again = check_graph(g._c, rows, u, v, what + " after export")
    assert all(np.array_equal(a, b) for a, b in zip(first[:2], again[:2]))
    same(ef_words(g._c), before, f"{what}: the object changed")


def test_graph_rows_three_trips_on_one_cu(small):
    """20 001 pairs on an arena object: three trips of k_ef_rank_arena at one CU, the last one ragged"""
    rows = graph_rows(700, 16, seed=41)
    u, v = edge_queries(rows)
    rng = np.random.default_rng(3)
    n = 2 * TRIP_ARENA + 3617
    pick = rng.integers(0, u.size, n)
    u, v = u[pick], v[pick]
    cd = _codecs()
    a = check_graph(cd.EfLists.encode_rows(rows), rows, u, v, "arena, default context")
    b = check_graph(cd.EfLists.encode_rows(rows, ctx=small), rows, u, v, "arena, one CU")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] > 0


# --------------------------------------------------------------------------------------------------------------------- derived objects
def all_queries(lists):
    ln, ids = [], []
    for l, li in enumerate(lists):
        q = er.queries(li)
        ln.append(np.full(q.size, l, np.int64))
        ids.append(q)
    return np.concatenate(ln), np.concatenate(ids)


def test_objects_built_by_append_remove_merge_subset_and_load(tmp_path):
    """their directories were built by other paths than the encoder's; the statement runs on each object's own decode_lists"""
    from vector_db_id_compression_amd import merge, persist, removal, subset

    rng = np.random.default_rng(77)
    sizes = [0, 40, 5200, 0, 70, 513, 1]
    lists = [np.sort(rng.choice(1 << 22, n, replace=False)).astype(np.uint64) for n in sizes]
    lists[2][:4500] = np.arange(4500)  # a bucket across a batch boundary
    obj = encode(lists)
    add_ln = rng.integers(-1, len(sizes) + 1, 3000).astype(np.int64)
    add = rng.integers(0, 1 << 23, 3000, dtype=np.uint64)
    grown, _ = obj.append(dev_i64(add_ln), dev_u64(add), labels=False)
    shrunk, _ = removal.remove(grown, None, dev_u64(lr.concat(lists)[::3]))
    other = encode([np.sort(rng.integers(0, 1 << 21, n, dtype=np.uint64)) for n in (5, 0, 900, 3, 0, 0, 4000)])
    merged = merge.merge(obj, other, add_id=1 << 33)
    part, _ = subset.subset(merged, subset.ID_MOD, 3, 1)
    loaded = persist.load(persist.save(merged, str(tmp_path / "merged")))
    for name, o in (("append", grown), ("remove", shrunk), ("merge", merged), ("subset", part), ("load", loaded)):
        own = lists_of_obj(o)
        ln, ids = all_queries(own)
        assert ln.size > 1000, name
        check_rank(o, own, ln, ids, f"after {name}")


def test_graph_objects_built_by_update_rows_and_load(tmp_path):
    from vector_db_id_compression_amd import persist

    cd, torch = _codecs(), _torch()
    rows = graph_rows(200, 16, seed=42)
    g = cd.EfLists.encode_rows(rows)
    n_new = 230
    new_rows = graph_rows(60, 16, seed=43)
    nodes = np.concatenate([np.arange(200, 230), np.random.default_rng(4).integers(0, 200, 30)]).astype(np.int64)
    g2 = cd.update_rows(g, dev_i64(nodes), torch.from_numpy(new_rows).cuda(), n_new=n_new)
    sync()
    R = g2.decode_rows(None, 16)[0].cpu().numpy()
    assert R.shape == (n_new, 16) and (R[200:] >= 0).any()
    u, v = edge_queries(R)
    check_graph(g2, R, u, v, "after update_rows")
    back = persist.load(persist.save(g2, str(tmp_path / "g2")))  # (an imported graph object holds per-list streams: the CSR kernel on rows)
    check_rank(back, row_lists(R), u, v.view(np.uint64), "graph after load", locate=False)


# ------------------------------------------------------------------------------------------------------------------------ Python layer
def test_count_range_and_contains():
    lists, ln, ids = designed_object()
    obj = encode(lists)
    rng = np.random.default_rng(5)
    n = 4000
    pick = rng.integers(0, ln.size, n)
    bl = ln[pick].copy()
    lo, hi = ids[pick].copy(), ids[rng.integers(0, ln.size, n)].copy()
    lo[:300], hi[300:600] = 0, M64                      # lo = 0; hi = 2^64 - 1
    bl[600:640], bl[640:680] = -2, len(lists) + 1        # skipped, invalid
    swap = np.flatnonzero(hi < lo)
    assert swap.size > 100 and (hi >= lo).sum() > 100   # both hi < lo and ordinary ranges
    want = er.count_range(lists, bl, lo, hi)
    assert (want > 0).sum() > 100 and (want[swap] == 0).all()
    for args in ((dev_i64(bl), dev_u64(lo), dev_u64(hi)), (bl, lo, hi)):
        got = _rank().count_range(obj, *args)
        sync()
        assert got.dtype == _torch().int64 and np.array_equal(got.cpu().numpy(), want)
    _, want_f, _ = er.statement(lists, bl, lo)
    got = _rank().contains(obj, dev_i64(bl), dev_u64(lo))
    sync()
    assert got.dtype == _torch().bool and np.array_equal(got.cpu().numpy(), want_f.astype(bool))
    assert _rank().contains(obj, np.zeros(0, np.int64), np.zeros(0, np.uint64)).numel() == 0


def test_container_rank_batch_and_contains_batch():
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch = _torch()
    xb = np.random.default_rng(53).standard_normal((2000, 8)).astype(np.float32)
    idx = IVFIndex(8, 16, "Flat")
    idx.train(xb)
    idx.add(xb)
    il, _ = ci.apply_id_compression(idx, "elias-fano")
    every = torch.arange(2000, dtype=torch.int64, device="cuda")
    labels = il.locate_batch(None, every)
    lists = labels >> 32
    r = il.rank_batch(lists, every)
    assert torch.equal((lists << 32) | r, labels) and il.contains_batch(lists, every).all()
    assert not il.contains_batch((lists + 1) % 16, every).any()
    own = lists_of_obj(il._c)
    ln = np.repeat(np.arange(16), 3).astype(np.int64)
    ids = np.tile(np.array([0, 1000, 5000], np.uint64), 16)
    assert np.array_equal(il.rank_batch(ln, ids).cpu().numpy(), er.statement(own, ln, ids)[0])


def test_refusals_on_a_live_context_leave_it_usable():
    from vector_db_id_compression_amd import VidcError

    torch = _torch()
    L = _lib()
    lists = [lr.u64([1, 2, 5]), np.zeros(0, np.uint64)]
    obj = encode(lists)
    fn = L.lib().vidc_ef_rank_dev
    d_ln, d_ids = dev_i64([0, 0]), dev_u64([2, 9])
    out = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    sync()
    for args in ((None, obj.h, 2, L.ptr(d_ln), L.ptr(d_ids), L.ptr(out)), (obj.ctx.h, None, 2, L.ptr(d_ln), L.ptr(d_ids), L.ptr(out)),
                 (obj.ctx.h, obj.h, 2, None, L.ptr(d_ids), L.ptr(out)), (obj.ctx.h, obj.h, 2, L.ptr(d_ln), None, L.ptr(out)),
                 (obj.ctx.h, obj.h, 2, L.ptr(d_ln), L.ptr(d_ids), None), (obj.ctx.h, obj.h, 2 ** 32 - 1, L.ptr(d_ln), L.ptr(d_ids), L.ptr(out))):
        assert fn(*args, None, None) == -1 and b"ef rank" in L.lib().vidc_last_error()
    sync()
    assert out.tolist() == [7, 7]
    with pytest.raises(VidcError, match="EfLists.*list_nos=None"):
        _rank().rank(obj, None, d_ids)
    with pytest.raises(VidcError, match="PackedLists"):
        _rank().rank(_codecs().PackedLists.encode(lr.offsets_of(lists), dev_u64(lr.concat(lists)), bits=8), d_ln, d_ids)
    with pytest.raises(ValueError):
        _rank().rank(obj, d_ln, d_ids, found=torch.zeros(2, dtype=torch.int64, device="cuda"))
    r, f, inv = check_rank(obj, lists, [0, 0, 1, 2], [2, 9, 0, 1], "after the refusals")
    assert r.tolist() == [1, 3, 0, -1] and f.tolist() == [1, 0, 0, 0] and inv == 1
