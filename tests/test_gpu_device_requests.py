"""Device-resident requests: Faiss labels translated to ids (vidc_*_translate_labels_dev) and graph rows of a device node array
(vidc_*_decode_rows_dev, vidc_compact_rows_decode_dev) equal the host-array calls (decode_lists + indexing, decode_rows with numpy
nodes) exactly, count invalid entries exactly, move no payload over PCIe, run behind torch's queued work without a synchronisation,
and reach the Python surface (containers, altid graphs, the batched graph search)."""
import numpy as np
import pytest

from golden_cases import CASES, make_ids

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def dev64(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


# ---------------------------------------------------------------------------------------------------------------- data sets
def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64))]).astype(np.uint64)


def _sorted_ids(off, universe, rng):
    ids = np.empty(int(off[-1]), np.uint64)
    for l in range(off.size - 1):
        n = int(off[l + 1] - off[l])
        if n:
            u = np.unique(rng.integers(0, universe, 2 * n + 16, dtype=np.uint64))
            ids[off[l]:off[l + 1]] = np.sort(u[rng.permutation(u.size)[:n]])
    return ids


def _wt_ids(off, rng):
    """ids 0..ntotal-1, ascending inside every list (what the wavelet tree requires)"""
    perm = rng.permutation(int(off[-1])).astype(np.uint64)
    for l in range(off.size - 1):
        perm[off[l]:off[l + 1]].sort()
    return perm


def dataset(name):
    rng = np.random.default_rng(["golden", "s1", "short65536", "long", "big_ids"].index(name) + 100)
    if name == "golden":  # the golden cases' lists back to back, an empty list between two of them
        lists = [np.asarray(make_ids(c), dtype=np.uint64) for c in CASES]
        lists.insert(3, np.zeros(0, np.uint64))
        off = _offsets([x.size for x in lists])
        ids = np.concatenate(lists)
    elif name == "s1":  # S1 shape: 10^6 ids in 1024 Zipf(0.75) lists
        from vector_db_id_compression_amd import synth

        off, ids = synth.make_lists_numpy(1_000_000, 1024, 0.75, seed=5)
    elif name == "short65536":  # 65 536 short lists (ROC lane classes), some empty
        off = _offsets(rng.integers(0, 40, 65536))
        ids = rng.integers(0, 1 << 31, int(off[-1]), dtype=np.uint64)
    elif name == "long":  # one list over 16 384 ids (ROC chain classes) next to small ones
        off = _offsets([5, 20000, 0, 300, 1])
        ids = rng.integers(0, 1 << 31, int(off[-1]), dtype=np.uint64)
    elif name == "big_ids":  # ids >= 2^32 (packed bits, Elias-Fano)
        off = _offsets(rng.integers(0, 3000, 200))
        ids = _sorted_ids(off, 1 << 40, rng)
    else:
        raise ValueError(name)
    return np.asarray(off, np.uint64), np.asarray(ids, np.uint64)


_OBJ = {}


def build(codec, name):
    key = (codec, name)
    if key not in _OBJ:
        cd = _codecs()
        off, ids = dataset(name)
        if codec.startswith("wt"):
            ids = _wt_ids(off, np.random.default_rng(3))
            obj = cd.WaveletTreeLists.build(off, ids, wt_type=int(codec[-1]))
        elif codec == "packed":  # (wide enough for every id: the golden and big-id lists exceed bits_for(ntotal))
            bits = max(cd.PackedLists.bits_for(int(off[-1])), int(ids.max()).bit_length() if ids.size else 1)
            obj = cd.PackedLists.encode(off, ids, bits=bits)
        elif codec == "ef":
            obj = cd.EfLists.encode(off, ids)
        else:
            obj = cd.RocLists.encode(off, ids)
        nlist = off.size - 1
        flat, out_off = obj.decode_lists(np.arange(nlist, dtype=np.uint64))
        assert np.array_equal(out_off, off)
        _OBJ[key] = (obj, off, flat.cpu().numpy())
    return _OBJ[key]


def make_labels(off, n, rng):
    """valid labels (repeats included) mixed with -1, other negatives, list >= nlist, offset >= size, labels aimed at empty lists"""
    nlist = off.size - 1
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    ne = np.flatnonzero(sizes)
    l = rng.choice(ne, n).astype(np.int64)
    o = rng.integers(0, sizes[l])
    lab = (l << 32) | o
    kind = rng.integers(0, 100, n)
    lab[kind < 8] = -1
    lab[(kind >= 8) & (kind < 10)] = -rng.integers(2, 1 << 62, int(((kind >= 8) & (kind < 10)).sum()))
    m = (kind >= 10) & (kind < 13)
    lab[m] = ((nlist + rng.integers(0, 1000, int(m.sum()))) << 32) | rng.integers(0, 4, int(m.sum()))
    m = (kind >= 13) & (kind < 16)
    lab[m] = (l[m] << 32) | (sizes[l[m]] + rng.integers(0, 3, int(m.sum())))
    empty = np.flatnonzero(sizes == 0)
    m = (kind >= 16) & (kind < 18)
    if empty.size:
        lab[m] = rng.choice(empty, int(m.sum())).astype(np.int64) << 32
    if n > 4:  # repeats
        lab[n // 2: n // 2 + 3] = lab[n // 4]
    return lab


def expect(lab, off, flat):
    nlist = off.size - 1
    sizes = (off[1:] - off[:-1]).astype(np.int64)
    l = np.where(lab >= 0, lab >> 32, 0)
    o = lab & 0xFFFFFFFF
    valid = (lab >= 0) & (l < nlist)
    valid[valid] = o[valid] < sizes[l[valid]]
    out = np.full(lab.size, -1, np.int64)
    out[valid] = flat[off[l[valid]].astype(np.int64) + o[valid]]
    return out, int(((lab >= 0) & ~valid).sum())


CASES_T = [(c, d) for c in ("packed", "ef", "wt0", "wt1", "roc") for d in ("golden", "s1", "short65536", "long")] + \
          [("packed", "big_ids"), ("ef", "big_ids")]


# ------------------------------------------------------------------------------------------------------- 1. translation
@pytest.mark.parametrize("codec,name", CASES_T)
def test_translate_labels_equals_host_calls(codec, name):
    torch = _torch()
    obj, off, flat = build(codec, name)
    rng = np.random.default_rng(7)
    for n in (0, 1, 1000, 1_000_000):
        lab = make_labels(off, n, rng)
        want, bad = expect(lab, off, flat)
        d_lab = dev64(lab)
        inv = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = obj.translate_labels(d_lab, invalid=inv)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want), (codec, name, n)
        assert int(inv.item()) == bad, (codec, name, n)
        assert np.array_equal(d_lab.cpu().numpy(), lab)  # the input is left alone
        inplace = obj.translate_labels(d_lab, out=d_lab, invalid=inv)
        torch.cuda.synchronize()
        assert inplace is d_lab and np.array_equal(d_lab.cpu().numpy(), want), (codec, name, n)
        assert int(inv.item()) == 2 * bad


def test_translate_labels_matches_decode_gather_of_the_touched_lists():
    """the host-array decode section of the deferred search (np.unique of the touched lists + vidc_*_decode_gather)"""
    rng = np.random.default_rng(11)
    for codec in ("packed", "ef", "wt0", "roc"):
        obj, off, flat = build(codec, "s1")
        lab = make_labels(off, 20000, rng)
        lab = lab[lab >= 0]
        want, _ = expect(lab, off, flat)
        ok = want >= 0
        l, o = (lab[ok] >> 32).astype(np.uint64), (lab[ok] & 0xFFFFFFFF).astype(np.uint64)
        uniq, slot = np.unique(l, return_inverse=True)
        ref = obj.decode_gather(uniq, slot.astype(np.uint64), o)
        got = obj.translate_labels(dev64(lab)).cpu().numpy()
        assert np.array_equal(got[ok], ref), codec
        assert np.all(got[~ok] == -1)


# ------------------------------------------------------------------------------------------------- 2. no payload on PCIe
@pytest.mark.parametrize("codec", ["packed", "ef", "wt0", "roc"])
def test_translate_moves_no_payload_over_pcie(codec):
    torch = _torch()
    obj, off, flat = build(codec, "short65536")
    lab = dev64(make_labels(off, 200_000, np.random.default_rng(2)))
    before = obj.ctx.d2h_bytes()
    for _ in range(3):
        obj.translate_labels(lab)
    torch.cuda.synchronize()
    assert obj.ctx.d2h_bytes() == before


# ------------------------------------------------------------------------------------------ 3. ordering and asynchrony
def _busy_labels(lab):
    """labels produced by torch behind >= 10 ms of queued matmuls on the current stream (uploaded first: a copy from pageable host
    memory queued behind the matmuls would make the host wait for them before the call under test runs)"""
    torch = _torch()
    up = dev64(lab)
    torch.cuda.synchronize()
    big = torch.randn(4096, 4096, device="cuda")
    for _ in range(24):
        big = big @ big
        big = big / big.norm()
    return up + (big[0, 0] * 0).to(torch.int64)


@pytest.mark.parametrize("codec", ["packed", "ef", "wt0", "wt1", "roc"])
def test_translate_is_ordered_after_torch_and_does_not_wait(codec):
    torch = _torch()
    obj, off, flat = build(codec, "s1")
    rng = np.random.default_rng(5)
    obj.translate_labels(dev64(make_labels(off, 1000, rng)))  # warm: lazy tables
    torch.cuda.synchronize()
    for _ in range(2):
        lab = make_labels(off, 200_000, rng)
        want, bad = expect(lab, off, flat)
        d_lab = _busy_labels(lab)
        inv = torch.zeros(1, dtype=torch.int64, device="cuda")
        got = obj.translate_labels(d_lab, invalid=inv)
        still_busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        if codec != "roc":  # (ROC plans on the host and waits for the touched lists)
            assert still_busy, f"{codec}: the call waited for the stream"
        assert np.array_equal(got.cpu().numpy(), want)
        assert int(inv.item()) == bad


# ----------------------------------------------------------------------------------------------------- 4. stale scratch
def test_roc_translate_with_poisoned_pool_and_changing_touched_sets():
    torch = _torch()
    obj, off, flat = build("roc", "short65536")
    rng = np.random.default_rng(9)
    obj.ctx.set_pool_poison(True)
    try:
        for it in range(12):
            n = [10, 5000, 100, 200_000][it % 4]
            lab = make_labels(off, n, rng)
            if it % 3 == 0:  # a narrow band of lists
                lo = int(rng.integers(0, 60000))
                sizes = (off[1:] - off[:-1]).astype(np.int64)
                ls = np.arange(lo, lo + 50)
                ls = ls[sizes[ls] > 0]
                pick = rng.choice(ls, n)
                lab = (pick.astype(np.int64) << 32) | rng.integers(0, sizes[pick])
            want, bad = expect(lab, off, flat)
            inv = torch.zeros(1, dtype=torch.int64, device="cuda")
            got = obj.translate_labels(dev64(lab), invalid=inv)
            assert np.array_equal(got.cpu().numpy(), want), it
            assert int(inv.item()) == bad, it
    finally:
        obj.ctx.set_pool_poison(False)


# ------------------------------------------------------------------------------------------------------------ 5. rows
_GRAPHS = {}


def graph(kind, N, K):
    key = (kind, N, K)
    if key not in _GRAPHS:
        from vector_db_id_compression_amd import synth

        cd = _codecs()
        rows = synth.make_graph_rows(N, K, seed=K, dmin=max(1, K // 4))
        rows[::97] = -1  # nodes without edges
        cls = {"compact": cd.CompactRows, "ef": cd.EfLists, "roc": cd.RocLists}[kind]
        _GRAPHS[key] = cls.encode_rows(rows)
    return _GRAPHS[key]


def make_nodes(N, m, rng):
    nodes = rng.integers(0, N, m).astype(np.int64)
    kind = rng.integers(0, 100, m)
    nodes[kind < 5] = -1
    nodes[(kind >= 5) & (kind < 7)] = -rng.integers(2, 1 << 40, int(((kind >= 5) & (kind < 7)).sum()))
    nodes[(kind >= 7) & (kind < 10)] = N + rng.integers(0, 1 << 40, int(((kind >= 7) & (kind < 10)).sum()))
    if m > 8:
        nodes[m // 3: m // 3 + 5] = nodes[1]  # repeats
    return nodes


def check_rows(obj, N, K, m, rng, via_c=False):
    torch = _torch()
    nodes = make_nodes(N, m, rng)
    ok = (nodes >= 0) & (nodes < N)
    ref_out, ref_cnt = obj.decode_rows(np.where(ok, nodes, 0).astype(np.uint64), K)
    ref_out = ref_out.cpu().numpy().copy()
    ref_out[~ok] = -1
    ref_cnt = ref_cnt.astype(np.int64)
    ref_cnt[~ok] = 0
    d_nodes = dev64(nodes)
    if via_c:  # with the invalid count
        L = _lib()
        out = torch.empty((m, K), dtype=torch.int32, device="cuda")
        cnt = torch.empty(m, dtype=torch.int32, device="cuda")
        inv = torch.zeros(1, dtype=torch.int64, device="cuda")
        name = type(obj).__name__
        if name == "CompactRows":
            st = L.lib().vidc_compact_rows_decode_dev(obj.ctx.h, obj.h, m, L.ptr(d_nodes), L.ptr(out), L.ptr(cnt), L.ptr(inv))
        else:
            fn = L.lib().vidc_ef_decode_rows_dev if name == "EfLists" else L.lib().vidc_roc_decode_rows_dev
            st = fn(obj.ctx.h, obj.h, m, L.ptr(d_nodes), K, L.ptr(out), L.ptr(cnt), L.ptr(inv))
        L.check(st)
        torch.cuda.synchronize()
        assert int(inv.item()) == int(((nodes >= N)).sum())
    else:
        out, cnt = obj.decode_rows(d_nodes, K)
        assert cnt.is_cuda and cnt.dtype == torch.int32
        out2, none = obj.decode_rows(d_nodes, K, want_counts=False)
        assert none is None
        assert np.array_equal(out2.cpu().numpy(), ref_out)
    assert out.is_cuda
    assert np.array_equal(out.cpu().numpy(), ref_out), (type(obj).__name__, K, m)
    assert np.array_equal(cnt.cpu().numpy().astype(np.int64), ref_cnt), (type(obj).__name__, K, m)


ROW_SHAPES = [(k, K) for k in ("compact", "ef", "roc") for K in (16, 32, 64)] + [("compact", 80), ("roc", 80)]


@pytest.mark.parametrize("kind,K", ROW_SHAPES)
def test_rows_of_device_nodes_equal_host_nodes(kind, K):
    N = 20000
    obj = graph(kind, N, K)
    rng = np.random.default_rng(K)
    for m in (1, 100, 2048, 100_000):
        check_rows(obj, N, K, m, rng)
    check_rows(obj, N, K, 5000, rng, via_c=True)


@pytest.mark.parametrize("env", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
@pytest.mark.parametrize("kind", ["roc", "ef", "compact"])
def test_rows_of_device_nodes_off_the_lane_path(kind, env, monkeypatch):
    monkeypatch.setenv(env, "1")
    N, K = 20000, 32
    obj = graph(kind, N, K)
    rng = np.random.default_rng(3)
    for m in (100, 4096):
        check_rows(obj, N, K, m, rng, via_c=(m == 4096))


def test_ef_rows_off_the_arena_take_the_host_path():
    """Elias-Fano list objects (no arena) and K below a graph object's K: the nodes cross once and the host-node path decodes; rows
    wider than K fail as the host call fails"""
    cd = _codecs()
    rng = np.random.default_rng(4)
    off = _offsets(rng.integers(0, 41, 5000))
    ids = _sorted_ids(off, 1 << 31, rng)
    e = cd.EfLists.encode(off, ids)
    for m in (1, 3000):
        check_rows(e, 5000, 48, m, rng)
        check_rows(e, 5000, 48, m, rng, via_c=True)
    obj = graph("ef", 20000, 64)
    nodes = np.array([1, 2, 3], np.int64)
    with pytest.raises(_lib().VidcError):
        obj.decode_rows(nodes.astype(np.uint64), 1)
    with pytest.raises(_lib().VidcError):
        obj.decode_rows(dev64(nodes), 1)


@pytest.mark.parametrize("kind", ["compact", "ef"])
def test_rows_of_device_nodes_do_not_wait(kind):
    """compact rows and Elias-Fano graph rows only enqueue work -- also the calls that grow the context's request block: a fresh
    context serves 100 nodes, then 5*10^4 (growth), then 10^5 (growth), then 10^5 again, each behind queued torch work"""
    torch = _torch()
    L = _lib()
    from vector_db_id_compression_amd import synth

    cd = _codecs()
    N, K = 20000, 32
    ctx = L.Context(torch.cuda.current_device())
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rows = synth.make_graph_rows(N, K, seed=9, dmin=8)
    cls = cd.CompactRows if kind == "compact" else cd.EfLists
    obj = cls.encode_rows(rows, ctx=ctx)
    rng = np.random.default_rng(8)
    for m in (100, 50_000, 100_000, 100_000):
        nodes = make_nodes(N, m, rng)
        ok = (nodes >= 0) & (nodes < N)
        ref, _ = obj.decode_rows(np.where(ok, nodes, 0).astype(np.uint64), K)
        ref = ref.cpu().numpy().copy()
        ref[~ok] = -1
        d_nodes = _busy_labels(nodes)
        out, cnt = obj.decode_rows(d_nodes, K)
        still_busy = not torch.cuda.current_stream().query()
        torch.cuda.synchronize()
        if m > 100:  # (the first call of the process may load the kernels it launches)
            assert still_busy, (kind, m)
        assert np.array_equal(out.cpu().numpy(), ref), (kind, m)
    del obj
    ctx.close()


def test_host_path_rows_with_invalid_nodes_do_not_ask_for_node_0():
    """list objects take the host-node path; an invalid node must not make it decode a row (node 0 here) that is longer than K"""
    torch = _torch()
    cd = _codecs()
    rng = np.random.default_rng(13)
    sizes = rng.integers(0, 41, 3000)
    sizes[0] = 100  # list 0 is longer than K
    off = _offsets(sizes)
    ids = _sorted_ids(off, 1 << 31, rng)
    K = 48
    for obj in (cd.EfLists.encode(off, ids), cd.RocLists.encode(off, ids)):
        with pytest.raises(_lib().VidcError):  # the host call refuses node 0 itself
            obj.decode_rows(np.array([0, 5], np.uint64), K)
        ref, ref_cnt = obj.decode_rows(np.array([5, 7], np.uint64), K)
        nodes = dev64(np.array([-1, 5, 3000 + 4, 7, -9], np.int64))
        out, cnt = obj.decode_rows(nodes, K)
        torch.cuda.synchronize()
        out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(out[[1, 3]], ref.cpu().numpy()) and np.array_equal(cnt[[1, 3]], ref_cnt.astype(np.int32))
        assert (out[[0, 2, 4]] == -1).all() and (cnt[[0, 2, 4]] == 0).all()
        out, cnt = obj.decode_rows(dev64(np.array([-1, 3000], np.int64)), K)  # no valid node at all: nothing is decoded
        assert (out.cpu().numpy() == -1).all() and (cnt.cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------------- 6. surface
@pytest.mark.parametrize("which", range(5))
def test_containers_translate_labels(which):
    torch = _torch()
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    rng = np.random.default_rng(21)
    assign = rng.integers(0, 64, 30000)
    il = ArrayInvertedLists.from_assignment(assign, 64, code_size=4)
    cls = [ci.CompressedIDInvertedListsPackedBits, ci.CompressedIDInvertedListsFenwickTree, ci.CompressedIDInvertedListsEliasFano,
           ci.CompressedIDInvertedListsWaveletTree, lambda x: ci.CompressedIDInvertedListsWaveletTree(x, 1)][which]
    c = cls(il)
    sizes = np.array([c.list_size(l) for l in range(64)], np.int64)
    l = rng.choice(np.flatnonzero(sizes), 5000)
    o = rng.integers(0, sizes[l])
    want = c.get_single_ids(l.astype(np.uint64), o.astype(np.uint64))
    lab = (l.astype(np.int64) << 32) | o
    lab[::10] = -1
    want[::10] = -1
    d_lab = dev64(lab.reshape(100, 50))  # (nq, k) as a search returns them
    got = c.translate_labels(d_lab, out=d_lab)
    torch.cuda.synchronize()
    assert got is d_lab
    assert np.array_equal(d_lab.cpu().numpy().reshape(-1), want)


def test_altid_graphs_get_neighbors_device_of_a_cuda_tensor():
    from vector_db_id_compression_amd import altid
    from vector_db_id_compression_amd.graph_search import RawGraph

    rng = np.random.default_rng(6)
    rows = _random_rows(rng, 3000, 24)
    nodes = rng.integers(0, 3000, 4000).astype(np.int64)
    raw = RawGraph(rows)
    ref = raw.get_neighbors_device(nodes).cpu().numpy()
    nodes_neg = nodes.copy()
    nodes_neg[::7] = -1
    ref_neg = ref.copy()
    ref_neg[::7] = -1
    assert np.array_equal(raw.get_neighbors_device(dev64(nodes_neg)).cpu().numpy(), ref_neg)
    nodes_big = nodes_neg.copy()
    nodes_big[3::11] = 3000 + 5  # nodes >= N: a row of -1 as well, for the raw and the compressed graphs
    ref_big = ref_neg.copy()
    ref_big[3::11] = -1
    assert np.array_equal(raw.get_neighbors_device(dev64(nodes_big)).cpu().numpy(), ref_big)
    for name, cls in altid.AVAILABLE_COMPRESSED_GRAPHS.items():
        if cls is None:
            continue
        g = cls(rows.copy())
        host = g.get_neighbors_device(nodes).cpu().numpy()
        got = g.get_neighbors_device(dev64(nodes)).cpu().numpy()
        assert np.array_equal(got, host), name
        exp = host.copy()
        exp[::7] = -1
        assert np.array_equal(g.get_neighbors_device(dev64(nodes_neg)).cpu().numpy(), exp), name
        exp[3::11] = -1
        assert np.array_equal(g.get_neighbors_device(dev64(nodes_big)).cpu().numpy(), exp), name


def _random_rows(rng, N, K):
    rows = np.full((N, K), -1, dtype=np.int32)
    for i in range(N):
        d = int(rng.integers(1, K + 1))
        rows[i, :d] = rng.choice(N, size=d, replace=False)
    return rows


def test_batched_graph_search_on_device_frontiers_is_identical():
    """search_batched hands its frontier over as a CUDA tensor; 2 048 queries put ROC on its lean device path"""
    from vector_db_id_compression_amd import altid
    from vector_db_id_compression_amd.graph_search import RawGraph, knn_graph, search_batched

    rng = np.random.default_rng(12)
    x = rng.normal(size=(6000, 16)).astype(np.float32)
    xq = rng.normal(size=(2048, 16)).astype(np.float32)
    rows = knn_graph(x, 24, seed=3)
    raw = RawGraph(rows)
    first = raw.get_neighbors_device(dev64(np.array([-1, 0])))  # a finished query's -1 gives a row of -1, not the last row
    assert (first[0] == -1).all() and np.array_equal(first[1].cpu().numpy(), rows[0])
    Dref, Iref = search_batched(raw, x, xq, 10, L=32)
    assert (Iref >= 0).all()
    for name, cls in altid.AVAILABLE_COMPRESSED_GRAPHS.items():
        if cls is None:
            continue
        D, I = search_batched(cls(rows.copy()), x, xq, 10, L=32)
        np.testing.assert_array_equal(I, Iref, err_msg=name)
        np.testing.assert_allclose(D, Dref, rtol=1e-6, err_msg=name)
