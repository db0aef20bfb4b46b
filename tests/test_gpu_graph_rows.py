"""The three graph-row containers (Elias-Fano arena, compact bits, ROC) against the numpy model of tests/rows_ref.py -- for ROC against
the pinned oracle -- on the row families that reach what uniform random rows never do: records on the 3 n + 1 high-bit bound and in
the last low word of the arena record, both sides of every step of l, the u < n branch, the sentinel in every field position, whole
tiles of empty and of full rows, garbage behind the terminator, ids up to 2^31 - 1; at every K on either side of a decoder template
switch (a_hw: 21/22, 42/43, 63/64; K % 4; K = 32 / 64) and node counts 1, 2, around the 64-row tile and around the powers of two at
which the compact field width and the sentinel change.

Every comparison is between integers and exact: stream words, bit counts, l, universe, byte images, sizes, every decode form.
tests/test_rows_ref_cpu.py checks the model itself and that the families produce the structures they are named for."""
import numpy as np
import pytest

import rows_ref as rr

pytestmark = pytest.mark.gpu

KS = [1, 3, 4, 20, 21, 22, 31, 32, 33, 42, 43, 63, 64]
#: every N with the K it is paired with: quad and non-quad, full and partial, every a_hw
N_WITH_K = [(1, 4), (2, 3), (63, 43), (64, 32), (65, 21), (129, 64), (700, 33), (4097, 20)]
K_SWEEP_N = 65  # two tiles, the second one of a single row
#: above this many rows the per-row exports look at a fixed sample (every row of a boundary family stays in)
EXPORT_ALL_MAX = 2000
LARGE_N = 65536 + 37


def _torch():
    import torch

    return torch


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def dev_rows(rows, misaligned=False):
    """int32 [N, K] CUDA tensor; misaligned: 4 bytes off a 16-byte boundary"""
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32))
    if not misaligned:
        return t.cuda()
    flat = torch.full((rows.size + 1,), -1, dtype=torch.int32, device="cuda")
    flat[1:] = t.reshape(-1).cuda()
    out = flat[1:].view(rows.shape)
    assert out.data_ptr() % 16 != 0
    return out


def sample_rows(N, boundary, seed=0):
    """the rows whose records are exported one by one: all of them up to EXPORT_ALL_MAX and in a boundary family, else a fixed sample
    with rows 0, 63, 64, N - 64, N - 1 and whatever `boundary` names"""
    if N <= EXPORT_ALL_MAX or boundary is True:
        return np.arange(N)
    rng = np.random.default_rng(seed)
    must = np.concatenate([[0, 63, 64, N - 64, N - 1], np.asarray(boundary if boundary is not False else [], dtype=np.int64)])
    rest = rng.choice(N, EXPORT_ALL_MAX - must.size, replace=False)
    return np.unique(np.concatenate([must, rest]))


def request_nodes(N, seed=0):
    """a host node list: every node in reverse order, then repeats"""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.arange(N)[::-1], [0, 0, N - 1], rng.integers(0, N, 5)]).astype(np.uint64)


def _diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}" if len(bad) else "equal"


def check_decodes(g, K, want, deg, what):
    """decode_rows of every node in order, of a host node list with repeats in reverse order and of a CUDA node tensor"""
    torch = _torch()
    N = want.shape[0]
    every, cnt = g.decode_rows(None, K)
    assert np.array_equal(every.cpu().numpy(), want), f"{what}: decode_rows(None) {_diff(every.cpu().numpy(), want)}"
    assert np.array_equal(cnt, deg), f"{what}: counts"
    nodes = request_nodes(N, seed=N)
    idx = nodes.astype(np.int64)
    sub, c2 = g.decode_rows(nodes, K)
    assert np.array_equal(sub.cpu().numpy(), want[idx]), f"{what}: decode_rows(host nodes) {_diff(sub.cpu().numpy(), want[idx])}"
    assert np.array_equal(c2, deg[idx]), f"{what}: counts of a host node list"
    dn = torch.from_numpy(np.concatenate([idx, [-1]])).cuda()
    dsub, c3 = g.decode_rows(dn, K)
    dsub = dsub.cpu().numpy()
    assert np.array_equal(dsub[:-1], want[idx]), f"{what}: decode_rows(CUDA nodes) {_diff(dsub[:-1], want[idx])}"
    assert (dsub[-1] == -1).all(), f"{what}: a negative node is a row of -1"
    assert np.array_equal(c3.cpu().numpy()[:-1], deg[idx]), f"{what}: counts of a CUDA node tensor"


def ef_all_words(g):
    """the CSR streams of the whole object (what save() writes)"""
    import ctypes as C

    from vector_db_id_compression_amd._lib import check, lib, ptr

    lw, hw = C.c_uint64(), C.c_uint64()
    check(lib().vidc_ef_stream_words(g.h, C.byref(lw), C.byref(hw)))
    low, high = np.zeros(max(lw.value, 1), np.uint64), np.zeros(max(hw.value, 1), np.uint64)
    check(lib().vidc_ef_export_all(g.ctx.h, g.h, ptr(low), lw.value, ptr(high), hw.value))
    return low[: lw.value], high[: hw.value]


# ------------------------------------------------------------------------------------------------------------------ Elias-Fano
def check_ef(rows, what, boundary=False, tmp_path=None, pairs_max=None):
    EfLists = _codecs().EfLists
    VidcError = _lib().VidcError
    N, K = rows.shape
    m = rr.ef_rows(rows)
    want, deg = rr.expected_ef(rows)
    g = EfLists.encode_rows(dev_rows(rows))
    info = g.info()
    assert np.array_equal(info["sizes"], deg), f"{what}: sizes"
    assert np.array_equal(info["low_bits"], m.l), f"{what}: low_bits {_diff(info['low_bits'], m.l)}"
    assert np.array_equal(info["universe"], m.u.astype(np.uint64)), f"{what}: universe {_diff(info['universe'], m.u)}"
    assert g.compressed_bytes == m.size_in_bytes, f"{what}: compressed_bytes {g.compressed_bytes}, model {m.size_in_bytes}"
    for i in sample_rows(N, boundary, seed=N + K):
        low, high, lb, hb = g.export(int(i))
        wl, wh = m.words(i)
        assert (lb, hb) == (int(m.low_nbits[i]), int(m.high_nbits[i])), f"{what}: row {i}: bits ({lb}, {hb})"
        assert np.array_equal(low, wl), f"{what}: row {i} (n {deg[i]}, l {m.l[i]}, u {m.u[i]}): low words {low} / {wl}"
        assert np.array_equal(high, wh), f"{what}: row {i} (n {deg[i]}, l {m.l[i]}, u {m.u[i]}): high words {high} / {wh}"
    check_decodes(g, K, want, deg, f"{what} elias-fano")
    # the same rows from an array 4 bytes off a 16-byte boundary: the same object
    g2 = EfLists.encode_rows(dev_rows(rows, misaligned=True))
    a, b = ef_all_words(g), ef_all_words(g2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{what}: misaligned rows give other words"
    assert g2.compressed_bytes == g.compressed_bytes
    assert np.array_equal(g2.decode_rows(None, K)[0].cpu().numpy(), want), f"{what}: misaligned rows decode"
    del g2
    # save, load, decode
    if tmp_path is not None:
        path = str(tmp_path / "ef.npz")
        g.save(path)
        back = EfLists.load(path)
        got, cnt = back.decode_rows(None, K)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cnt, deg), f"{what}: decode after save / load"
        assert back.compressed_bytes == m.size_in_bytes
        del back
    # get and decode_lists through the CSR built from the arena
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    assert np.array_equal(g.offsets, off.astype(np.uint64)), f"{what}: offsets"
    flat = want[np.arange(K)[None, :] < deg[:, None]].astype(np.int64)
    if flat.size:
        pl = np.repeat(np.arange(N), deg)
        po = np.arange(flat.size) - off[pl]
        pick = np.arange(flat.size)
        if pairs_max is not None and flat.size > pairs_max:
            pick = np.random.default_rng(N).integers(0, flat.size, pairs_max)
        got = g.get(pl[pick], po[pick])
        assert np.array_equal(got, flat[pick]), f"{what}: get {_diff(got, flat[pick])}"
    rng = np.random.default_rng(K)
    req = sample_rows(N, boundary, seed=N)
    req = req[rng.permutation(req.size)]
    req = np.concatenate([req, req[:2]]).astype(np.uint64)
    out, out_off = g.decode_lists(req)
    ri = req.astype(np.int64)
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum(deg[ri])]).astype(np.uint64)), f"{what}: decode_lists offsets"
    want_flat = np.concatenate([want[i, : deg[i]] for i in ri] + [np.zeros(0, np.int32)]).astype(np.int64)
    assert np.array_equal(out.cpu().numpy(), want_flat), f"{what}: decode_lists"
    # a narrower output: fine while the requested nodes fit, an error otherwise
    if K > 1:
        K2 = K - 1
        fits = np.flatnonzero(deg <= K2)[:200].astype(np.uint64)
        if fits.size:
            got, cnt = g.decode_rows(fits, K2)
            assert np.array_equal(got.cpu().numpy(), want[fits.astype(np.int64), :K2]), f"{what}: decode_rows at K - 1"
            assert np.array_equal(cnt, deg[fits.astype(np.int64)])
        wide = np.flatnonzero(deg > K2)
        if wide.size:
            with pytest.raises(VidcError, match="more than K edges"):
                g.decode_rows(np.concatenate([fits[:3], wide[:1].astype(np.uint64)]), K2)
    return g


# --------------------------------------------------------------------------------------------------------------------- compact
def check_compact(rows, what, boundary=False):
    CompactRows = _codecs().CompactRows
    VidcError = _lib().VidcError
    N, K = rows.shape
    img = rr.compact_rows(rows)
    want, deg = rr.expected_compact(rows)
    for misaligned in (False, True):
        tag = f"{what} compact{' (misaligned rows)' if misaligned else ''}"
        c = CompactRows.encode_rows(dev_rows(rows, misaligned))
        assert (c.bits, c.stride) == (rr.compact_bits(N), rr.compact_stride(N, K)), f"{tag}: bits / stride ({c.bits}, {c.stride})"
        assert c.size_in_bytes == N * rr.compact_stride(N, K), f"{tag}: size_in_bytes"
        for i in (sample_rows(N, boundary, seed=N + K) if not misaligned else sample_rows(N, False, seed=1)[:64]):
            got = c.export_row(int(i))
            assert np.array_equal(got, img[i]), f"{tag}: row {i} (degree {deg[i]}): image {got.tolist()} / {img[i].tolist()}"
        check_decodes(c, K, want, deg, tag)
        del c
    bad = np.array(rows, dtype=np.int32)
    bad[N // 2, 0] = N  # an id equal to N (the sentinel's value) where a neighbour must stand
    bad[N // 2, 1:] = -1
    with pytest.raises(VidcError, match="status -4"):
        CompactRows.encode_rows(dev_rows(bad))


# ------------------------------------------------------------------------------------------------------------------------- ROC
_roc_cache = {}


def roc_expectation(oracle, rows, key, only=None):
    """Per row what the pinned oracle makes of it: precision, head, stack words, encoder-side mt19937 draws, and the row as its decoder
    gives it back -- roc_decode(roc_encode(row)), power-of-two precision quirk included.  Computed once per input."""
    if key in _roc_cache:
        return _roc_cache[key]
    N, K = rows.shape
    deg = rr.row_degrees(rows)
    idx = np.arange(N) if only is None else only
    exp = dict(rows=idx, prec=np.zeros(N, np.uint32), heads=np.zeros(N, np.uint64), nwords=np.zeros(N, np.uint32),
               draws=np.zeros(N, np.uint32), words={}, dec=np.full((N, K), -1, np.int32))
    for i in idx:
        d = int(deg[i])
        if not d:
            continue
        ids = rows[i, :d].astype(np.uint64)
        P = oracle.list_precision(ids)
        e = oracle.roc_encode(ids, P)
        exp["prec"][i], exp["heads"][i], exp["nwords"][i], exp["draws"][i] = P, e["head"], e["words"].size, e["mt_draws"]
        exp["words"][int(i)] = e["words"]
        exp["dec"][i, :d] = oracle.roc_decode(e["head"], e["words"], d, P, e["mt_draws"])[0].astype(np.int64)
    _roc_cache[key] = exp
    return exp


def check_roc(rows, what, oracle, monkeypatch, key, boundary=False):
    RocLists = _codecs().RocLists
    N, K = rows.shape
    deg = rr.row_degrees(rows)
    full = N <= EXPORT_ALL_MAX or boundary is True
    exp = roc_expectation(oracle, rows, key, None if full else sample_rows(N, boundary, seed=N + K))
    idx = exp["rows"]
    ne = idx[deg[idx] > 0]  # (an empty row has no stream: only its size and word count are compared)
    for force in ("1", "0"):
        monkeypatch.setenv("VIDC_FORCE_LANE", force)
        monkeypatch.setenv("VIDC_NO_LANE", "0" if force == "1" else "1")
        tag = f"{what} roc ({'lane' if force == '1' else 'wave'}-per-row kernels)"
        g = RocLists.encode_rows(dev_rows(rows))
        info = g.info()
        assert np.array_equal(info["sizes"], deg), f"{tag}: num_outgoing_edges"
        assert np.array_equal(g.offsets, np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)), f"{tag}: offsets"
        assert not info["nwords"][deg == 0].any(), f"{tag}: words of an empty row"
        for name, k in (("precision", "prec"), ("heads", "heads"), ("nwords", "nwords"), ("mt_draws", "draws")):
            assert np.array_equal(info[name][ne], exp[k][ne]), f"{tag}: {name} {_diff(info[name][ne], exp[k][ne])}"
        words = g.all_words()
        woff = np.concatenate([[0], np.cumsum(info["nwords"].astype(np.int64))])
        for i in ne:
            assert np.array_equal(words[woff[i]:woff[i + 1]], exp["words"][int(i)]), f"{tag}: row {i}: stack words"
        every, cnt = g.decode_rows(None, K)
        every = every.cpu().numpy()
        assert np.array_equal(cnt, deg), f"{tag}: counts"
        assert np.array_equal(every[idx], exp["dec"][idx]), f"{tag}: decode_rows(None) {_diff(every[idx], exp['dec'][idx])}"
        assert (every[np.arange(K)[None, :] >= deg[:, None]] == -1).all(), f"{tag}: -1 behind the degree"
        nodes = idx[::-1].astype(np.uint64)
        nodes = np.concatenate([nodes, nodes[:2]])
        sub, c2 = g.decode_rows(nodes, K)
        assert np.array_equal(sub.cpu().numpy(), exp["dec"][nodes.astype(np.int64)]), f"{tag}: decode_rows(host nodes)"
        assert np.array_equal(c2, deg[nodes.astype(np.int64)])
        dsub, c3 = g.decode_rows(_torch().from_numpy(nodes.astype(np.int64)).cuda(), K)
        assert np.array_equal(dsub.cpu().numpy(), exp["dec"][nodes.astype(np.int64)]), f"{tag}: decode_rows(CUDA nodes)"
        assert np.array_equal(c3.cpu().numpy(), deg[nodes.astype(np.int64)])
        del g
    monkeypatch.delenv("VIDC_FORCE_LANE")
    monkeypatch.delenv("VIDC_NO_LANE")


def check_graph(name, N, K, oracle, monkeypatch, tmp_path, codecs=("ef", "compact", "roc")):
    rows = rr.family(name, N, K, seed=N + K)
    what = f"{name} N {N} K {K}"
    boundary = name in rr.BOUNDARY
    if "ef" in codecs:
        check_ef(rows, what, boundary, tmp_path)
    if "compact" in codecs and name not in rr.NOT_FOR_COMPACT:
        check_compact(rows, what, boundary)
    if "roc" in codecs and name not in rr.NOT_FOR_ROC:
        check_roc(rows, what, oracle, monkeypatch, (name, N, K), boundary)


# ----------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", rr.FAMILIES)
def test_every_family_at_every_K(name, K, oracle, monkeypatch, tmp_path):
    """65 nodes (a full tile and a tile of one row) at every K around the decoder template switches"""
    check_graph(name, K_SWEEP_N, K, oracle, monkeypatch, tmp_path)


@pytest.mark.parametrize("N,K", N_WITH_K)
@pytest.mark.parametrize("name", rr.FAMILIES)
def test_every_family_at_every_N(name, N, K, oracle, monkeypatch, tmp_path):
    """1 node and 2 nodes (the one-word record: LW = 0, S = 1), either side of the 64-row tile, several tiles, and 4 097 nodes (13-bit
    compact fields, 65 tiles)"""
    check_graph(name, N, K, oracle, monkeypatch, tmp_path)


#: per N: a K whose stride is a whole number of dwords (the tile kernels), one whose stride is not (the wave-per-row kernels), one
#: above 64 (the wide kernels)
COMPACT_SHAPES = [(255, 4), (255, 3), (255, 70), (256, 32), (256, 5), (256, 65), (257, 32), (257, 5), (257, 65),
                  (4095, 8), (4095, 3), (4095, 66), (4096, 32), (4096, 5), (4096, 67)]


@pytest.mark.parametrize("N,K", COMPACT_SHAPES)
def test_compact_field_width_boundaries(N, K):
    """N = 255 | 256 (8 | 9 bits, the sentinel 2^8 itself), 257, 4095 | 4096 (12 | 13 bits), through each of the three kernel pairs"""
    bits = rr.compact_bits(N)
    assert bits == {255: 8, 256: 9, 257: 9, 4095: 12, 4096: 13}[N]
    stride = rr.compact_stride(N, K)
    assert (K > 64) or (stride % 4 == 0) == (K in (4, 32, 8))
    for name in ("degrees", "dups", "garbage_tail", "blocks"):
        check_compact(rr.family(name, N, K, seed=N + K), f"{name} N {N} K {K}")


def test_a_graph_whose_roc_decode_orders_rows_by_edge_count(oracle, monkeypatch, tmp_path):
    """65 573 nodes: uniform rows, with rows of every boundary family (built for this N) and blocks of full and of empty rows placed
    inside; per-row exports on a fixed sample of 2 000 rows that holds rows 0, 63, 64, N - 64, N - 1 and every one of the placed rows;
    50 000 random (row, offset) pairs for get; every row through every decode form."""
    N, K = LARGE_N, 43  # (K: neither full nor a multiple of 4, three high words)
    rows = rr.family("uniform", N, K, seed=K)
    placed = []
    at = 640
    for name, count in (("l_steps", 320), ("max_high", 128), ("max_low", 64), ("prefix", 64), ("blocks", 192)):
        rows[at:at + count] = rr.family(name, N, K, seed=K, nrows=count)
        placed.append(np.arange(at, at + count))
        at += count + 37
    placed = np.concatenate(placed)
    what = f"large N {N} K {K}"
    check_ef(rows, what, placed, tmp_path, pairs_max=50_000)
    check_compact(rows, what, placed)
    check_roc(rows, what, oracle, monkeypatch, ("large", N, K), placed)


def test_global_ids_size_the_arena_on_a_second_pass():
    """ids far above N: the first pass sizes records for ids < N, meets a larger id and reports it, the second pass sizes them for
    2^31 - 1 (K = 64: 25 low words).  The same rows with the large ids taken out fit the first pass: both objects against the model."""
    N, K = 129, 64
    rows = rr.family("global_ids", N, K, seed=1)
    g = check_ef(rows, "global ids")
    assert int(g.info()["universe"].max()) == rr.TOP
    check_ef(np.where(rows >= N, rows % N, rows).astype(np.int32), "global ids folded below N")


@pytest.mark.parametrize("name", ["blocks", "max_high", "max_low"])
def test_poisoned_pool(name, oracle, monkeypatch, tmp_path):
    """Every cached device block is 0xFF when it is handed out: the unused words of an arena record, the records of empty rows, the
    fields behind a sentinel and the bytes of a tile that holds empty rows only must be written, not inherited.  Twice: the second
    pass takes the blocks the first one released."""
    ctx = _lib().default_context()
    ctx.set_pool_poison(True)
    try:
        for N, K in ((129, 64), (200, 21)):
            check_graph(name, N, K, oracle, monkeypatch, tmp_path)
            check_graph(name, N, K, oracle, monkeypatch, tmp_path)
    finally:
        ctx.set_pool_poison(False)


@pytest.mark.parametrize("N,K", [(200, 33), (130, 64)])
def test_altid_graph_classes_on_every_degree(N, K, oracle):
    """The three drop-in graph classes on rows of degree 0 .. K: get_neighbors_batch, get_neighbors, the size fields."""
    from vector_db_id_compression_amd import altid

    rows = rr.family("degrees", N, K, seed=N + K)
    deg = rr.row_degrees(rows)
    nodes = np.concatenate([np.arange(N)[::-1], [3, 3]])
    exp = roc_expectation(oracle, rows, ("degrees", N, K))
    wants = {"elias-fano": rr.expected_ef(rows)[0], "compact": rr.expected_compact(rows)[0], "roc": exp["dec"]}
    for cname, want in wants.items():
        g = altid.AVAILABLE_COMPRESSED_GRAPHS[cname](rows.copy())
        out, cnt = g.get_neighbors_batch(nodes)
        assert np.array_equal(out, want[nodes]), f"{cname}: get_neighbors_batch {_diff(out, want[nodes])}"
        assert np.array_equal(cnt, deg[nodes]), cname
        for i in (0, K, N - 1):
            assert g.get_neighbors(i).tolist() == want[i, : deg[i]].tolist(), (cname, i)
        if cname == "elias-fano":
            assert g.compressed_ids_size_in_bytes == rr.ef_rows(rows).size_in_bytes
        elif cname == "compact":
            assert (g.bits, g.stride) == (rr.compact_bits(N), rr.compact_stride(N, K))
            assert g.compressed_ids_size_in_bytes == N * rr.compact_stride(N, K)
        else:
            assert np.array_equal(g.num_outgoing_edges, deg)
            assert g.compressed_ids_size_in_bytes == 8 * N + 4 * int(exp["nwords"].sum())
            assert np.array_equal(g.id_symbol_precision[deg > 0], exp["prec"][deg > 0])
