"""tests/rows_ref.py against the CPU oracle, a bit-by-bit packer and hand-computed graphs; and every family against its name.
(The GPU side of the same model and families: tests/test_gpu_graph_rows.py.)"""
import numpy as np
import pytest

import rows_ref as rr

#: (N, K): one row, the one-word record, a tile edge with K on an a_hw switch, odd K over several tiles, full-width rows
SHAPES = [(1, 4), (2, 3), (65, 21), (257, 33), (300, 64)]


def _rows(name, N, K):
    return rr.family(name, N, K, seed=N + K)


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("name", rr.FAMILIES)
def test_model_equals_the_oracle_on_every_row(name, N, K, oracle):
    rows = _rows(name, N, K)
    assert rows.shape == (N, K) and rows.dtype == np.int32
    deg = rr.row_degrees(rows)
    m = rr.ef_rows(rows)
    bits, stride = rr.compact_bits(N), rr.compact_stride(N, K)
    assert bits == oracle.packed_bits_for(N) and stride == (K * bits + 7) // 8
    img = rr.compact_rows(rows) if name not in rr.NOT_FOR_COMPACT else None
    total = 0
    for i in range(N):
        d = int(deg[i])
        assert int(m.n[i]) == d
        low, high = m.words(i)
        if d == 0:
            assert low.size == 0 and high.size == 0 and m.low_nbits[i] == 0 and m.high_nbits[i] == 0
        else:
            ids = rows[i, :d].astype(np.uint64)
            e = oracle.ef_build(np.sort(ids), universe=int(ids.max()))
            assert (int(m.l[i]), int(m.low_nbits[i]), int(m.high_nbits[i]), int(m.u[i])) == (e["l"], e["low_nbits"], e["high_nbits"],
                                                                                             int(ids.max())), (name, i)
            assert np.array_equal(low, e["low"]) and np.array_equal(high, e["high"]), (name, i)
            assert np.array_equal(e["decoded"], np.sort(ids))
            total += e["low_nbits"] + e["high_nbits"]
        if img is not None:
            fields = np.concatenate([rows[i, :d], [N] if d < K else []]).astype(np.uint64)
            want = oracle.packed_encode(fields, bits)
            assert np.array_equal(img[i, : want.size], want) and not img[i, want.size:].any(), (name, i)
    assert m.size_in_bytes == total // 8
    assert not m.low[np.arange(m.low.shape[1])[None, :] >= ((m.low_nbits + 63) // 64)[:, None]].any()
    assert not m.high[np.arange(m.high.shape[1])[None, :] >= ((m.high_nbits + 63) // 64)[:, None]].any()


def _pack_bits(fields, width, nbytes):
    """one bit at a time, LSB first"""
    out = np.zeros(nbytes, dtype=np.uint8)
    pos = 0
    for f in fields:
        for b in range(width):
            if (int(f) >> b) & 1:
                out[pos >> 3] |= 1 << (pos & 7)
            pos += 1
    return out


@pytest.mark.parametrize("name", ["uniform", "l_steps", "max_high", "max_low", "degrees", "dups", "global_ids"])
def test_model_equals_a_bit_by_bit_packer(name):
    N, K = 40, 7
    rows = _rows(name, N, K)
    deg = rr.row_degrees(rows)
    m = rr.ef_rows(rows)
    bits, stride = rr.compact_bits(N), rr.compact_stride(N, K)
    img = rr.compact_rows(rows) if name not in rr.NOT_FOR_COMPACT else None
    for i in range(N):
        d = int(deg[i])
        ids = sorted(int(x) for x in rows[i, :d])
        if d:
            u = max(ids)
            l = (u // d).bit_length() - 1 if u // d else 0
            lb, hb = d * l, d + (u >> l) + 2
            low = _pack_bits([x & ((1 << l) - 1) for x in ids], l, 8 * ((lb + 63) // 64)).view(np.uint64)
            high = np.zeros(8 * ((hb + 63) // 64), dtype=np.uint8)
            for e, x in enumerate(ids):
                p = (x >> l) + e
                assert p < hb
                high[p >> 3] |= 1 << (p & 7)
            got_low, got_high = m.words(i)
            assert (int(m.low_nbits[i]), int(m.high_nbits[i])) == (lb, hb)
            assert np.array_equal(got_low, low) and np.array_equal(got_high, high.view(np.uint64)), (name, i)
        if img is not None:
            fields = [int(x) for x in rows[i, :d]] + ([N] if d < K else [])
            assert np.array_equal(img[i], _pack_bits(fields, bits, stride)), (name, i)


def test_sizes_of_two_hand_computed_graphs():
    # graph A: 4 nodes, K = 3.  Compact: 2^3 >= 5: 3 bits, stride 2.
    a = np.array([[1, 3, -1], [0, -1, -1], [-1, -1, -1], [2, 0, 1]], dtype=np.int32)
    m = rr.ef_rows(a)
    # row 0: n 2, u 3, l = msb(1) = 0: no low bits, 2 + 3 + 2 high bits, bits 1 + 0 and 3 + 1.  row 1: n 1, u 0: 3 high bits, bit 0.
    # row 3: ids 0 1 2, u 2 < n: l 0, 3 + 2 + 2 bits, bits 0 2 4
    assert m.l.tolist() == [0, 0, 0, 0] and m.u.tolist() == [3, 0, 0, 2]
    assert m.low_nbits.tolist() == [0, 0, 0, 0] and m.high_nbits.tolist() == [7, 3, 0, 7]
    assert [m.words(i)[1].tolist() for i in range(4)] == [[0b10010], [1], [], [0b10101]]
    assert m.size_in_bytes == 17 // 8
    assert rr.compact_bits(4) == 3 and rr.compact_stride(4, 3) == 2
    # fields of row 0: 1, 3, sentinel 4 -> 1 | 3 << 3 | 4 << 6 = 0x119
    assert rr.compact_rows(a).tolist() == [[0x19, 0x01], [0x20, 0], [0x04, 0], [0x42, 0]]
    assert rr.expected_compact(a)[0].tolist() == a.tolist() and rr.expected_ef(a)[0].tolist()[3] == [0, 1, 2]
    assert rr.expected_ef(a)[1].tolist() == [2, 1, 0, 3]
    # graph B: ids of a larger graph, K = 2.  row 0: n 2, u 99, l = msb(49) = 5: 10 low bits (10 | 3 << 5), 2 + 3 + 2 high bits, bits
    # 0 + 0 and 3 + 1.  row 1: n 1, u 37, l = 5: low 5, 1 + 1 + 2 high bits, bit 1
    b = np.array([[99, 10], [37, -1]], dtype=np.int32)
    m = rr.ef_rows(b)
    assert m.l.tolist() == [5, 5] and m.low_nbits.tolist() == [10, 5] and m.high_nbits.tolist() == [7, 4]
    assert [[w.tolist() for w in m.words(i)] for i in range(2)] == [[[106], [17]], [[5], [2]]]
    assert m.size_in_bytes == 26 // 8
    # two nodes, K = 2: 2 bits, stride 1: 1 | 0 << 2; 1 | sentinel 2 << 2
    c = np.array([[1, 0], [1, -1]], dtype=np.int32)
    assert rr.compact_bits(2) == 2 and rr.compact_rows(c).tolist() == [[1], [9]]
    assert [rr.compact_bits(n) for n in (1, 2, 3, 255, 256, 4095, 4096)] == [1, 2, 2, 8, 9, 12, 13]


def test_garbage_behind_the_terminator_is_ignored():
    N, K = 300, 33
    rows = _rows("garbage_tail", N, K)
    deg = rr.row_degrees(rows)
    tail = np.arange(K)[None, :] > deg[:, None]
    assert (rows[tail] < -1).any() and (rows[tail] >= N).any() and (rows[tail] == -1).any()
    clean = np.where(tail, -1, rows)
    a, b = rr.ef_rows(rows), rr.ef_rows(clean)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("n", "l", "u", "low_nbits", "high_nbits", "low", "high"))
    assert np.array_equal(rr.compact_rows(rows), rr.compact_rows(clean))
    assert np.array_equal(rr.expected_ef(rows)[0], rr.expected_ef(clean)[0])
    assert np.array_equal(rr.expected_compact(rows)[0], clean)


@pytest.mark.parametrize("N,K", SHAPES + [(700, 20), (4097, 64)])
def test_families_keep_their_ids_inside_the_graph(N, K):
    for name in rr.FAMILIES:
        rows = _rows(name, N, K)
        deg = rr.row_degrees(rows)
        valid = np.arange(K)[None, :] < deg[:, None]
        assert (rows[valid] >= 0).all(), name
        if name != "global_ids":
            assert (rows[valid] < N).all(), name
        if name not in rr.NOT_FOR_ROC:
            srt = np.sort(np.where(valid, rows.astype(np.int64), rr.BIG + np.arange(K)[None, :]), axis=1)
            assert (srt[:, 1:] != srt[:, :-1]).all(), f"{name}: a repeated id"
    d = _rows("dups", N, K)
    if K > 1:
        assert any(len(set(r[:n])) < n for r, n in zip(d.tolist(), rr.row_degrees(d)))


@pytest.mark.parametrize("N,K", [(65, 21), (129, 64), (700, 20), (4097, 64), (4096, 43)])
def test_families_produce_what_they_are_named_for(N, K):
    # prefix: u = n - 1 < n, l = 0
    m = rr.ef_rows(_rows("prefix", N, K))
    assert (m.l == 0).all() and (m.u == m.n - 1).all() and set(m.n.tolist()) == set(range(1, min(K, N) + 1))
    # max_high: every row has 3 n + 1 high bits and its last set bit at 3 n - 2
    m = rr.ef_rows(_rows("max_high", N, K))
    assert (m.high_nbits == 3 * m.n + 1).all() and (m.n > 0).all()
    top = 3 * m.n - 2
    assert ((m.high[np.arange(N), top >> 6] >> (top & 63).astype(np.uint64)) == 1).all()  # (nothing above it either)
    if N >= 2 * K:
        assert m.n.max() == K and int(m.high_nbits.max()) == rr.record_bound(K, N - 1)[1]
    assert len(set(m.l.tolist())) > 1
    # max_low: the largest low stream a graph of N nodes can hold, up to its last bit
    m = rr.ef_rows(_rows("max_low", N, K))
    bound = rr.record_bound(K, N - 1)[0]
    assert (m.low_nbits == bound).all() and bound > 0
    assert m.low.shape[1] == (bound + 63) // 64
    lmask = (1 << m.l) - 1
    rows = _rows("max_low", N, K)
    low_ones = ((rows.astype(np.int64) & lmask[:, None]) == lmask[:, None]) | (rows < 0)
    assert (low_ones.sum(axis=1) >= K - 1).all()  # (every id but, where no u with its low bits set keeps l, the largest)
    last = bound - 1  # the stream's last bit is the top low bit of u; the bit below u's field is the top low bit of its predecessor
    assert np.array_equal((m.low[:, last >> 6] >> np.uint64(last & 63)) == 1, (m.u & lmask) == lmask)
    if (m.n >= 2).all():
        prev = (m.n - 1) * m.l - 1
        assert (((m.low[np.arange(N), prev >> 6] >> (prev & 63).astype(np.uint64)) & np.uint64(1)) == 1).all()
    # l_steps: both sides of every step
    specs = rr.l_steps_specs(N, K)
    m = rr.ef_rows(_rows("l_steps", N, K))
    have = set(zip(m.n.tolist(), m.u.tolist(), m.l.tolist()))
    if N >= len(specs):
        for n in range(1, min(K, N) + 1):
            j = 0
            while n << j <= N - 1:
                assert (n, (n << j) - 1, max(j - 1, 0)) in have and (n, n << j, j) in have, (n, j)
                j += 1
    else:  # a window of the (minus, plus) pairs: pairs stay whole
        minus = {(n, u + 1) for n, u, _ in have if (u + 1) % n == 0 and ((u + 1) // n) & ((u + 1) // n - 1) == 0}
        plus = {(n, u) for n, u, _ in have if u % n == 0 and u and (u // n) & (u // n - 1) == 0}
        assert len(minus & plus) >= N // 2 - 1
    # degrees: the sentinel in every field position
    rows = _rows("degrees", N, K)
    deg = rr.row_degrees(rows)
    assert np.array_equal(deg, np.minimum(np.arange(N) % (K + 1), N))
    if N > K:
        assert set(deg.tolist()) == set(range(K + 1))
        assert all({0, N - 1} <= set(r[:d]) for r, d in zip(rows.tolist(), deg) if d >= 2)
    # blocks: whole tiles of each kind
    deg = rr.row_degrees(_rows("blocks", N, K))
    assert (deg[:64] == min(K, N)).all()
    if N >= 128:
        assert (deg[64:128] == 0).all()
    if N >= 192:
        assert (deg[128:192:2] == K).all() and (deg[129:192:2] == 0).all()
    # runs, hub, tiny_universe, global_ids
    e, d = rr.expected_ef(_rows("runs", N, K))
    assert all((np.diff(r[:n]) == 1).all() for r, n in zip(e, d))
    e, d = rr.expected_ef(_rows("hub", N, K))
    assert len({tuple(r[:n]) for r, n in zip(e.tolist(), d)}) == 1
    t = [r[:n] for r, n in zip(*(lambda x: (x.tolist(), rr.row_degrees(x)))(_rows("tiny_universe", N, K)))]
    assert [0] in t and [1] in t and ([0, 1] in t or K == 1) and max(max(r) for r in t) <= N - 1
    if N >= 64 and K >= 64:
        assert any(sorted(r) == list(range(64)) for r in t)
    g = rr.ef_rows(_rows("global_ids", N, K))
    assert (g.n[0], g.u[0], g.l[0]) == (1, rr.TOP, 30) and g.u.max() == rr.TOP and (g.u > N).sum() > N // 2


def test_no_modelled_row_exceeds_the_documented_record():
    """low <= max over n <= K of n * msb(U // n) bits, high <= 3 n + 1 bits: for every n <= K <= 64, every universe bound U of a set
    that holds both sides of every power of two, and every u <= U on a step of l.  (This checks the model and the bound against each
    other, not the kernels.)"""
    Us = sorted({x for p in range(0, 32) for x in ((1 << p) - 1, 1 << p, (1 << p) + 1) if x <= rr.TOP} | {62, 699, 4096, 65572})
    for K in range(1, 65):
        for U in Us:
            low_bound, high_bound = rr.record_bound(K, U)
            nn = np.arange(1, K + 1, dtype=np.int64)[:, None]
            j = np.arange(32, dtype=np.int64)[None, :]
            u = np.concatenate([((nn << j) - 1).ravel(), (nn << j).ravel(), ((nn << (j + 1)) - 1).ravel(), np.full(K, U)])
            n = np.concatenate([np.repeat(nn.ravel(), 32)] * 3 + [nn.ravel()])
            keep = u <= U
            n, u = n[keep], u[keep]
            l = rr.msb(u // n)
            assert (n * l <= low_bound).all(), (K, U)
            assert (n + (u >> l) + 2 <= 3 * n + 1).all() and 3 * K + 1 == high_bound
            assert ((u >> l) < 2 * n).all() and ((u >> l) + n - 1 <= 3 * n - 2).all()  # (the last set bit)
    # and the modelled rows of every family stay inside the record of their graph
    for N, K in SHAPES + [(4097, 64)]:
        for name in rr.FAMILIES:
            m = rr.ef_rows(_rows(name, N, K))
            low_bound, _ = rr.record_bound(K, max(N - 1, int(m.u.max())))
            assert (m.low_nbits <= low_bound).all() and (m.high_nbits <= np.where(m.n > 0, 3 * m.n + 1, 0)).all(), (name, N, K)
