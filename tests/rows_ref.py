"""The two closed-form graph-row containers as a plain numpy model, and the named row families the CPU and the GPU tests share.

A graph is `rows`: int32 [N, K], row i = the neighbours of node i, ended by the first -1 (entries behind it are never looked at).

  row_degrees                 entries before the first -1
  ef_rows                     EliasFanoNSGGraph (altid_impl.cpp:53-90, elias_fano.hpp:22-57): per row u = the largest id, taken before
                              the sort; the ids sorted; l = msb(u // n), 0 when u // n == 0; low stream n * l bits, l bits per element,
                              LSB first; high stream n + (u >> l) + 2 bits, bit (x >> l) + e set for element e; an empty row has no
                              stream; object size = sum(low_nbits + high_nbits) // 8
  compact_bits / compact_rows CompactBitNSGGraph (altid_impl.cpp:20-51): bits = the smallest b with 2^b >= N + 1, stride =
                              ceil(K * bits / 8); the fields of a row are its neighbours in input order, then the sentinel N if the
                              degree is below K, then zeros; fields are `bits` wide, LSB first
  expected_compact / expected_ef   what decode_rows must answer: input order / ascending, -1 behind the degree, and the degrees
  record_bound                the documented bound of one Elias-Fano record, for the property check
  FAMILIES / family           the named inputs

It is an ordinary helper module: no torch, no oracle, nothing from the product package.  (ROC rows have no closed form: their
expectation is the pinned oracle's roc_decode(roc_encode(row)), taken in the tests.)
"""
import numpy as np

BIG = np.int64(1) << 40  # sorts behind every id


def _rows64(rows):
    rows = np.asarray(rows)
    assert rows.ndim == 2
    return rows.astype(np.int64)


def row_degrees(rows):
    """int64[N]: the number of entries before the first -1 (K for a row without one)"""
    rows = np.asarray(rows)
    end = rows == -1
    return np.where(end.any(axis=1), end.argmax(axis=1), rows.shape[1]).astype(np.int64)


def msb(q):
    """floor(log2(q)) of an int64 array, 0 where q == 0 (values below 2^53: the float64 exponent is exact)"""
    q = np.asarray(q, dtype=np.int64)
    return np.where(q > 0, np.frexp(np.maximum(q, 1).astype(np.float64))[1] - 1, 0).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ Elias-Fano
class EfRows:
    """The model of one graph: per row n, l, u, low_nbits, high_nbits and the stream words (row i: low[i, :ceil(low_nbits / 64)],
    high[i, :ceil(high_nbits / 64)]; words behind them are zero)."""

    def __init__(self, n, l, u, low_nbits, high_nbits, low, high):
        self.n, self.l, self.u, self.low_nbits, self.high_nbits, self.low, self.high = n, l, u, low_nbits, high_nbits, low, high

    def words(self, i):
        return self.low[i, : (int(self.low_nbits[i]) + 63) // 64], self.high[i, : (int(self.high_nbits[i]) + 63) // 64]

    @property
    def size_in_bytes(self):
        return int(self.low_nbits.sum() + self.high_nbits.sum()) // 8


def ef_rows(rows):
    rows = _rows64(rows)
    N, K = rows.shape
    n = row_degrees(rows)
    valid = np.arange(K)[None, :] < n[:, None]
    u = np.where(valid, rows, 0).max(axis=1, initial=0)
    srt = np.sort(np.where(valid, rows, BIG), axis=1)
    l = msb(u // np.maximum(n, 1))
    low_nbits = n * l
    high_nbits = np.where(n > 0, n + (u >> l) + 2, 0)
    low = np.zeros((N, int((low_nbits.max(initial=0) + 63) // 64) + 1), dtype=np.uint64)
    high = np.zeros((N, int((high_nbits.max(initial=0) + 63) // 64) + 1), dtype=np.uint64)
    lu = l.astype(np.uint64)
    one = np.uint64(1)
    for e in range(K):
        on = np.flatnonzero(n > e)
        if not on.size:
            break
        x = srt[on, e].astype(np.uint64)
        le = lu[on]
        lv = x & ((one << le) - one)
        bp = np.uint64(e) * le
        w, s = (bp >> np.uint64(6)).astype(np.int64), bp & np.uint64(63)
        low[on, w] |= lv << s
        spill = s + le > np.uint64(64)  # (s > 0 there)
        low[on[spill], w[spill] + 1] |= lv[spill] >> (np.uint64(64) - s[spill])
        hp = (x >> le) + np.uint64(e)
        high[on, (hp >> np.uint64(6)).astype(np.int64)] |= one << (hp & np.uint64(63))
    return EfRows(n, l, u, low_nbits, high_nbits, low[:, :-1], high[:, :-1])


def record_bound(K, U):
    """(low bits, high bits) no row of at most K ids <= U exceeds: max over n <= K of n * msb(U // n), and 3 K + 1"""
    nn = np.arange(1, K + 1, dtype=np.int64)
    return int((nn * msb(U // nn)).max()), 3 * K + 1


def expected_ef(rows):
    """-> (int32 [N, K] ascending, -1 behind the degree; degrees)"""
    rows = _rows64(rows)
    n = row_degrees(rows)
    valid = np.arange(rows.shape[1])[None, :] < n[:, None]
    srt = np.sort(np.where(valid, rows, BIG), axis=1)
    return np.where(valid, srt, -1).astype(np.int32), n


# --------------------------------------------------------------------------------------------------------------- compact bits
def compact_bits(N):
    b = 0
    while (1 << b) < N + 1:
        b += 1
    return b


def compact_stride(N, K):
    return (K * compact_bits(N) + 7) // 8


def compact_rows(rows, N=None):
    """uint8 [N, stride]: the byte image of every row"""
    rows = _rows64(rows)
    N = rows.shape[0] if N is None else N
    K = rows.shape[1]
    bits, stride = compact_bits(N), compact_stride(N, K)
    n = row_degrees(rows)
    col = np.arange(K)[None, :]
    fields = np.where(col < n[:, None], rows, np.where(col == n[:, None], N, 0)).astype(np.uint32)
    out = np.zeros((rows.shape[0], stride), dtype=np.uint8)
    sh = np.arange(bits, dtype=np.uint32)
    for a in range(0, rows.shape[0], 4096):
        f = fields[a:a + 4096]
        b = ((f[:, :, None] >> sh) & np.uint32(1)).astype(np.uint8).reshape(f.shape[0], K * bits)
        out[a:a + 4096] = np.packbits(b, axis=1, bitorder="little")[:, :stride]
    return out


def expected_compact(rows):
    """-> (int32 [N, K] in input order, -1 behind the degree; degrees)"""
    rows = _rows64(rows)
    n = row_degrees(rows)
    return np.where(np.arange(rows.shape[1])[None, :] < n[:, None], rows, -1).astype(np.int32), n


# ------------------------------------------------------------------------------------------------------------------- families
FAMILIES = ("uniform", "prefix", "l_steps", "max_high", "max_low", "runs", "hub", "degrees", "blocks", "garbage_tail", "dups",
            "tiny_universe", "global_ids")
#: the families whose every row sits on a boundary of the Elias-Fano geometry
BOUNDARY = ("prefix", "l_steps", "max_high", "max_low")
NOT_FOR_ROC = ("dups",)  # ROC codes sets
NOT_FOR_COMPACT = ("global_ids",)  # compact bits stores ids below N
TOP = (1 << 31) - 1


def _from_lists(lists, N, K, start=0):
    """rows: row i = lists[(start + i) % len(lists)]"""
    rows = np.full((N, K), -1, dtype=np.int32)
    for i in range(N):
        li = lists[(start + i) % len(lists)]
        rows[i, : len(li)] = li
    return rows


def _distinct(rng, R, K, universe, deg):
    """R rows of distinct uniform ids below `universe` in random order; row i has min(deg[i], its number of distinct draws) ids"""
    if universe <= 4 * K:  # a random permutation of the universe per row
        vals = np.full((R, K), -1, dtype=np.int64)
        w = min(K, universe)
        vals[:, :w] = np.argsort(rng.random((R, universe)), axis=1)[:, :w]
        have = np.full(R, w)
    else:  # 3 K + 8 draws, the distinct ones in random order
        M = 3 * K + 8
        cand = np.sort(rng.integers(0, universe, (R, M)), axis=1)
        dup = np.zeros((R, M), dtype=bool)
        dup[:, 1:] = cand[:, 1:] == cand[:, :-1]
        keys = rng.random((R, M))
        keys[dup] = 2.0
        vals = np.take_along_axis(cand, np.argsort(keys, axis=1), axis=1)[:, :K]
        have = np.minimum(K, M - dup.sum(axis=1))
    deg = np.minimum(np.asarray(deg), have)
    return np.where(np.arange(K)[None, :] < deg[:, None], vals, -1).astype(np.int32)


def _with_max(rng, n, u):
    """n distinct ids, the largest one u, the others random below it, in random order (u >= n - 1)"""
    if n == 1:
        return np.array([u], dtype=np.int64)
    if u <= 4096:
        rest = rng.choice(u, n - 1, replace=False)
    else:
        rest = rng.permutation(np.unique(rng.integers(0, u, 4 * n)))[: n - 1]
        assert rest.size == n - 1
    return rng.permutation(np.concatenate([rest, [u]]))


def l_steps_specs(N, K):
    """(n, u) of the l_steps family, pairs (n * 2^j - 1, n * 2^j) adjacent: l = j - 1 | j (for j = 0: the u < n branch | l = 0)"""
    out = []
    for n in range(1, min(K, N) + 1):
        j = 0
        while n << j <= N - 1:
            out += [(n, (n << j) - 1), (n, n << j)]
            j += 1
    return out or [(1, 0)]


def max_high_specs(N, K):
    """(n, l) with u = n * 2^(l + 1) - 1 <= N - 1: first the largest l of every n (n descending), then the others"""
    first, rest = [], []
    for n in range(min(K, N), 0, -1):
        ls = [l for l in range(31) if (n << (l + 1)) - 1 <= N - 1]
        if ls:
            first.append((n, ls[-1]))
            rest += [(n, l) for l in ls[:-1]]
    return first + rest


def max_low_n(N, K):
    """the degrees n <= min(K, N) at which n * msb((N - 1) // n) is largest, and that largest bit count"""
    nn = np.arange(1, min(K, N) + 1, dtype=np.int64)
    b = nn * msb((N - 1) // nn)
    return nn[b == b.max()], int(b.max())


def family(name, N, K, seed=0, nrows=None):
    """rows (int32 [N, K]; nrows: only that many rows of a graph of N nodes) of a named family; every id lies in [0, N) unless the
    name says otherwise:
      uniform        distinct uniform ids, uniform degrees: the baseline
      prefix         ids {0 .. n-1} in random order: u = n - 1 < n, the l = 0 branch
      l_steps        for every degree n, u = n * 2^j - 1 and u = n * 2^j for every j that fits: both sides of every step of l
      max_high       u = n * 2^(l+1) - 1, the other ids at 0 .. n-2 / at u-n+1 .. u-1: 3 n + 1 high bits, last set bit 3 n - 2
      max_low        n at the argmax of n * msb((N-1) / n), u as large as N allows, every id with its l low bits all ones (u itself
                     too wherever that keeps l)
      runs           consecutive ids from a random base, ascending or descending
      hub            every row holds the same neighbour set, in its own order
      degrees        row i has degree i mod (K+1) (at most N: the ids are distinct); ids 0, N-1, alternating-bit patterns first
      blocks         tiles of 64 rows: full rows, empty rows, full and empty rows alternating, ...
      garbage_tail   uniform rows; behind the terminator random values: negatives other than -1, values >= N, further -1s
      dups           repeated ids inside a row, every degree
      tiny_universe  distinct ids from {0 .. 3} (every subset in every rotation) and n ids from {0 .. n}
      global_ids     ids up to 2^31 - 1 in a graph of N nodes, a one-edge row [2^31 - 1] among them"""
    rng = np.random.default_rng([seed, N, K, FAMILIES.index(name)])
    R = N if nrows is None else nrows
    Kn = min(K, N)  # the most distinct ids a row can hold
    col = np.arange(K)[None, :]
    if name == "uniform":
        return _distinct(rng, R, K, N, rng.integers(0, K + 1, R))
    if name == "prefix":
        return _from_lists([rng.permutation(n) for n in range(1, Kn + 1)], R, K)
    if name == "l_steps":
        specs = l_steps_specs(N, K)
        start = 2 * int(rng.integers(0, len(specs) // 2 + 1)) if R < len(specs) else 0
        return _from_lists([_with_max(rng, n, u) for n, u in specs], R, K, start)
    if name == "max_high":
        lists = []
        for n, l in max_high_specs(N, K):
            u = (n << (l + 1)) - 1
            lists.append(rng.permutation(np.concatenate([np.arange(n - 1), [u]])))
            lists.append(rng.permutation(np.arange(u - n + 1, u + 1)))
        return _from_lists(lists or [[0]], R, K)
    if name == "max_low":
        ns, _ = max_low_n(N, K)
        lists = []
        for n in ns:
            n = int(n)
            l = int(msb((N - 1) // n))
            hmax = N // (1 << l) - 1  # the largest h with (h + 1) * 2^l - 1 <= N - 1
            top = ((hmax + 1) << l) - 1
            for kind in range(3):
                if int(msb(top // n)) == l:
                    u, pool = top, hmax  # u has its low bits set too; the others have h < hmax
                else:
                    u, pool = N - 1, hmax + 1
                h = (np.arange(n - 1), np.arange(pool - n + 1, pool), rng.choice(pool, n - 1, replace=False))[kind]
                lists.append(rng.permutation(np.concatenate([((h + 1) << l) - 1, [u]])))
        return _from_lists(lists, R, K)
    if name == "runs":
        d = rng.integers(0, Kn + 1, R)
        base = (rng.random(R) * (N - d + 1)).astype(np.int64)
        ids = base[:, None] + np.where((rng.random(R) < 0.5)[:, None], col, d[:, None] - 1 - col)
        return np.where(col < d[:, None], ids, -1).astype(np.int32)
    if name == "hub":
        hub = rng.choice(N, max(1, (3 * Kn) // 4), replace=False)
        return _from_lists([rng.permutation(hub) for _ in range(min(R, 97))], R, K)
    if name == "degrees":
        pat = [0, N - 1] + [p >> s for s in range(32) for p in (0x55555555, 0xAAAAAAAA)]
        pat = [p for p in dict.fromkeys(pat) if 0 <= p < N]
        lists = []
        for i in range(R):
            d = min(i % (K + 1), N)
            ids = pat[:d]
            if len(ids) < d:
                more = rng.permutation(N)[: 2 * K + len(pat)] if N <= 4096 else rng.integers(0, N, 4 * K)
                ids = list(dict.fromkeys(ids + [int(x) for x in more]))[:d]
            lists.append(rng.permutation(np.array(ids, dtype=np.int64)))
        return _from_lists(lists, R, K)
    if name == "blocks":
        full = _distinct(rng, R, K, N, np.full(R, K))
        i = np.arange(R)
        kind = (i // 64) % 3  # 0: full rows, 1: empty rows, 2: alternating
        empty = (kind == 1) | ((kind == 2) & (i % 2 == 1))
        return np.where(empty[:, None], -1, full).astype(np.int32)
    if name == "garbage_tail":
        rows = _distinct(rng, R, K, N, rng.integers(0, K, R)).astype(np.int64)
        d = row_degrees(rows)
        junk = rng.choice(np.array([-2, -(1 << 31), -7, -1, N, N + 1, TOP, 0, 1]), (R, K))
        junk = np.where(rng.random((R, K)) < 0.5, junk, rng.integers(-(1 << 31), 1 << 31, (R, K)))
        return np.where(col > d[:, None], junk, rows).astype(np.int32)
    if name == "dups":
        d = (K - np.arange(R)) % (K + 1)
        rng.shuffle(d)
        pool = rng.integers(0, N, max(2, K // 3))
        ids = pool[rng.integers(0, pool.size, (R, K))]
        ids[::5] = ids[::5, :1]  # one id, K times over
        return np.where(col < d[:, None], ids, -1).astype(np.int32)
    if name == "tiny_universe":
        t = min(4, N)
        lists = [[0], [1], [0, 1], [1, 0]] if N >= 2 else [[0]]
        for m in range(1, 1 << t):
            s = [b for b in range(t) if m >> b & 1]
            lists += [s[r:] + s[:r] for r in range(len(s))]
        for n in range(1, min(K, N - 1) + 1):  # n of the n + 1 ids {0 .. n}, each one left out in turn for small n
            for out in ([n // 2] if n > 6 else range(n + 1)):
                lists.append(rng.permutation([x for x in range(n + 1) if x != out]))
        if N >= 64 and K >= 64:
            lists.append(rng.permutation(64))  # all of 2^6
        return _from_lists([li[:K] for li in lists], R, K)
    if name == "global_ids":
        rows = _distinct(rng, R, K, 1 << 31, rng.integers(0, K + 1, R))
        special = [[TOP], rng.permutation(np.concatenate([[TOP], np.arange(K - 1)])), [TOP - 1, TOP][:K], [1 << 30], [0],
                   rng.permutation(TOP - np.arange(K))]
        for i, li in enumerate(special[:R]):
            rows[i] = -1
            rows[i, : len(li)] = li
        return rows
    raise ValueError(name)
