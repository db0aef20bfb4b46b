"""Rank inside Elias-Fano lists (vidc_ef_rank_dev) as numpy: the statement of the contract, a port of the select0 algorithm that looks
at nothing but a list's image, the designed lists of the issue, and the query set every list is asked.

  statement(lists, list_nos, ids)     ranks (np.searchsorted(..., "left") over the list's own entries, unsigned 64-bit), found, invalid:
                                      -1 / 0 for a negative list number, -1 / 0 and counted for one >= nlist
  count_range(lists, list_nos, lo, hi)  entries with lo <= id < hi; 0 for hi < lo and for skipped pairs
  Image(ids) / rank_image(im, x)      the port: m, u, l, the low and high words of lists_ref.ef_list and lists_ref.ef_directory, and
                                      csrc/ef_rank_ref.h step by step (batch_of_zero with its tie rule, select_in_word, the clamp, the
                                      bucket lower bound).  It never sees the ids.
  designed()                          name -> ids, with check_designed() asserting from the directory and the positions that every
                                      list holds what it is named for
  queries(ids)                        every entry, every entry +- 1, 0, u, u + 1, 2^32, 2^63, 2^64 - 1

An ordinary helper module: no torch, nothing from the product package.
"""
import numpy as np

import lists_ref as lr

U64 = np.uint64
M64 = (1 << 64) - 1
BATCH = lr.BATCH_BITS
EXTREMES = (0, 1 << 32, 1 << 63, M64)


# ------------------------------------------------------------------------------------------------------------------ the statement
def statement(lists, list_nos, ids):
    """-> (ranks int64[n], found uint8[n], invalid)"""
    list_nos = np.asarray(list_nos, dtype=np.int64)
    ids = lr.u64(ids)
    ranks = np.full(ids.size, -1, np.int64)
    found = np.zeros(ids.size, np.uint8)
    for ln in np.unique(list_nos[(list_nos >= 0) & (list_nos < len(lists))]).tolist():
        at = np.flatnonzero(list_nos == ln)
        li = lr.u64(lists[ln])
        r = np.searchsorted(li, ids[at], side="left")
        ranks[at] = r
        if li.size:
            found[at] = (r < li.size) & (li[np.minimum(r, li.size - 1)] == ids[at])
    return ranks, found, int((list_nos >= len(lists)).sum())


def count_range(lists, list_nos, lo, hi):
    n = len(list_nos)
    r, _, _ = statement(lists, np.concatenate([list_nos, list_nos]), np.concatenate([lr.u64(lo), lr.u64(hi)]))
    return np.maximum(r[n:] - r[:n], 0)


def has_edges(rows, u, v):
    """rows: int32 [N, K], -1 padded -> bool[n]: v[i] is an entry of row u[i]; False for u[i] outside 0 .. N-1"""
    N = rows.shape[0]
    out = np.zeros(len(u), bool)
    for i, (a, b) in enumerate(zip(np.asarray(u).tolist(), np.asarray(v).tolist())):
        if 0 <= a < N:
            out[i] = b >= 0 and b in rows[a][rows[a] >= 0].tolist()
    return out


# ----------------------------------------------------------------------------------------------------------------------- the port
class Image:
    """what the kernel sees of one non-empty list"""

    def __init__(self, ids):
        e = lr.ef_list(ids)
        self.m, self.u, self.l = e.m, e.u, e.l
        self.low = [int(w) for w in e.low] + [0]   # (the padding word of the CSR streams)
        self.high = [int(w) for w in e.high]
        self.hrank = [int(v) for v in lr.ef_directory(ids)]
        assert len(self.hrank) == (len(self.high) + 63) // 64 and self.hrank[0] == 0


def zeros_before_batch(k, hrank_k):
    return BATCH * k - hrank_k


def batch_of_zero(hrank, j):
    lo, hi = 0, len(hrank)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if zeros_before_batch(mid, hrank[mid]) <= j:
            lo = mid
        else:
            hi = mid
    return lo


def select_in_word(w, k):
    pos, s = 0, 32
    while s:
        c = bin((w >> pos) & ((1 << s) - 1)).count("1")
        if k >= c:
            k -= c
            pos += s
        s >>= 1
    return pos


def select0(im, j):
    k = batch_of_zero(im.hrank, j)
    need = j - zeros_before_batch(k, im.hrank[k])
    for wi in range(k * 64, min(k * 64 + 64, len(im.high))):
        z = ~im.high[wi] & M64
        c = bin(z).count("1")
        if need < c:
            return wi * 64 + select_in_word(z, need)
        need -= c
    return len(im.high) * 64


def low_field(im, pos):
    l = im.l
    if not l:
        return 0
    w, sh = pos >> 6, pos & 63
    v = im.low[w] >> sh if w < len(im.low) else 0
    if sh + l > 64 and w + 1 < len(im.low):
        v |= (im.low[w + 1] << (64 - sh)) & M64
    return v & ((1 << l) - 1)


def rank_image(im, x):
    """-> (rank, found) of x (a Python int below 2^64) in the list behind `im`"""
    x = int(x)
    if x > im.u:
        return im.m, 0
    h = x >> im.l
    p0 = select0(im, h - 1) + 1 if h else 0
    p1 = select0(im, h)
    r0 = min(max(p0 - h, 0), im.m)
    c = min(max(p1 - p0, 0), im.m - r0)
    if not im.l:
        return r0, int(c > 0)
    xl = x & ((1 << im.l) - 1)
    lo, hi = 0, c
    while lo < hi:
        mid = (lo + hi) >> 1
        if low_field(im, (r0 + mid) * im.l) < xl:
            lo = mid + 1
        else:
            hi = mid
    return r0 + lo, int(lo < c and low_field(im, (r0 + lo) * im.l) == xl)


# -------------------------------------------------------------------------------------------------------------------- the queries
def queries(ids):
    """uint64: every entry, every entry +- 1 (kept inside 0 .. 2^64 - 1), 0, u, u + 1, 2^32, 2^63, 2^64 - 1; no repeats"""
    x = [int(v) for v in lr.u64(ids)]
    q = set(EXTREMES)
    for v in x:
        q.update((v, max(v - 1, 0), min(v + 1, M64)))
    if x:
        q.update((x[-1], min(x[-1] + 1, M64)))
    return np.array(sorted(q), dtype=np.uint64)


# -------------------------------------------------------------------------------------------------------------- the designed lists
SIZES = (1, 2, 15, 16, 17, 63, 64, 65)  # (and the empty list, which has no image: the objects place it)


def _word_lists(rng):
    """l = 2 lists placed bit by bit (lists_ref.from_positions): position p holds a one unless it is in `zeros`.  A list of m ids whose
    high parts end in [m, 2 m): about as many zeros as ones, so runs of ones are cut where the case wants a zero."""
    out = {}

    def build(zeros, nbits):
        z = np.zeros(nbits, bool)
        z[np.asarray(sorted(zeros))] = True
        p = np.flatnonzero(~z)
        m = p.size
        h_last = int(p[-1]) - (m - 1)
        assert m <= h_last < 2 * m, (m, h_last)
        return lr.from_positions(rng, p, 2)

    # every second bit a zero, and the first 16 bits all zeros: a few more zeros than ones in front of the last one, which is what keeps
    # the last high part in [m, 2 m)
    def base(n):
        return set(range(1, n, 2)) | set(range(16))

    # a target zero on bit 63 of a word (word 1: position 127), ones around it
    z = (base(4200) - {125, 129}) | {127}
    out["zero_on_bit_63"] = build(z, 4200)
    # a target zero on bit 0 of a batch (position 4096) and on the last bit of a batch (position 4095); the bucket behind the zero at
    # 4095 starts on the first bit of batch 1 when 4096 is a one
    z = (base(9000) - {4093, 4097}) | {4096}
    z -= {4095}
    out["zero_on_bit_0_of_a_batch"] = build(z, 9000)
    z = (base(9000) - {4097}) | {4095}
    z -= {4096, 4098}
    out["zero_on_last_bit_of_a_batch"] = build(z, 9000)  # (ones at 4096, 4097, 4098: a bucket whose first entry opens batch 1)
    return out


def designed(seed=0):
    """name -> uint64 ids, ascending and non-empty"""
    rng = np.random.default_rng([seed, 40])
    d = {f"size_{n}": np.sort(rng.choice(1 << 16, n, replace=False)).astype(U64) for n in SIZES}
    d["l0_consecutive"] = np.arange(100, dtype=U64)
    d["l29_two_ids"] = lr.u64([0, 1 << 30])
    d["above_2_32"] = lr.u64([5, (1 << 32) + 7, (1 << 33) + 1, (1 << 40) + 3, (1 << 40) + 3, (1 << 45) + 9])
    d["bucket_over_batch"] = np.concatenate([np.arange(5000, dtype=U64), lr.u64([1 << 33])])
    d["dup_over_batch"] = np.concatenate([np.zeros(5000, U64), lr.u64([7])])
    d["dup_bucket_ends"] = lr.u64([3, 3, 3, 9000, 9000, 20000])
    d.update(_word_lists(rng))
    d["random_3000"] = np.sort(rng.choice(1 << 20, 3000, replace=False)).astype(U64)
    d["random_300_below_50"] = np.sort(rng.integers(0, 50, 300)).astype(U64)
    return d


def check_designed(d):
    """every designed list holds what it is named for (asserted from the model's l, positions and directory)"""
    def zeros_of(ids):
        e = lr.ef_list(ids)
        bits = np.zeros(len(e.high) * 64, bool)
        bits[e.pos] = True
        return e, np.flatnonzero(~bits[: e.high_nbits])

    assert lr.ef_list(d["l0_consecutive"]).l == 0 and lr.ef_list(d["l29_two_ids"]).l == 29
    assert lr.ef_list(d["above_2_32"]).u >= 1 << 32
    e, z = zeros_of(d["bucket_over_batch"])
    dr = lr.ef_directory(d["bucket_over_batch"])
    assert e.l == 20 and z[0] == 5000 and e.pos[4999] == 4999 and dr[1] == 4096  # bucket 0 fills batch 0 and reaches into batch 1
    assert dr.size >= 4 and np.all(dr[2:-1] == 5000)                           # whole empty batches behind it: directory ties
    assert np.array_equal(BATCH * np.arange(dr.size) - dr >= 0, np.ones(dr.size, bool))
    e, z = zeros_of(d["dup_over_batch"])
    assert e.l == 0 and z[0] == 5000 and lr.ef_directory(d["dup_over_batch"])[1] == 4096  # batch 0 holds ones only: a tie with batch 1
    e, z = zeros_of(d["dup_bucket_ends"])
    assert e.l > 0 and (d["dup_bucket_ends"][:3] >> U64(e.l)).max() == 0
    e, z = zeros_of(d["zero_on_bit_63"])
    assert e.l == 2 and 127 in z and 126 not in z and 128 not in z
    e, z = zeros_of(d["zero_on_bit_0_of_a_batch"])
    assert e.l == 2 and 4096 in z and 4095 not in z and 4097 not in z
    e, z = zeros_of(d["zero_on_last_bit_of_a_batch"])
    assert e.l == 2 and 4095 in z and not ({4096, 4097, 4098} & set(z.tolist()))  # the bucket behind it opens batch 1
    e, _ = zeros_of(d["random_3000"])
    assert len(e.high) > 64  # two batches
    for n in SIZES:
        assert d[f"size_{n}"].size == n


# ------------------------------------------------------------------------------------------------ cases for tests/ef_rank_test.cpp
def case_text(name_ids):
    """the text tests/ef_rank_test.cpp reads: per list `L m l u nlw nhw nb nq`, its low words, high words, directory, and per query
    `x rank found` as the PORT answers it"""
    out = []
    for ids in name_ids:
        im = Image(ids)
        q = queries(ids)
        out.append(f"L {im.m} {im.l} {im.u} {len(im.low)} {len(im.high)} {len(im.hrank)} {q.size}")
        out.append(" ".join(str(w) for w in im.low))
        out.append(" ".join(str(w) for w in im.high))
        out.append(" ".join(str(w) for w in im.hrank))
        for x in q:
            r, f = rank_image(im, int(x))
            out.append(f"{int(x)} {r} {f}")
    return "\n".join(out) + "\n"
