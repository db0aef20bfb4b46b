"""The two closed-form IVF-list containers as a plain numpy model, and the named id families the CPU and the GPU tests share.

Written from the layout comment at the top of csrc/ef.hip (succinct::elias_fano, elias_fano.hpp:22-57), not from the kernels:

  ef_list(ids)        one ascending (non-strict) list of m ids, u = its last id:  l = msb(u // m), 0 when u // m == 0;  low stream
                      m * l bits, element i's low l bits at bit i * l;  high stream (m + 1) + (u >> l) + 1 bits, bit (x_i >> l) + i
                      set for element i;  both as LSB-first 64-bit words
  ef_sizes(lists)     compressed_bytes of an object = (sum of low_nbits + high_nbits over the non-empty lists) // 8
  ef_directory(ids)   the select directory: per batch of 4096 high bits (64 high words) the number of elements before it.  The
                      library does not export its directory; the family checks use this to prove which ties and full / empty
                      batches an input holds.
  ef_chunk_stats(ids) what the single-pass encoder's 512-id chunks meet, derived from the positions p_i = (x_i >> l) + i alone: a
                      chunk owns the high words behind the word of the id before it up to the word of its own last id (a list's
                      first chunk: from word 0, its last chunk: up to the stream's last word), the directory batches likewise
                      (batch = position >> 12), and it also writes the bits of the following ids that share its last word.
  packed_list(ids, bits)   ceil(n * bits / 8) bytes, value i at bit i * bits, LSB first, little endian

FAMILIES / family(name, seed) are the named inputs: every family puts lists on one structural boundary of the encoder or of the
decoders; tests/test_lists_ref_cpu.py asserts from ef_chunk_stats / ef_directory that it does.

An ordinary helper module: no torch, no oracle, nothing from the product package.
"""
import numpy as np

CHUNK = 512          # ids per encoder chunk
BATCH_BITS = 4096    # high bits per select-directory entry
U64 = np.uint64
_1, _6, _63, _64 = U64(1), U64(6), U64(63), U64(64)


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------------------ Elias-Fano
def low_bits_for(m, u):
    """l = msb(u // m), 0 when the quotient is 0 (elias_fano.hpp:28)"""
    q = int(u) // int(m)
    return q.bit_length() - 1 if q else 0


class EfList:
    """The model of one list: m, u, l, low_nbits, high_nbits, low / high (uint64 words), pos (int64: the set high bits)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def ef_list(ids):
    x = u64(ids)
    m = int(x.size)
    assert m > 0 and (m == 1 or bool(np.all(x[1:] >= x[:-1]))), "one non-empty ascending list"
    u = int(x[-1])
    l = low_bits_for(m, u)
    low_nbits = m * l
    high_nbits = (m + 1) + (u >> l) + 1
    i = np.arange(m, dtype=np.uint64)
    pos = (x >> U64(l)) + i
    high = np.zeros((high_nbits + 63) // 64, dtype=np.uint64)
    np.bitwise_or.at(high, (pos >> _6).astype(np.int64), _1 << (pos & _63))
    low = np.zeros((low_nbits + 63) // 64 + 1, dtype=np.uint64)
    if l:
        lv = x & ((_1 << U64(l)) - _1)
        bp = i * U64(l)
        w, s = (bp >> _6).astype(np.int64), bp & _63
        np.bitwise_or.at(low, w, lv << s)
        spill = s + U64(l) > _64  # (s > 0 there)
        np.bitwise_or.at(low, w[spill] + 1, lv[spill] >> (_64 - s[spill]))
    return EfList(m=m, u=u, l=l, low_nbits=low_nbits, high_nbits=high_nbits, low=low[:-1], high=high, pos=pos.astype(np.int64))


def ef_sizes(lists):
    """-> dict(compressed_bytes, total_bits): the object's size (custom_invlists_impl.cpp:272-282)"""
    bits = 0
    for li in lists:
        if len(li):
            u, m = int(li[-1]), len(li)
            l = low_bits_for(m, u)
            bits += m * l + (m + 1) + (u >> l) + 1
    return dict(total_bits=bits, compressed_bytes=bits // 8)


def _positions(ids):
    x = u64(ids)
    l = low_bits_for(x.size, x[-1])
    pos = ((x >> U64(l)) + np.arange(x.size, dtype=np.uint64)).astype(np.int64)
    return pos, l, (x.size + 1) + (int(x[-1]) >> l) + 1


def ef_directory(ids):
    """int64[number of batches]: elements at high-bit positions below k * 4096, for every batch k of the high stream"""
    pos, _, hb = _positions(ids)
    nb = ((hb + 63) // 64 + 63) // 64
    return np.searchsorted(pos, np.arange(nb, dtype=np.int64) * BATCH_BITS, side="left").astype(np.int64)


def ef_chunk_stats(ids):
    """Per 512-id chunk: dict of int64 arrays first_word, last_word, owned_words, owned_batches, followers (ids behind the chunk
    whose bit falls into the word of the chunk's last id), last_bit (bit-in-word of the chunk's last id), n (ids of the chunk)."""
    pos, _, hb = _positions(ids)
    m = pos.size
    nw = (hb + 63) // 64
    nb = (nw + 63) // 64
    start = np.arange(0, m, CHUNK, dtype=np.int64)
    end = np.minimum(start + CHUNK, m)  # one past the chunk's last id
    last = pos[end - 1]
    before = pos[np.maximum(start - 1, 0)]
    first_word = np.where(start > 0, (before >> 6) + 1, 0)
    last_word = np.where(end == m, nw - 1, last >> 6)
    kfirst = np.where(start > 0, (before >> 12) + 1, 0)
    kend = np.where(end == m, nb, (last >> 12) + 1)
    followers = np.searchsorted(pos, ((last >> 6) + 1) << 6, side="left") - end
    return dict(first_word=first_word, last_word=last_word, owned_words=np.maximum(last_word - first_word + 1, 0),
                owned_batches=np.maximum(kend - kfirst, 0), followers=followers, last_bit=last & 63, n=end - start)


# ------------------------------------------------------------------------------------------------------------------ packed bits
def packed_list(ids, bits):
    x = u64(ids)
    if not x.size:
        return np.zeros(0, np.uint8)
    b = ((x[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & _1).astype(np.uint8)
    return np.packbits(b.reshape(-1), bitorder="little")[: (x.size * bits + 7) // 8]


def packed_patterns(n, bits, kind):
    """n values of `bits` bits that show a stray bit across a field boundary: 'ones_zeros' all-ones fields next to all-zero fields,
    'alternating' 0x55.. / 0xAA.., 'walking' a single one walking through the field"""
    i = np.arange(n, dtype=np.uint64)
    mask = U64((1 << bits) - 1)
    if kind == "ones_zeros":
        return np.where((i & _1) == 0, mask, U64(0))
    if kind == "alternating":
        return np.where((i & _1) == 0, U64(0x5555555555555555), U64(0xAAAAAAAAAAAAAAAA)) & mask
    if kind == "walking":
        return _1 << (i % U64(bits))
    raise ValueError(kind)


PACKED_PATTERNS = ("ones_zeros", "alternating", "walking")
PACKED_SIZES = (0, 1, 63, 64, 65, 511, 512, 513, 1025, 4097)


# ---------------------------------------------------------------------------------------------------------------------- labels
def all_labels(sizes, rng):
    """Faiss labels (list_no << 32 | offset) of EVERY position of the object, shuffled, mixed with the invalid kinds of
    test_gpu_device_requests.make_labels: -1, other negatives, list >= nlist, offset >= size, labels aimed at empty lists."""
    sizes = np.asarray(sizes, dtype=np.int64)
    nlist = sizes.size
    l = np.repeat(np.arange(nlist, dtype=np.int64), sizes)
    o = np.arange(l.size, dtype=np.int64) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    k = max(8, l.size // 16)
    ne = np.flatnonzero(sizes)
    pick = rng.choice(ne, k).astype(np.int64)
    empty = np.flatnonzero(sizes == 0)
    bad = [np.full(k, -1, np.int64), -rng.integers(2, 1 << 62, k),
           ((nlist + rng.integers(0, 1000, k)) << 32) | rng.integers(0, 4, k),
           (pick << 32) | (sizes[pick] + rng.integers(0, 3, k))]
    if empty.size:
        bad.append(rng.choice(empty, k).astype(np.int64) << 32)
    lab = np.concatenate([(l << 32) | o] + bad)
    return lab[rng.permutation(lab.size)]


def expect_labels(lab, sizes, flat):
    """-> (ids, -1 for every label that is not a position of the object; the number of non-negative labels among those)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    l = np.where(lab >= 0, lab >> 32, 0)
    o = lab & 0xFFFFFFFF
    valid = (lab >= 0) & (l < sizes.size)
    valid[valid] = o[valid] < sizes[l[valid]]
    out = np.full(lab.size, -1, np.int64)
    out[valid] = np.asarray(flat).view(np.int64)[off[l[valid]] + o[valid]]
    return out, int(((lab >= 0) & ~valid).sum())


# -------------------------------------------------------------------------------------------------------------------- families
FAMILIES = ("quotient_edges", "low_widths", "constant_runs", "consecutive", "head_and_outlier", "chunk_seams", "batch_seams",
            "owned_batches", "window_spans", "uniform")
QUOTIENT_M = (1, 2, 3, 63, 64, 65, 511, 512, 513, 4096, 4097)
LOW_WIDTH_SIZES = (1, 2, 65, 513)
SEAM_IDS = (511, 1023, 1535)                       # the chunk-ending ids the chunk_seams family places
SEAM_KINDS = ((63, 0), (0, 0), (0, 1), (0, 63))    # (bit-in-word of the chunk's last id, followers in that word)
OWNED_BATCHES = (0, 1, 4, 5)                       # and one chunk owning more than 64
WINDOW_SPANS = (128, 129, 256, 257)


def quotient_ks(m):
    """0, 1, 5, 20 and the largest k that keeps m * 2^k + 1 below 2^32"""
    kmax = 0
    while (m << (kmax + 1)) + 1 < (1 << 32):
        kmax += 1
    return tuple(sorted({k for k in (0, 1, 5, 20) if k <= kmax} | {kmax}))


def _with_last(rng, n, u):
    """n ascending ids (repeats allowed), the last one u, the others uniform in [0, u]"""
    rest = np.sort(rng.integers(0, int(u) + 1, n - 1, dtype=np.uint64, endpoint=False)) if n > 1 else np.zeros(0, np.uint64)
    return np.concatenate([rest, [U64(u)]]).astype(np.uint64)


def from_positions(rng, p, L):
    """The list whose high-bit positions are exactly p (strictly increasing, p_i - i ascending, p[-1] - (m - 1) in [m, 2 m) so that
    l = L): high parts h_i = p_i - i, random low bits of L bits, ascending inside every run of equal high parts."""
    p = np.asarray(p, dtype=np.int64)
    m = p.size
    h = p - np.arange(m)
    assert np.all(np.diff(h) >= 0) and h[0] >= 0
    assert L == 0 or m <= h[-1] < 2 * m, (m, int(h[-1]))
    lowbits = rng.integers(0, 1 << L, m, dtype=np.uint64) if L else np.zeros(m, np.uint64)
    return np.sort((h.astype(np.uint64) << U64(L)) | lowbits)


def _chunk_targets(m, targets, spread):
    """positions of m ids: chunk c's last id sits at targets[c] (chunks behind len(targets) are dense); inside a chunk the ids are
    consecutive with the jump in front of the last id (spread=False) or evenly spaced (spread=True)"""
    p = np.zeros(m, dtype=np.int64)
    prev = -1
    for c, a in enumerate(range(0, m, CHUNK)):
        n = min(CHUNK, m - a)
        t = targets[c] if c < len(targets) else prev + n
        assert t >= prev + n
        if spread and n > 1:
            p[a:a + n] = prev + 1 + (np.arange(n) * (t - prev - 1)) // (n - 1)
        else:
            p[a:a + n] = prev + 1 + np.arange(n)
            p[a + n - 1] = t
        prev = t
    return p


def _seam_list(s, bit, f, m):
    """l = 0 list of m ids whose id number s sits at bit `bit` of a high word, followed by exactly f ids in that same word (equal
    ids: consecutive positions), the next one in a later word; elsewhere an id repeats three times then steps by one"""
    g = np.arange(m, dtype=np.int64) // 3
    g[s:] += (bit - (s + g[s])) % 64                       # position s + g[s] lands on `bit`
    g[s + 1:s + f + 1] = g[s]                              # f equal ids behind it
    nxt = (s + g[s] - bit) + 64 - (s + f + 1)              # id s + f + 1 at the first bit of the next word, or later
    g[s + f + 1:] = np.maximum(g[s + f + 1:], nxt)
    g = np.maximum.accumulate(g)
    assert g[-1] < m  # u < m: l = 0
    return g.astype(np.uint64)


def family(name, seed=0):
    """list of uint64 arrays, every one ascending (non-strict) and non-empty:
      quotient_edges    for m in QUOTIENT_M and k in quotient_ks(m): last id m 2^k - 1, m 2^k, m 2^k + 1 (l = k - 1 | k | k; for k = 0:
                        the u < m branch | l = 0), and u = m // 2
      low_widths        every l 0..31 with ids below 2^32 (the single id 2^32 - 1 among them), every l 32..61 with wide ids, lists of
                        1, 2, 65, 513 ids wherever u = (n + 1) 2^l - 1 stays below 2^32 / 2^63
      constant_runs     n copies of v
      consecutive       base + arange(n)
      head_and_outlier  n - 1 consecutive ids and one far maximum; one small id and a dense run at the top
      chunk_seams       l = 0 lists whose ids 511 / 1023 / 1535 end their chunk at bit 63 / bit 0 of a high word with 0, 1, 63
                        followers in that word; lists of exactly 512 and 1024 ids
      batch_seams       elements at high positions 4095 and 4096 (both, either); high streams of exactly 4096, 4097, 8192, 8193 bits
      owned_batches     chunks owning exactly 0, 1, 4, 5 and more than 64 directory batches
      window_spans      chunks owning exactly 128, 129, 256, 257 high words
      uniform           rng.choice over 2^20, the control"""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    out = []
    if name == "quotient_edges":
        for m in QUOTIENT_M:
            for k in quotient_ks(m):
                for u in ((m << k) - 1, m << k, (m << k) + 1):
                    out.append(_with_last(rng, m, u))
            out.append(_with_last(rng, m, m // 2))
    elif name == "low_widths":
        for l in range(62):
            for n in LOW_WIDTH_SIZES:
                u = ((n + 1) << l) - 1
                if u < (1 << 32 if l < 32 else 1 << 63):
                    out.append(_with_last(rng, n, u))
    elif name == "constant_runs":
        for v in (0, 7):
            for n in (1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193):
                out.append(np.full(n, v, dtype=np.uint64))
    elif name == "consecutive":
        for n in (512, 513, 3000):
            for base in (0, 1, 1 << 20, (1 << 32) - n, 1 << 40):
                out.append(U64(base) + np.arange(n, dtype=np.uint64))
    elif name == "head_and_outlier":
        for n in (2, 513, 2000, 6001):
            for top in ((1 << 31) - 1, (1 << 32) - 1, 1 << 40):
                out.append(np.concatenate([np.arange(n - 1, dtype=np.uint64), [U64(top)]]))
                out.append(np.concatenate([[U64(3)], U64(top) - np.arange(n - 1, dtype=np.uint64)[::-1]]))
    elif name == "chunk_seams":
        for s in SEAM_IDS:
            for bit, f in SEAM_KINDS:
                out.append(_seam_list(s, bit, f, 1536 + 300))
        out.append(_seam_list(511, 63, 0, 512))   # FULL chunks only
        out.append(_seam_list(511, 0, 63, 1024))
        out.append(_seam_list(255, 63, 0, 256))   # (the SMALL kernels' predicate-free body takes chunks of exactly 256 ids)
        out.append(_seam_list(511, 0, 1, 768))
    elif name == "batch_seams":
        a = np.arange(2000, dtype=np.uint64)
        tail = U64(2097) + np.arange(998, dtype=np.uint64)
        out.append(np.concatenate([a, u64([2095, 2095]), tail]))  # positions 4095 and 4096
        out.append(np.concatenate([a, u64([2095, 2097]), tail]))  # 4095 and 4098
        out.append(np.concatenate([a, u64([2094, 2095]), tail]))  # 4094 and 4096
        for hb in (4096, 4097, 8192, 8193):                       # m + u + 2 high bits, l = 0
            m = (hb - 2) // 2
            out.append(_with_last(rng, m, hb - 2 - m))
    elif name == "owned_batches":
        B = BATCH_BITS
        for spread in (False, True):
            # chunk 0 ends inside batch 0 (the first chunk owns batch 0: 1), chunk 1 stays there (0), chunk 2 ends in batch 1 (1),
            # chunk 3 in batch 5 (4), chunk 4 in batch 10 (5); dense chunks behind
            out.append(from_positions(rng, _chunk_targets(20000, [511, 1023, B + 100, 5 * B + 100, 10 * B + 100], spread), 2))
        # more than 64: the first chunk of a list ends in batch 64 and owns batches 0..64.  u >> l < 2 m bounds every high stream by
        # 3 m + 2 bits, so a chunk reaches batch 64 only in a list of more than 130 816 ids.
        out.append(from_positions(rng, _chunk_targets(131500, [64 * B + 50], True), 1))
    elif name == "window_spans":
        for spread in (False, True):
            t, targets = 511, [511]
            for W in WINDOW_SPANS:  # the chunk's last id W words behind the word of the id before it
                t = ((t >> 6) + W) * 64 + int(rng.integers(0, 64))
                targets.append(t)
            out.append(from_positions(rng, _chunk_targets(24000, targets, spread), 3))
    elif name == "uniform":
        for n in (1, 2, 5, 63, 64, 65, 300, 5000, 20000):
            out.append(np.sort(rng.choice(1 << 20, size=n, replace=False)).astype(np.uint64))
    else:
        raise ValueError(name)
    return out


# --------------------------------------------------------------------------------------------------------------------- objects
# The encoder picks its kernel per OBJECT (csrc/ef_plan.h, ef_chunk_form), so the families are dealt into objects by list length:
OBJECTS = ("short", "half", "full_q", "full_runs", "full_seams", "full_big")
ROUTES = ("host", "dev", "wide", "unsorted")
NARROW = 1 << 32
WIDE_EXTRA = u64([7, 1 << 32, (1 << 45) + 3])


def _is_narrow(li):
    return int(li[-1]) < NARROW


def base_lists(name, seed=0):
    """the non-empty narrow (every id below 2^32) lists of an object:
      short       every list of at most 256 ids, of every family
      half        the lists of at most 600 ids of quotient_edges and low_widths, the chunk_seams lists of at most 1024 ids
      full_q      quotient_edges, m = 4096 and 4097            full_runs   constant_runs, consecutive, head_and_outlier, uniform: above 256 ids
      full_seams  chunk_seams, batch_seams, window_spans, the two 20 000-id lists of owned_batches
      full_big    the owned_batches list with a chunk of more than 64 batches, and one uniform list"""
    fam = {f: [li for li in family(f, seed) if _is_narrow(li)] for f in FAMILIES}
    if name == "short":
        return [li for f in FAMILIES for li in fam[f] if li.size <= 256]
    if name == "half":
        return ([li for f in ("quotient_edges", "low_widths") for li in fam[f] if li.size <= 600]
                + [li for li in fam["chunk_seams"] if li.size <= 1024])
    if name == "full_q":
        return [li for li in fam["quotient_edges"] if li.size > 600]
    if name == "full_runs":
        return [li for f in ("constant_runs", "consecutive", "head_and_outlier", "uniform") for li in fam[f] if li.size > 256]
    if name == "full_seams":
        return fam["chunk_seams"] + fam["batch_seams"] + fam["window_spans"] + fam["owned_batches"][:2]
    if name == "full_big":
        return [fam["owned_batches"][2], fam["uniform"][-2]]
    raise ValueError(name)


def wide_lists(name, seed=0):
    """the lists with an id of 2^32 or more that the `wide` route adds behind an object's own"""
    wide = [li for f in FAMILIES for li in family(f, seed) if not _is_narrow(li)]
    if name == "short":
        return [li for li in wide if li.size <= 256]
    if name == "half":
        return [li for li in wide if 256 < li.size <= 600]
    if name == "full_runs":
        return [li for li in wide if li.size > 600]
    return [WIDE_EXTRA]


def object_lists(name, route, seed=0):
    """-> (lists, nbase): the object's own lists with an empty list in front, behind every seventh list and at the end -- the first
    nbase entries, the same under every route -- and behind them what the route adds: `wide` lists with an id of 2^32 or more,
    `unsorted` one list that is not ascending (`host` / `dev`: nothing; they differ in where the offsets live)."""
    lists = [np.zeros(0, np.uint64)]
    for i, li in enumerate(base_lists(name, seed)):
        lists.append(li)
        if i % 7 == 6:
            lists.append(np.zeros(0, np.uint64))
    lists.append(np.zeros(0, np.uint64))
    nbase = len(lists)
    if route == "wide":
        lists += wide_lists(name, seed)
    elif route == "unsorted":
        rng = np.random.default_rng([seed, 77])
        src = family("uniform", seed)[5 if name == "short" else 6]  # 65 / 300 ids
        perm = rng.permutation(src)
        assert np.any(perm[1:] < perm[:-1])
        lists.append(perm)
    elif route not in ("host", "dev"):
        raise ValueError(route)
    return lists, nbase


def encoder_form(lists):
    """which chunk kernel the single-pass encoder runs for an object of these lists (csrc/ef_plan.h: ef_chunk_form, and
    tests/test_ef_plan_cpu.py holds this restatement against it; the device-offset route takes the k_ef_lowhigh32_dev form of
    the same name): 'general' (some list not ascending: the three-pass path for the whole object),
    'wide' (some id of 2^32 or more: k_ef_lowhigh), 'short' (no list above 256 ids: k_ef_lowhigh32<4, SMALL>), 'half' (ntotal <
    256 * nchunks: <8, SMALL>), 'full' (<8>)"""
    ne = [u64(li) for li in lists if len(li)]
    if any(np.any(li[1:] < li[:-1]) for li in ne):
        return "general"
    if any(int(li[-1]) >= NARROW for li in ne):
        return "wide"
    nchunks = sum((li.size + CHUNK - 1) // CHUNK for li in ne)
    ntotal = sum(li.size for li in ne)
    if max(li.size for li in ne) <= 256:
        return "short"
    return "half" if ntotal < 256 * nchunks else "full"


def offsets_of(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(li) for li in lists])
    return off


def concat(lists):
    return np.concatenate([u64(li) for li in lists]) if lists else np.zeros(0, np.uint64)
