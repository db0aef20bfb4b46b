"""The wavelet tree of csrc/wt.hip as a plain numpy model, stated without the library.

The codec's only input is the symbol sequence sym[id] = the list of id `id` (ids 0 .. ntotal - 1, every list ascending), given to it
as the CSR (offsets, ids) with ids = the stable argsort of sym.  sdsl is absent from the reference tree, so nothing outside this
repository pins the tree's internal layout: this module does.  It gives

  lists / levels / model_select        the definition of select and the L level bit vectors of the pointerless layout
  plain_size / rrr_size                the two documented byte counts, recomputed from those bit vectors
  structure_counts                     how many constant RRR blocks, rank blocks and samples an input produces
  FAMILIES / family_shape / family_sym the named inputs the CPU and the GPU tests share
  expected_lists / expected_labels     what decode_lists / translate_labels must answer (tests/contract_ref.py semantics, vectorised)

It is an ordinary helper module: it imports neither torch nor the product package.
"""
import math

import numpy as np

RRR_BLOCK = 63  # bits per RRR block
RRR_SAMPLE = 32  # blocks per sample: one sample per 2 016 bits
RANK_BLOCK = 512  # bits per rank-directory block of the plain coding
SAMPLE_BITS = RRR_BLOCK * RRR_SAMPLE


def n_levels(nlist):
    """L = max(1, bit_width(nlist - 1))"""
    return max(1, int(nlist - 1).bit_length())


def lists(sym, nlist):
    """-> (offsets uint64[nlist + 1], ids uint64[ntotal]): ids[offsets[l] + o] is the definition of select(l, o)"""
    sym = np.asarray(sym, dtype=np.int64)
    assert sym.ndim == 1 and (sym.size == 0 or (0 <= int(sym.min()) and int(sym.max()) < nlist))
    counts = np.bincount(sym, minlength=nlist)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return off, np.argsort(sym, kind="stable").astype(np.uint64)


def levels(sym, nlist):
    """-> L uint8 arrays of ntotal bits.  Level l holds bit L - 1 - l of every symbol, in the order obtained by stable-sorting the
    ids on the top l bits of their symbol."""
    sym = np.asarray(sym, dtype=np.int64)
    L = n_levels(nlist)
    out = []
    for level in range(L):
        order = np.argsort(sym >> (L - level), kind="stable")
        out.append(((sym[order] >> (L - 1 - level)) & 1).astype(np.uint8))
    return out


def model_select(lv, offsets, nlist, l, o):
    """The id at offset o of list l, by walking the level bit vectors bottom-up: at every level the (o+1)-th bit of the symbol's
    value inside the symbol's node, nothing else."""
    L = len(lv)
    off = np.asarray(offsets).astype(np.int64)
    pos = int(o)
    for level in range(L - 1, -1, -1):
        sh = L - level
        p = l >> sh
        ns, ne = int(off[min(p << sh, nlist)]), int(off[min((p + 1) << sh, nlist)])
        bit = (l >> (L - 1 - level)) & 1
        pos = int(np.flatnonzero(lv[level][ns:ne] == bit)[pos])
    return pos


def _levels_of(sym_or_levels, nlist):
    if isinstance(sym_or_levels, list):
        return sym_or_levels
    return levels(sym_or_levels, nlist)


def plain_size(sym_or_levels, nlist):
    """Bytes of the wt_type 0 tree (csrc/wt.hip): per level the ceil(nt / 64) words of the bit vector and one 4-byte rank entry per
    512-bit block of the level as it is stored -- with its pad word: ceil(nt / 64) + 1 words -- plus the entry behind the last
    block; then the (nlist + 1) symbol start positions, 8 bytes each.  Takes sym or the result of levels()."""
    total = (nlist + 1) * 8
    for bits in _levels_of(sym_or_levels, nlist):
        words = -(-bits.size // 64)
        rank_blocks = -(-(words + 1) * 64 // RANK_BLOCK)
        total += words * 8 + (rank_blocks + 1) * 4
    return total


def offset_widths():
    """ceil(log2 C(63, c)) for c = 0 .. 63"""
    return np.array([0 if c in (0, RRR_BLOCK) else math.ceil(math.log2(math.comb(RRR_BLOCK, c))) for c in range(RRR_BLOCK + 1)],
                    dtype=np.int64)


def rrr_size(sym_or_levels, nlist):
    """Bytes of a levelwise wavelet tree whose levels are RRR coded with 63-bit blocks and one sample per 32 blocks:
    6-bit class + ceil(log2 C(63, class)) offset bits per block, (32-bit stream pointer + 32-bit rank) per sample
    (+ the final one), plus the table of symbol start positions (csrc/wt.hip).  Takes sym or the result of levels()."""
    lv = _levels_of(sym_or_levels, nlist)
    L = len(lv)
    nt = lv[0].size
    ow = offset_widths()
    nblk = (nt + 62) // 63
    nsamp = (nblk + 31) // 32
    off_bits = 0
    for bits in lv:
        padded = np.zeros(nblk * 63, dtype=np.int64)
        padded[:nt] = bits
        cls = padded.reshape(nblk, 63).sum(1)
        off_bits += int(ow[cls].sum())
    return (off_bits + 7) // 8 + L * ((6 * nblk + 7) // 8) + L * (nsamp + 1) * 8 + (nlist + 1) * 8


def _constant_spans(bits, span):
    """full spans of `span` bits that are all zeros or all ones"""
    n = bits.size // span
    s = bits[: n * span].reshape(n, span).sum(1, dtype=np.int64)
    return int(np.count_nonzero((s == 0) | (s == span)))


def structure_counts(sym_or_levels, nlist):
    """-> (RRR blocks of class 0 or 63, constant 512-bit rank blocks, constant 2 016-bit sample spans), summed over the levels;
    whole blocks / spans only."""
    lv = _levels_of(sym_or_levels, nlist)
    return tuple(sum(_constant_spans(b, span) for b in lv) for span in (RRR_BLOCK, RANK_BLOCK, SAMPLE_BITS))


# ----------------------------------------------------------------------------------------------------------- input families
DEEP_NLIST = 65537  # L = 17
DEEP_NTOTAL = DEEP_NLIST + 3000
FAMILIES = ("control", "runs", "one_list_first", "one_list_mid", "one_list_last", "low_half", "high_half", "giant", "stripes_63",
            "stripes_512", "stripes_2016", "two_ends", "deep")


def family_shape(family, ntotal, nlist):
    """(ntotal, nlist) the family is built at: `deep` brings its own list count and, at full size, its own id count"""
    if family == "deep" and ntotal > 10000:
        return DEEP_NTOTAL, DEEP_NLIST
    return ntotal, nlist


def family_sym(family, ntotal, nlist, seed=0):
    """sym[id] (int64[ntotal], values < nlist) of a named input family:
      control        uniform random: every level close to a fair coin
      runs           sorted: every list a contiguous id range, a few empty lists among them
      one_list_*     every id in list 0 / nlist // 2 / nlist - 1
      low_half / high_half  random over the lists below / from 2^(L-1): the top level is all zeros / all ones (nlist >= 2)
      giant          every 700th id in a random list, the rest in list nlist - 1
      stripes_P      (id // P) % min(3, nlist): bit flips on the edges of RRR blocks (63), rank blocks (512), samples (2 016)
      two_ends       ids alternate between list 0 and list nlist - 1
      deep           (almost) as many lists as ids: most lists hold one id, some two, some none"""
    rng = np.random.default_rng(seed)
    ids = np.arange(ntotal, dtype=np.int64)
    L = n_levels(nlist)
    if family == "control":
        sym = rng.integers(0, nlist, ntotal)
    elif family == "runs":
        w = rng.random(nlist) + 0.05
        if nlist >= 3:
            w[rng.choice(nlist, max(1, nlist // 8), replace=False)] = 0.0
        sym = np.repeat(np.arange(nlist), rng.multinomial(ntotal, w / w.sum()))
    elif family.startswith("one_list_"):
        k = {"first": 0, "mid": nlist // 2, "last": nlist - 1}[family[len("one_list_"):]]
        sym = np.full(ntotal, k)
    elif family == "low_half":
        assert nlist >= 2
        sym = rng.integers(0, 1 << (L - 1), ntotal)
    elif family == "high_half":
        assert nlist >= 2
        sym = rng.integers(1 << (L - 1), nlist, ntotal)
    elif family == "giant":
        sym = np.where(ids % 700 == 699, rng.integers(0, nlist, ntotal), nlist - 1)
    elif family.startswith("stripes_"):
        sym = (ids // int(family[len("stripes_"):])) % min(3, nlist)
    elif family == "two_ends":
        sym = np.where(ids % 2 == 0, 0, nlist - 1)
    elif family == "deep":
        once = min(ntotal, nlist - nlist // 20)
        sym = np.concatenate([rng.permutation(nlist)[:once], rng.integers(0, nlist, ntotal - once)])
        rng.shuffle(sym)
    else:
        raise ValueError(family)
    sym = np.asarray(sym, dtype=np.int64)
    assert sym.size == ntotal
    return sym


# ------------------------------------------------------------------------------------------------------------ expected answers
def expected_lists(offsets, ids, list_nos):
    """-> (uint64[total], uint64 out_offsets[m + 1]): the requested lists back to back (contract_ref.expected_lists("wt", ...)
    without its loop over the lists; the lists of a wavelet tree are ascending as they come)"""
    off = np.asarray(offsets).astype(np.int64)
    ln = np.asarray(list_nos).astype(np.int64).reshape(-1)
    sizes = off[ln + 1] - off[ln]
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src = np.repeat(off[ln] - out_off[:-1], sizes) + np.arange(int(out_off[-1]), dtype=np.int64)
    return np.asarray(ids, dtype=np.uint64)[src], out_off.astype(np.uint64)


def all_pairs(offsets):
    """(list, offset) of every position of the object, in object order"""
    off = np.asarray(offsets).astype(np.int64)
    sizes = off[1:] - off[:-1]
    l = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    return l, np.arange(int(off[-1]), dtype=np.int64) - off[l]


def expected_labels(offsets, ids, labels):
    """-> (int64 ids, invalid): a label list << 32 | offset gives that id; a negative label gives -1 and is not counted; a label
    whose list is >= nlist or whose offset is >= the list's size gives -1 and is counted"""
    off = np.asarray(offsets).astype(np.int64)
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    nlist = off.size - 1
    sizes = off[1:] - off[:-1]
    l = np.where(lab >= 0, lab >> 32, 0)
    o = lab & 0xFFFFFFFF
    valid = (lab >= 0) & (l < nlist)
    valid[valid] = o[valid] < sizes[l[valid]]
    out = np.full(lab.size, -1, np.int64)
    out[valid] = np.asarray(ids, dtype=np.uint64).view(np.int64)[off[l[valid]] + o[valid]]
    return out, int(np.count_nonzero((lab >= 0) & ~valid))
