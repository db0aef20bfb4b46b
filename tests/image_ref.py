"""The flat images of a wavelet tree (include/vidc.h, vidc_wt_export_all / vidc_wt_import) as a numpy model, built on wt_ref.py.

  wt_plain_image     the wt_type 0 image: L * ceil(nt / 64) little-endian words, level after level
  wt_rrr_classes     the wt_type 1 class words (6 bits per 63-bit block, whole samples of 32 blocks per level) and off_bits
  unpack_plain       the level bit vectors back out of a plain image
  node_counts_ok     the rule an import checks an image by: at every node boundary of every level, the ones in front of it are what
                     the offsets alone demand

The offsets of the RRR blocks are the library's own combinatorial rank: nothing outside it pins them, so they are not modelled here
(the GPU tests check them by round trip).  An ordinary helper module: it imports neither torch nor the product package.
"""
import numpy as np

import wt_ref as wr


def words_per_level(nt):
    return (nt + 63) // 64


def wt_plain_image(sym, nlist):
    """uint64[L * W]: bit i of level l is bit i & 63 of word l * W + (i >> 6); bits at positions >= nt are zero.  Takes sym or the
    result of wt_ref.levels()."""
    lv = sym if isinstance(sym, list) else wr.levels(sym, nlist)
    W = words_per_level(lv[0].size)
    out = np.zeros((len(lv), W * 8), dtype=np.uint8)
    for l, bits in enumerate(lv):
        b = np.packbits(bits, bitorder="little")
        out[l, : b.size] = b
    return out.reshape(-1).view("<u8").astype(np.uint64)


def unpack_plain(image, nt, nlist):
    """-> the L uint8 bit vectors of a plain image"""
    L, W = wr.n_levels(nlist), words_per_level(nt)
    by = np.ascontiguousarray(np.asarray(image, dtype="<u8")).view(np.uint8).reshape(L, W * 8)
    return [np.unpackbits(by[l], bitorder="little")[:nt].copy() for l in range(L)]


def rrr_geometry(nt):
    nblk = (nt + wr.RRR_BLOCK - 1) // wr.RRR_BLOCK
    return nblk, (nblk + wr.RRR_SAMPLE - 1) // wr.RRR_SAMPLE


def block_classes(bits):
    """popcount of every 63-bit block of one level (the last block may be short)"""
    nblk, _ = rrr_geometry(bits.size)
    padded = np.zeros(nblk * wr.RRR_BLOCK, dtype=np.int64)
    padded[: bits.size] = bits
    return padded.reshape(nblk, wr.RRR_BLOCK).sum(1)


def wt_rrr_classes(sym, nlist):
    """-> (uint32[L * 6 * nsamp] class words, uint64[L] off_bits): the class of block b of a level is the 6 bits at bit 6 b of the
    level's words, LSB first; class fields of blocks >= nblk are zero; off_bits[l] = sum of ceil(log2 C(63, class)).  Takes sym or
    the result of wt_ref.levels()."""
    lv = sym if isinstance(sym, list) else wr.levels(sym, nlist)
    nblk, nsamp = rrr_geometry(lv[0].size)
    ow = wr.offset_widths()
    words = np.zeros((len(lv), 6 * nsamp), dtype=np.uint32)
    off_bits = np.zeros(len(lv), dtype=np.uint64)
    sh = np.arange(6, dtype=np.int64)
    for l, bits in enumerate(lv):
        cls = block_classes(bits)
        off_bits[l] = int(ow[cls].sum())
        fields = np.zeros(nsamp * wr.RRR_SAMPLE, dtype=np.int64)
        fields[:nblk] = cls
        fb = ((fields[:, None] >> sh) & 1).astype(np.uint8).reshape(-1)
        if fb.size:
            words[l] = np.packbits(fb, bitorder="little").view("<u4")
    return words.reshape(-1), off_bits


def node_rank_table(offsets, nlist, level):
    """ones in front of node boundary p = 0 .. 2^level of a level, from the offsets alone: the sizes of the right children of the
    nodes in front of p"""
    L = wr.n_levels(nlist)
    off = np.asarray(offsets).astype(np.int64)
    shn = L - level
    p = np.arange(1 << level, dtype=np.int64)
    mid = off[np.minimum((2 * p + 1) << (shn - 1), nlist)]
    hi = off[np.minimum((p + 1) << shn, nlist)]
    return np.concatenate([[0], np.cumsum(hi - mid)])


def node_counts_ok(levels, offsets, nlist):
    """For every level l and node boundary p = 0 .. 2^l: the ones of levels[l] in front of position offsets[min(p << (L - l), nlist)]
    equal node_rank_table.  Equal counts at both ends of every node mean every node holds exactly as many ones as its right child
    has elements: what a select / decode walk relies on to stay inside its node.  (It does not say WHICH positions hold them.)"""
    L = wr.n_levels(nlist)
    off = np.asarray(offsets).astype(np.int64)
    assert len(levels) == L
    for level in range(L):
        shn = L - level
        p = np.arange((1 << level) + 1, dtype=np.int64)
        pos = off[np.minimum(p << shn, nlist)]
        before = np.concatenate([[0], np.cumsum(np.asarray(levels[level], dtype=np.int64))])
        if not np.array_equal(before[pos], node_rank_table(off, nlist, level)):
            return False
    return True
