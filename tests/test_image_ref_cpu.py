"""CPU: the image model of tests/image_ref.py against the tree model of tests/wt_ref.py, and what the import's node check
(node_counts_ok) does and does not promise."""
import numpy as np
import pytest

import image_ref as ir
import wt_ref as wr

NTOTALS = (1, 63, 64, 65, 513, 2017)
NLISTS = (1, 3, 257)
#: every single-bit flip is tried up to this many image bits; beyond it a seeded sample of this many flips per level
ALL_FLIPS_MAX = 2048


def cases():
    return [(nt, nlist) for nt in NTOTALS for nlist in NLISTS]


def _sym(nt, nlist):
    return wr.family_sym("control", nt, nlist, seed=nt * 1000 + nlist)


@pytest.mark.parametrize("nt,nlist", cases())
def test_select_on_the_unpacked_image_gives_the_lists(nt, nlist):
    sym = _sym(nt, nlist)
    img = ir.wt_plain_image(sym, nlist)
    L, W = wr.n_levels(nlist), ir.words_per_level(nt)
    assert img.dtype == np.uint64 and img.size == L * W
    lv = ir.unpack_plain(img, nt, nlist)
    for a, b in zip(lv, wr.levels(sym, nlist)):
        assert np.array_equal(a, b)
    # bits at positions >= nt are zero
    if nt & 63:
        assert not np.any(img.reshape(L, W)[:, -1] >> np.uint64(nt & 63))
    off, ids = wr.lists(sym, nlist)
    pl, po = wr.all_pairs(off)
    got = np.array([wr.model_select(lv, off, nlist, int(l), int(o)) for l, o in zip(pl, po)], dtype=np.uint64)
    assert np.array_equal(got, ids)
    assert ir.node_counts_ok(lv, off, nlist)


@pytest.mark.parametrize("nt,nlist", cases())
def test_classes_and_off_bits_follow_the_levels(nt, nlist):
    sym = _sym(nt, nlist)
    cls, off_bits = ir.wt_rrr_classes(sym, nlist)
    lv = wr.levels(sym, nlist)
    L = len(lv)
    nblk, nsamp = ir.rrr_geometry(nt)
    assert cls.dtype == np.uint32 and cls.size == L * 6 * nsamp and off_bits.size == L
    ow = wr.offset_widths()
    words = cls.reshape(L, 6 * nsamp)
    for l in range(L):
        # the fields read back the way the library reads them: 6 bits at bit 6 b, LSB first, across word boundaries
        big = int.from_bytes(words[l].astype("<u4").tobytes(), "little")
        fields = np.array([(big >> (6 * b)) & 63 for b in range(nsamp * wr.RRR_SAMPLE)], dtype=np.int64)
        assert np.array_equal(fields[:nblk], ir.block_classes(lv[l]))
        assert not fields[nblk:].any()
        assert int(fields.sum()) == int(lv[l].sum())
        assert int(off_bits[l]) == int(ow[fields[:nblk]].sum())
    # the documented size of the coded tree is made of exactly these numbers
    assert wr.rrr_size(lv, nlist) == (int(off_bits.sum()) + 7) // 8 + L * ((6 * nblk + 7) // 8) + L * (nsamp + 1) * 8 + (nlist + 1) * 8


@pytest.mark.parametrize("nt,nlist", cases())
def test_a_flipped_bit_breaks_the_node_counts(nt, nlist):
    sym = _sym(nt, nlist)
    off, _ = wr.lists(sym, nlist)
    lv = wr.levels(sym, nlist)
    rng = np.random.default_rng(5)
    for level in range(len(lv)):
        where = np.arange(nt) if len(lv) * nt <= ALL_FLIPS_MAX else np.unique(
            np.concatenate([[0, nt - 1], rng.integers(0, nt, ALL_FLIPS_MAX // len(lv))]))
        for i in where:
            lv[level][i] ^= 1
            assert not ir.node_counts_ok(lv, off, nlist), (level, int(i))
            lv[level][i] ^= 1
    assert ir.node_counts_ok(lv, off, nlist)


@pytest.mark.parametrize("nt,nlist", [(65, 3), (513, 3), (2017, 257)])
def test_a_swap_inside_one_node_keeps_the_node_counts(nt, nlist):
    """What the check does not promise: two unequal bits of one node exchanged leave every boundary count as it was.  Such an image
    is walked in bounds -- and answers with other ids."""
    sym = _sym(nt, nlist)
    off, ids = wr.lists(sym, nlist)
    lv = wr.levels(sym, nlist)
    L = len(lv)
    o64 = off.astype(np.int64)
    swapped = 0
    for level in range(L):
        shn = L - level
        for p in range(1 << level):
            ns, ne = int(o64[min(p << shn, nlist)]), int(o64[min((p + 1) << shn, nlist)])
            seg = lv[level][ns:ne]
            ones, zeros = np.flatnonzero(seg == 1), np.flatnonzero(seg == 0)
            if not ones.size or not zeros.size:
                continue
            a, b = ns + int(ones[0]), ns + int(zeros[-1])
            lv[level][a], lv[level][b] = 0, 1
            assert ir.node_counts_ok(lv, off, nlist), (level, p)
            lv[level][a], lv[level][b] = 1, 0
            swapped += 1
            break
    assert swapped >= 1
