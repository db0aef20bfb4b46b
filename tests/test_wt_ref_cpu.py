"""tests/wt_ref.py checked without a GPU: the level model against brute force and the CPU oracle, the input families against what
they are meant to provoke, the two size formulas against values worked out by hand."""
import numpy as np
import pytest

import contract_ref as cr
import wt_ref as wr

SMALL = [(fam, nt, nlist) for fam in wr.FAMILIES for nt, nlist in ((1, 1), (64, 2), (130, 5), (300, 33), (257, 256))
         if not (fam in ("low_half", "high_half") and nlist < 2)] + [("deep", 300, 290), ("control", 200, 1000)]


@pytest.mark.parametrize("family,ntotal,nlist", SMALL, ids=[f"{f}-{n}-{k}" for f, n, k in SMALL])
def test_model_walk_equals_brute_force_and_the_oracle(family, ntotal, nlist, oracle):
    """every (list, offset): the bottom-up walk over the model's levels, the oracle's wt_select and the definition
    np.flatnonzero(sym == l)[o] agree; lists() is that definition in CSR form"""
    sym = wr.family_sym(family, ntotal, nlist, seed=ntotal + nlist)
    off, ids = wr.lists(sym, nlist)
    lv = wr.levels(sym, nlist)
    assert len(lv) == wr.n_levels(nlist) and all(b.size == ntotal for b in lv)
    assert int(off[-1]) == ntotal and np.array_equal(np.sort(ids), np.arange(ntotal, dtype=np.uint64))
    sym32 = sym.astype(np.uint32)
    seen = 0
    for l in range(nlist):
        members = np.flatnonzero(sym == l)
        assert members.size == int(off[l + 1] - off[l])
        for o, want in enumerate(members):
            assert wr.model_select(lv, off, nlist, l, o) == want
            assert oracle.wt_select(sym32, l, o) == want
            assert int(ids[int(off[l]) + o]) == want
            seen += 1
    assert seen == ntotal
    # the vectorised expectations against tests/contract_ref.py
    rng = np.random.default_rng(1)
    req = rng.integers(0, nlist, 7)
    flat, out_off = wr.expected_lists(off, ids, req)
    cflat, coff = cr.expected_lists("wt", off, ids, req)
    assert np.array_equal(flat, cflat) and np.array_equal(out_off, coff)
    pl, po = wr.all_pairs(off)
    ref = cr.ListRef("wt", off, ids)
    assert all(ref.item(int(a), int(b)) == int(ids[i]) for i, (a, b) in enumerate(zip(pl, po)))
    lab = np.concatenate([(pl << 32) | po, [-1, -7, nlist << 32, (nlist + 3) << 32 | 1, int(off[1] - off[0])]])
    out, invalid = wr.expected_labels(off, ids, lab)
    assert np.array_equal(out[:ntotal], ids.view(np.int64)) and np.all(out[ntotal:] == -1) and invalid == 3


def test_levels_small_case_by_hand():
    """nlist 4 (L = 2), sym = 2 0 3 1 0 2: level 0 is the top bit in id order, level 1 the low bit with the ids of lists 0, 1 in
    front of those of lists 2, 3"""
    sym = np.array([2, 0, 3, 1, 0, 2])
    lv = wr.levels(sym, 4)
    assert [b.tolist() for b in lv] == [[1, 0, 1, 0, 0, 1], [0, 1, 0, 0, 1, 0]]
    off, ids = wr.lists(sym, 4)
    assert off.tolist() == [0, 2, 3, 5, 6] and ids.tolist() == [1, 4, 3, 0, 5, 2]
    assert wr.structure_counts(sym, 4) == (0, 0, 0)


def test_families_reach_the_structures_they_are_for():
    """At 70 000 ids in 256 lists (deep: 68 537 ids in 65 537 lists) the uniform input the suite used so far has no constant RRR
    block, rank block or sample on any level; every other family has all three (deep: the first two), so a GPU test on them runs
    the class 0 / 63 branches, zero-width offsets and searches over equal directory entries.

    (class 0 / 63 blocks, constant 512-bit blocks, constant 2 016-bit spans) of this implementation:
      control (0, 0, 0)                runs (8462, 742, 116)            one_list_first (8888, 1088, 272)
      one_list_mid (8888, 1088, 272)   one_list_last (8888, 1088, 272)  low_half (1111, 136, 34)
      high_half (1111, 136, 34)        giant (8776, 982, 190)           stripes_63 (8887, 860, 214)
      stripes_512 (8709, 1087, 214)    stripes_2016 (8887, 1044, 271)   two_ends (7770, 945, 231)
      deep (1086, 132, 32)"""
    got = {}
    for fam in wr.FAMILIES:
        nt, nlist = wr.family_shape(fam, 70_000, 256)
        sym = wr.family_sym(fam, nt, nlist, seed=7)
        assert sym.size == nt and 0 <= sym.min() and sym.max() < nlist
        got[fam] = wr.structure_counts(sym, nlist)
    print(got)
    assert got["control"] == (0, 0, 0)
    for fam in wr.FAMILIES:
        if fam == "control":
            continue
        need = 2 if fam == "deep" else 3
        assert all(c >= 1 for c in got[fam][:need]), (fam, got[fam])
    nt, nlist = wr.family_shape("deep", 70_000, 256)
    assert (nt, nlist) == (68_537, 65_537) and wr.n_levels(nlist) == 17
    sizes = np.bincount(wr.family_sym("deep", nt, nlist, seed=7), minlength=nlist)
    assert np.count_nonzero(sizes == 1) > nlist // 2 and np.count_nonzero(sizes == 2) > 100 and np.count_nonzero(sizes == 0) > 100
    runs = wr.family_sym("runs", 70_000, 256, seed=7)
    assert np.all(np.diff(runs) >= 0) and np.count_nonzero(np.bincount(runs, minlength=256) == 0) >= 1


def test_sizes_by_hand():
    """plain_size / rrr_size against byte counts worked out on paper"""
    assert [wr.n_levels(n) for n in (1, 2, 3, 4, 5, 256, 257, 65536, 65537)] == [1, 1, 2, 2, 3, 8, 9, 16, 17]
    # one id, one list: L = 1.  plain: 1 word (8) + rank entries for the 2-word level: 1 block + 1 = 2 (8) + 2 starts (16)
    # RRR: one block of class 0 = no offset bits, 6 class bits -> 1 byte, 2 samples (16), 2 starts (16)
    one = np.zeros(1, np.int64)
    assert wr.plain_size(one, 1) == 8 + 8 + 16 == 32
    assert wr.rrr_size(one, 1) == 0 + 1 + 16 + 16 == 33
    # 64 ids alternating between 2 lists: L = 1.  plain: 1 word (8) + 2 rank entries (8) + 3 starts (24)
    # RRR: block 0 = 0101...0 (31 ones in 63 bits): ceil(log2 C(63, 31)) = 60 bits; block 1 = the single bit 1: C(63, 1) = 63 -> 6
    # bits; 66 bits -> 9 bytes; 2 classes -> 12 bits -> 2 bytes; 2 samples (16); 3 starts (24)
    alt = np.arange(64) % 2
    assert wr.plain_size(alt, 2) == 8 + 8 + 24 == 40
    assert wr.rrr_size(alt, 2) == 9 + 2 + 16 + 24 == 51
    # 1 000 ids, all in list 0 of 5: L = 3, every level zeros.  plain per level: 16 words (128) + rank entries for 17 words:
    # 3 blocks + 1 = 4 (16); 6 starts (48).  RRR per level: 16 blocks of class 0 -> 96 class bits = 12 bytes, 2 samples (16)
    zeros = np.zeros(1000, np.int64)
    assert wr.plain_size(zeros, 5) == 3 * (128 + 16) + 48 == 480
    assert wr.rrr_size(zeros, 5) == 3 * (12 + 16) + 48 == 132
    # 512 ids: the pad word opens a second rank block -- 8 words (64) + (2 + 1) entries (12) + 2 starts (16)
    assert wr.plain_size(np.zeros(512, np.int64), 1) == 64 + 12 + 16 == 92
    assert wr.plain_size(np.zeros(511, np.int64), 1) == 64 + 12 + 16 == 92
    assert wr.plain_size(np.zeros(448, np.int64), 1) == 56 + 8 + 16 == 80
