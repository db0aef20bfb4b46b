"""The wavelet tree (csrc/wt.hip) against the numpy model of tests/wt_ref.py on the inputs that reach what uniform random lists never
do: RRR blocks of class 0 and 63 (no offset bits), constant 512-bit rank blocks and constant samples (directory searches over equal
entries), id counts on the edges of the word, the RRR block, the rank block, the sample, the decode tile and the build tile, level
counts on both sides of every power of two, the threshold of the partitioned scatter, a pool full of 0xFF, and appends.

Every comparison is between integers and exact.  check_tree asks every entry point for every position of the object; the model
gives the level count, both sizes and every id (tests/test_wt_ref_cpu.py checks the model itself, and that the families below do
produce the structures they are named for)."""
import numpy as np
import pytest

import append_ref as ar
import wt_ref as wr

pytestmark = pytest.mark.gpu

#: above this many ids check_tree replaces the one select call over every (list, offset) by 50 000 random selects; decode_all,
#: decode_lists of every list and translate_labels of every pair still cover every position
EXHAUSTIVE_SELECT_MAX = 1 << 16


def _torch():
    import torch

    return torch


def _wt():
    from vector_db_id_compression_amd.codecs import WaveletTreeLists

    return WaveletTreeLists


def _ctx():
    from vector_db_id_compression_amd import _lib

    return _lib.default_context()


def dev(a):
    """uint64 / int64 numpy -> int64 CUDA tensor"""
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64)).cuda()


def build(off, ids, wt_type, dev_offsets=False):
    return _wt().build(dev(off) if dev_offsets else off, dev(ids), wt_type=wt_type)


class Requests:
    """The questions check_tree asks one input, and the model's answers: drawn once, asked of every build of that input."""

    def __init__(self, off, ids, nlist, seed=0):
        rng = np.random.default_rng(seed)
        self.off, self.ids, self.nlist = off, ids, nlist
        nt = ids.size
        sizes = (off[1:] - off[:-1]).astype(np.int64)
        nonempty, empty = np.flatnonzero(sizes), np.flatnonzero(sizes == 0)
        longest = int(np.argmax(sizes))
        # select: every (list, offset) of the object in one call, or a sample of them (EXHAUSTIVE_SELECT_MAX)
        self.sel_l, self.sel_o = wr.all_pairs(off)
        self.sel_want = ids.view(np.int64)
        self.exhaustive = nt <= EXHAUSTIVE_SELECT_MAX
        if not self.exhaustive:
            pick = rng.integers(0, nt, 50_000)
            self.sel_l, self.sel_o, self.sel_want = self.sel_l[pick], self.sel_o[pick], self.sel_want[pick]
        # decode_lists: every non-empty list in shuffled order, a few empty lists and one repeat mixed in
        req = np.concatenate([nonempty, empty[:3], nonempty[:1]])
        self.req = req[rng.permutation(req.size)].astype(np.uint64)
        self.req_flat, self.req_off = wr.expected_lists(off, ids, self.req)
        # translate_labels: every valid pair, -1, lists >= nlist, an offset equal to its list's size, a label into an empty list
        pl, po = wr.all_pairs(off)
        odd = [-1, -(1 << 40), nlist << 32, ((nlist + 5) << 32) | 3, (longest << 32) | int(sizes[longest])]
        odd += [int(e) << 32 for e in empty[:2]]
        lab = np.concatenate([(pl << 32) | po, np.array(odd, dtype=np.int64)])
        self.labels = lab[rng.permutation(lab.size)]
        self.lab_want, self.lab_invalid = wr.expected_labels(off, ids, self.labels)
        assert self.lab_invalid == len(odd) - 2 and np.count_nonzero(self.lab_want >= 0) == nt
        # decode_gather: a few hundred items over the longest list and some others; the longest list's first and last id among them
        self.g_lists = np.concatenate([[longest], rng.choice(nonempty, min(30, nonempty.size))]).astype(np.uint64)
        gs = sizes[self.g_lists.astype(np.int64)]
        slot = np.concatenate([[0, 0], rng.integers(0, self.g_lists.size, 300)])
        self.g_slot = slot.astype(np.uint64)
        self.g_off = np.concatenate([[0, gs[0] - 1], (rng.random(300) * gs[slot[2:]]).astype(np.int64)]).astype(np.uint64)
        self.g_want = ids.view(np.int64)[off[self.g_lists[slot].astype(np.int64)].astype(np.int64) + self.g_off.astype(np.int64)]

    def ask(self, wt, what):
        """every entry point of `wt`, each compared with the model -> the answers (for comparing builds with each other)"""
        torch = _torch()
        ids64 = self.ids.view(np.int64)
        dec = wt.decode_all().cpu().numpy()
        assert np.array_equal(dec, ids64), f"{what}: decode_all {_first_diff(dec, ids64)}"
        sel = wt.select(self.sel_l, self.sel_o)
        assert np.array_equal(sel, self.sel_want), f"{what}: select {_first_diff(sel, self.sel_want, self.sel_l, self.sel_o)}"
        flat, out_off = wt.decode_lists(self.req)
        flat = flat.cpu().numpy()
        assert np.array_equal(out_off, self.req_off), f"{what}: decode_lists offsets"
        assert np.array_equal(flat.view(np.uint64), self.req_flat), f"{what}: decode_lists {_first_diff(flat, self.req_flat.view(np.int64))}"
        inv = torch.zeros(1, dtype=torch.int64, device="cuda")
        tr = wt.translate_labels(dev(self.labels), invalid=inv).cpu().numpy()
        assert np.array_equal(tr, self.lab_want), f"{what}: translate_labels {_first_diff(tr, self.lab_want)}"
        assert int(inv.item()) == self.lab_invalid, f"{what}: invalid labels counted"
        gat = wt.decode_gather(self.g_lists, self.g_slot, self.g_off)
        assert np.array_equal(gat, self.g_want), f"{what}: decode_gather {_first_diff(gat, self.g_want)}"
        return dict(size=wt.size_in_bytes, levels=wt.levels, decode_all=dec, select=sel, lists=flat, labels=tr, gather=gat)


def _first_diff(got, want, *coords):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if not bad.size:
        return f"sizes {np.asarray(got).shape} / {np.asarray(want).shape}"
    i = int(bad[0])
    at = f", (list, offset) = ({int(coords[0][i])}, {int(coords[1][i])})" if coords else ""
    return f"{bad.size} of {np.asarray(want).size} differ, first at {i}{at}: got {got[i]}, expected {want[i]}"


def same_answers(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def check_tree(sym, nlist, what="", builds=((0, False), (0, True), (1, False), (1, True))):
    """Build the tree of sym for every (wt_type, device offsets?) of `builds`; levels, size and the answer of every entry point for
    every position must be the model's, and equal between the wt_types (all but the size) and the offset sources
    -> {wt_type: answers}"""
    off, ids = wr.lists(sym, nlist)
    lv = wr.levels(sym, nlist)
    want_size = {0: wr.plain_size(lv, nlist), 1: wr.rrr_size(lv, nlist)}
    rq = Requests(off, ids, nlist, seed=int(ids.size) + nlist)
    out = {}
    for wt_type, dev_offsets in builds:
        tag = f"{what} wt_type {wt_type}, {'device' if dev_offsets else 'host'} offsets"
        wt = build(off, ids, wt_type, dev_offsets)
        assert wt.levels == len(lv), f"{tag}: levels"
        assert wt.size_in_bytes == want_size[wt_type], f"{tag}: size_in_bytes {wt.size_in_bytes}, model {want_size[wt_type]}"
        assert np.array_equal(wt.offsets, off), f"{tag}: offsets"
        ans = rq.ask(wt, tag)
        del wt
        if wt_type in out:
            same_answers(out[wt_type], ans, tag)
        out[wt_type] = ans
    if 0 in out and 1 in out:
        same_answers({k: v for k, v in out[0].items() if k != "size"}, {k: v for k, v in out[1].items() if k != "size"},
                     f"{what}: wt_type 0 against wt_type 1")
    return out


# ------------------------------------------------------------------------------------------- a. structural boundaries of ntotal
EDGES = [1, 2, 62, 63, 64, 65, 511, 512, 513, 2015, 2016, 2017, 8191, 8192, 8193, 16383, 16384, 16385, 32769]


@pytest.mark.parametrize("ntotal", EDGES)
@pytest.mark.parametrize("family", ["runs", "one_list_first", "one_list_last", "two_ends"])
def test_id_counts_on_structural_boundaries(family, ntotal):
    """one id either side of the 64-bit word, the 63-bit RRR block, the 512-bit rank block, the 2 016-bit sample, the 8 192-position
    decode tile and the 16 384-position build tile; 32 769 = the first chained scan over three tiles.  33 lists (L = 6)."""
    check_tree(wr.family_sym(family, ntotal, 33, seed=ntotal), 33, f"{family} {ntotal}")


# ---------------------------------------------------------------------------------------------------- b. every family at 70 000
@pytest.mark.parametrize("family", wr.FAMILIES)
def test_every_family_at_70000(family):
    """70 000 ids in 256 lists (deep: 68 537 ids in 65 537 lists, L = 17): the constant blocks and samples counted in
    tests/test_wt_ref_cpu.py, every position asked"""
    nt, nlist = wr.family_shape(family, 70_000, 256)
    check_tree(wr.family_sym(family, nt, nlist, seed=7), nlist, family)


# -------------------------------------------------------------------------------------------------- c. level-count boundaries
@pytest.mark.parametrize("nlist", [1, 2, 3, 4, 5, 255, 256, 257, 65_536, 65_537])
@pytest.mark.parametrize("family", ["control", "runs"])
def test_level_count_boundaries(family, nlist):
    """L = 1, 1, 2, 2, 3, 8, 8, 9, 16, 17 at 5 000 ids: lists that do not fill the last node of a level, more lists than ids"""
    out = check_tree(wr.family_sym(family, 5000, nlist, seed=nlist), nlist, f"{family} nlist {nlist}")
    assert out[0]["levels"] == {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 255: 8, 256: 8, 257: 9, 65_536: 16, 65_537: 17}[nlist]


# ------------------------------------------------------------------------------------------------------ d. the scatter threshold
@pytest.mark.parametrize("ntotal", [262_143, 262_144, 262_145])
@pytest.mark.parametrize("family", ["runs", "one_list_mid", "giant"])
def test_scatter_threshold(family, ntotal, monkeypatch):
    """From 2^18 ids on, list_nos[id] is built by the partitioned scatter, below by the direct one; VIDC_WT_SCATTER=1 forces the
    direct one.  Both must build the model's tree: same size, same answers.  (Above 2^16 ids the select call asks 50 000 random
    (list, offset) pairs instead of all; decode_all, decode_lists of every list and translate_labels of every pair still reach
    every position.)"""
    sym = wr.family_sym(family, ntotal, 700, seed=ntotal)
    monkeypatch.delenv("VIDC_WT_SCATTER", raising=False)
    out = check_tree(sym, 700, f"{family} {ntotal}")
    monkeypatch.setenv("VIDC_WT_SCATTER", "1")
    direct = check_tree(sym, 700, f"{family} {ntotal} direct scatter", builds=((0, False), (1, True)))
    monkeypatch.delenv("VIDC_WT_SCATTER")
    for wt_type in (0, 1):
        same_answers(out[wt_type], direct[wt_type], f"{family} {ntotal}: partitioned against direct scatter, wt_type {wt_type}")


def test_more_lists_than_the_partitioned_scatter_takes():
    """2^18 ids in 2^18 + 1 lists: one list too many for the partitioned scatter, so the direct scatter builds a 19-level tree"""
    nlist = (1 << 18) + 1
    out = check_tree(wr.family_sym("control", 1 << 18, nlist, seed=18), nlist, "control 2^18 ids, 2^18 + 1 lists")
    assert out[0]["levels"] == 19


# ------------------------------------------------------------------------------------------------------------ e. poisoned pool
@pytest.mark.parametrize("family", ["one_list_mid", "stripes_63"])
def test_poisoned_pool(family):
    """Every cached device block is 0xFF when it is handed out: a class-0 / class-63 block has no offset bits, a constant level no
    offset stream at all -- nothing read for them may depend on what the memory held.  Size and answers as from the clean pool."""
    sym = wr.family_sym(family, 70_000, 256, seed=7)
    ctx = _ctx()
    ctx.set_pool_poison(False)
    clean = check_tree(sym, 256, f"{family} clean")
    ctx.set_pool_poison(True)
    try:
        dirty = check_tree(sym, 256, f"{family} poisoned")
        again = check_tree(sym, 256, f"{family} poisoned again")  # (blocks released by the first poisoned pass, poisoned again)
    finally:
        ctx.set_pool_poison(False)
    for wt_type in (0, 1):
        same_answers(clean[wt_type], dirty[wt_type], f"{family} wt_type {wt_type}: poisoned pool")
        same_answers(clean[wt_type], again[wt_type], f"{family} wt_type {wt_type}: poisoned pool, second pass")


# -------------------------------------------------------------------------------------------------------------------- f. append
@pytest.mark.parametrize("wt_type", [0, 1])
@pytest.mark.parametrize("ntotal", [2015, 16_380])
@pytest.mark.parametrize("family", ["one_list_mid", "runs"])
def test_append_onto_constant_levels(family, ntotal, wt_type):
    """A small batch (ids ntotal .. in add order, so every list stays ascending and the whole a permutation) onto a tree of constant
    blocks, across a sample edge (2 016) and a build-tile edge (16 384): the result is the tree `build` makes of the merged lists --
    size, decode_all, every select -- which is the model's."""
    nlist, n = 33, 12
    rng = np.random.default_rng(ntotal)
    sym = wr.family_sym(family, ntotal, nlist, seed=ntotal)
    off, ids = wr.lists(sym, nlist)
    ln = rng.integers(0, nlist, n).astype(np.int64)
    ln[:3] = int(sym[0])  # (the one list / the first run grows too)
    ln[5], ln[7] = -1, nlist  # skipped; the second one counted
    valid = (ln >= 0) & (ln < nlist)
    add = (ntotal + np.cumsum(valid) - 1).astype(np.uint64)
    sym2 = np.concatenate([sym, ln[valid]])
    off2, ids2 = wr.lists(sym2, nlist)
    m = ar.merge(off, ids, ln, add)
    assert np.array_equal(m.offsets, off2) and np.array_equal(m.ids, ids2) and m.invalid == 1
    lv2 = wr.levels(sym2, nlist)
    old = build(off, ids, wt_type)
    inv = _torch().zeros(1, dtype=_torch().int64, device="cuda")
    new, lab = old.append(dev(ln), dev(add), invalid=inv)
    ref = build(off2, ids2, wt_type)
    assert int(inv.item()) == 1
    assert np.array_equal(lab.cpu().numpy(), ar.labels("wt", m))
    want_size = wr.plain_size(lv2, nlist) if wt_type == 0 else wr.rrr_size(lv2, nlist)
    assert new.size_in_bytes == ref.size_in_bytes == want_size and new.levels == ref.levels == len(lv2)
    assert np.array_equal(new.offsets, off2)
    pl, po = wr.all_pairs(off2)
    for obj, name in ((new, "appended"), (ref, "built from the merged lists")):
        assert np.array_equal(obj.decode_all().cpu().numpy().view(np.uint64), ids2), name
        assert np.array_equal(obj.select(pl, po), ids2.view(np.int64)), name
    assert np.array_equal(old.decode_all().cpu().numpy().view(np.uint64), ids), "the old object changed"
