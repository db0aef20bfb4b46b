"""CPU: the numpy model of tests/churn_ref.py against a brute-force double loop, and the designed schedules against what they claim to
contain.  The second part is a condition on the inputs of tests/test_gpu_churn.py, checked here without a GPU: a chain that never
crosses a seam, never widens the packed container or never meets a skipped pair would pass for the wrong reason."""
import numpy as np
import pytest

import churn_ref as ch
from test_gpu_remove import SEAM_SIZES


# ------------------------------------------------------------------------------------------------------------------- the model
def brute_add(lists, ln, ids):
    out = [list(li) for li in lists]
    for l, v in zip(ln, ids):
        if l >= 0:
            out[l].append(v)
    return out


def brute_remove(lists, ln, ids):
    """-> (lists, removed, missing, invalid): every entry against every pair"""
    nlist = len(lists)
    out, removed = [], 0
    hit = [False] * len(ids)
    for l, li in enumerate(lists):
        keep = []
        for v in li:
            gone = False
            for i, w in enumerate(ids):
                if v == w and (ln is None or ln[i] == l):
                    gone = hit[i] = True
            if gone:
                removed += 1
            else:
                keep.append(v)
        out.append(keep)
    valid = [ln is None or 0 <= ln[i] < nlist for i in range(len(ids))]
    missing = sum(1 for i in range(len(ids)) if valid[i] and not hit[i])
    invalid = 0 if ln is None else sum(1 for l in ln if l >= nlist)
    return out, removed, missing, invalid


def brute_find(lists, ln, ids):
    out = []
    for i, w in enumerate(ids):
        at = -1
        for l, li in enumerate(lists):
            if at < 0 and (ln is None or ln[i] == l):
                for v in li:
                    if v == w:
                        at = l
        out.append(at)
    return out


@pytest.mark.parametrize("seed", range(6))
def test_model_against_a_double_loop(seed):
    rng = np.random.default_rng(seed)
    nlist = 5
    lists = [rng.choice(40, int(rng.integers(0, 12)), replace=False).astype(np.uint64) for _ in range(nlist)]  # ids shared between lists
    m = ch.Model(lists)
    want = [list(li) for li in lists]
    for step in range(8):
        n = int(rng.integers(0, 9))
        ids = rng.integers(0, 60, n).astype(np.uint64)
        if step % 3 == 0:
            ln = rng.integers(-2, nlist, n)
            ids = (100 * (step + 1) + np.arange(n)).astype(np.uint64)
            touched = m.add(ln, ids)
            want = brute_add(want, ln, ids)
            assert touched == sorted({int(l) for l in ln if l >= 0})
        else:
            ln = None if step % 3 == 1 else rng.integers(-2, nlist + 2, n)
            before = [len(li) for li in want]
            c = m.remove(ln, ids)
            want, removed, missing, invalid = brute_remove(want, ln, ids)
            assert (c.removed, c.missing, c.invalid) == (removed, missing, invalid)
            assert c.touched == [l for l in range(nlist) if len(want[l]) != before[l]]
        assert [li.tolist() for li in m.lists] == [[int(v) for v in li] for li in want]
        probe = rng.integers(0, 60, 20).astype(np.uint64)
        pl = rng.integers(0, nlist, 20)
        assert m.find(None, probe).tolist() == brute_find(want, None, probe)
        assert m.find(pl, probe).tolist() == brute_find(want, pl, probe)
        assert np.array_equal(m.offsets(), np.concatenate([[0], np.cumsum([len(li) for li in want])]))


def test_code_is_the_golden_ratio_product():
    ids = np.array([0, 1, 2, 16_000, (1 << 31) - 1], np.uint64)
    want = [(int(i) * ch.GOLDEN) % (1 << 64) for i in ids]
    assert ch.code(ids).view(np.uint64).tolist() == want
    assert ch.code(ids.view(np.int64)).view(np.uint64).tolist() == want
    # neighbouring ids differ in every byte
    a, b = ch.code(np.arange(5000, dtype=np.uint64)).view(np.uint8).reshape(-1, 8), ch.code(np.arange(1, 5001, dtype=np.uint64)).view(np.uint8).reshape(-1, 8)
    assert (a != b).all()


# ---------------------------------------------------------------------------------------------------------------- the schedules
def replay(scheme):
    """-> (initial lists, steps, the model's lists behind every step)"""
    init, steps = ch.schedule(scheme)
    m = ch.Model(init)
    states = []
    for st in steps:
        if st.kind == "add":
            assert m.add(st.list_nos, st.ids) == st.touched
        elif st.kind == "remove":
            c = m.remove(st.list_nos, st.ids)
            assert (c.removed, c.missing, c.invalid, c.touched) == (st.expect.removed, st.expect.missing, st.expect.invalid, st.touched)
        assert np.array_equal(m.sizes(), st.sizes)
        states.append([li.copy() for li in m.lists])
    return init, steps, states


@pytest.fixture(scope="module", params=ch.SCHEMES)
def chain(request):
    return (request.param,) + replay(request.param)


def sizes_of(states, l):
    return [int(s[l].size) for s in states]


def test_shape_of_the_chain(chain):
    scheme, init, steps, states = chain
    assert len(init) == ch.NLIST == 16 and tuple(li.size for li in init) == ch.INIT_SIZES and sum(ch.INIT_SIZES) == 16_000
    assert len(steps) == (12 if scheme != "perm" else 8)
    assert [st.name for st in steps if st.kind != "remove"] == ["fresh", "seams_up", "add_600", "every_list", "one_list", "empty", "add_800", "last"]
    if scheme != "perm":
        assert [st.name for st in steps] == ["fresh", "seams_up", "remove_500", "seams_down", "add_600", "every_list", "precision_down",
                                             "one_list", "empty", "remove_any", "add_800", "last"]
        assert steps[ch.S_REMOVE_500].list_nos is not None and steps[ch.S_SEAMS_DOWN].list_nos is None
    assert max(int(st.sizes.sum()) for st in steps) <= 25_000
    for s in states:
        for li in s:
            assert li.size < 65_536 and (li.size == 0 or int(li.max()) < (1 << 31))
            assert np.unique(li).size == li.size, "ids are distinct inside every list"


def test_ids(chain):
    scheme, init, steps, states = chain
    every = np.concatenate(init + [st.ids[st.list_nos >= 0] for st in steps if st.kind == "add"])
    dups = 0 if scheme == "perm" else 2
    assert np.unique(every).size == every.size - dups, "an id is handed out once"
    if scheme == "sparse":
        for s in states:
            for li in s:
                if li.size:
                    top = int(li.max())
                    assert top & (top - 1), "a list's largest id is a power of two"
    else:  # the packed container takes ids below ntotal, an append ids below the number ever handed out; the tree a permutation
        assert int(np.concatenate(init).max()) < 16_000
        handed = 16_000
        for st in steps:
            if st.kind == "add":
                v = st.ids[st.list_nos >= 0]
                assert np.array_equal(v, handed + np.arange(v.size))
                handed += v.size
        if scheme == "perm":
            assert np.array_equal(np.sort(np.concatenate(states[-1])), np.arange(handed))
            for li in init:
                assert (np.diff(li.astype(np.int64)) > 0).all()


def test_seams(chain):
    """63 -> 65 -> 63, 1023 -> 1025 -> 1023, 4090 -> 4100 -> 4090 (the seams of test_gpu_remove.SEAM_SIZES), 2040 -> 2060 -> 2040"""
    scheme, init, steps, states = chain
    assert {63, 65, 1023, 1025, 4100} <= set(SEAM_SIZES.tolist())
    for l, seam, lo, hi in ((ch.L_64, 64, 63, 65), (ch.L_1024, 1024, 1023, 1025), (ch.L_2048, 2048, 2040, 2060),
                            (ch.L_WIDE, 4096, 4090, 4100), (ch.L_NARROW, 4096, 4090, 4100)):
        sz = sizes_of(states, l)
        assert sz[0] == lo and sz[1] == hi and lo < seam < hi
        if scheme != "perm":
            assert sz[ch.S_SEAMS_DOWN] == lo
            # old and new entries leave alike
            gone = np.setdiff1d(states[ch.S_SEAMS_UP][l], states[ch.S_SEAMS_DOWN][l])
            assert np.isin(gone, init[l]).any() and (~np.isin(gone, init[l])).any()


def test_the_20_bit_chain_launch(chain):
    scheme, init, steps, states = chain
    if scheme != "sparse":
        return
    for s in states[:ch.S_SEAMS_DOWN + 1]:
        assert int(s[ch.L_WIDE].max()).bit_length() in (19, 20)
        assert int(s[ch.L_NARROW].max()).bit_length() < 19


def test_empty_and_small_lists(chain):
    scheme, init, steps, states = chain
    assert init[ch.L_STARTS_EMPTY].size == 0 and states[-1][ch.L_STARTS_EMPTY].size > 0
    if scheme == "perm":
        return
    sz = sizes_of(states, ch.L_REFILL)
    assert sz[ch.S_SEAMS_DOWN - 1] == 300 and sz[ch.S_SEAMS_DOWN] == 0 and sz[ch.S_SEAMS_DOWN + 1] == 0 and sz[ch.S_SEAMS_DOWN + 2] == 300
    sz = sizes_of(states, ch.L_ONE)
    assert sz[ch.S_REMOVE_500 - 1] == 1 and sz[ch.S_REMOVE_500] == 0


def test_precision(chain):
    scheme, init, steps, states = chain
    if scheme != "sparse":
        return
    tops = [int(s[ch.L_PREC].max()) for s in states]
    before, down, up = tops[ch.S_PRECISION_DOWN - 1], tops[ch.S_PRECISION_DOWN], tops[ch.S_ONE_LIST]
    assert down.bit_length() < before.bit_length(), "the removal takes the largest id and its leading bit"
    assert up > (1 << down.bit_length()), "the append passes the next power of two"
    assert steps[ch.S_ONE_LIST].touched == [ch.L_PREC]


def test_packed_width(chain):
    """16 000 ids (14 bits); 500 leave; 600 come, so that the ids ever handed out pass 16 384 while ntotal stays below"""
    scheme, init, steps, states = chain
    if scheme != "dense":
        return
    assert steps[ch.S_REMOVE_500].expect.removed == 500
    handed = 16_000
    for i, st in enumerate(steps):
        if st.kind == "add":
            handed += int((st.list_nos >= 0).sum())
        ntotal = int(st.sizes.sum())
        if i < ch.S_ADD_600:
            assert handed <= 16_384
        if i == ch.S_ADD_600:
            assert int((st.list_nos >= 0).sum()) == 600 and handed > 16_384 > ntotal
    assert steps[ch.S_ADD_600 + 2].kind == "remove", "a removal behind the widening append"


def test_duplicates(chain):
    scheme, init, steps, states = chain
    if scheme == "perm":
        return
    both = np.intersect1d(init[ch.L_DUP_A], init[ch.L_DUP_B])
    assert both.size == 2
    d1, d2 = init[ch.L_DUP_A][10], init[ch.L_DUP_A][40]
    assert set(both.tolist()) == {int(d1), int(d2)}
    st = steps[ch.S_SEAMS_DOWN]  # any-list mode: both copies
    assert st.list_nos is None and d1 in st.ids
    assert d1 not in states[ch.S_SEAMS_DOWN][ch.L_DUP_A] and d1 not in states[ch.S_SEAMS_DOWN][ch.L_DUP_B]
    st = steps[ch.S_PRECISION_DOWN]  # by pair: the named list only
    assert ((st.list_nos == ch.L_DUP_A) & (st.ids == d2)).sum() == 1 and not ((st.list_nos == ch.L_DUP_B) & (st.ids == d2)).any()
    assert d2 not in states[ch.S_PRECISION_DOWN][ch.L_DUP_A] and d2 in states[ch.S_PRECISION_DOWN][ch.L_DUP_B]
    assert d2 in states[ch.S_PRECISION_DOWN - 1][ch.L_DUP_A]


def test_skipped_pairs(chain):
    scheme, init, steps, states = chain
    adds = [st for st in steps if st.kind == "add"]
    assert any((st.list_nos < 0).any() for st in adds)
    if scheme == "perm":
        return
    for i in (ch.S_REMOVE_500, ch.S_PRECISION_DOWN):
        st, before = steps[i], ch.Model(states[i - 1])
        ln, ids = st.list_nos, st.ids
        assert (ln < 0).sum() >= 2 and st.expect.invalid == 0
        held = before.find(None, ids)
        assert ((ln < 0) & (held >= 0)).any(), "a negative list number with a present id"
        assert ((ln >= 0) & (held < 0)).any(), "an absent id"
        assert ((ln >= 0) & (held >= 0) & (before.find(ln, ids) < 0)).any(), "a present id under the wrong list"
        key = ln * (1 << 32) + ids.astype(np.int64)
        assert np.unique(key[ln >= 0]).size < int((ln >= 0).sum()), "a repeated pair"
        assert st.expect.missing == 2
        # (the ids under negative list numbers stay)
        for l, v in zip(ln, ids):
            if l < 0 and before.find(None, [v])[0] >= 0:
                assert ch.Model(states[i]).find(None, [v])[0] >= 0
    for i in (ch.S_SEAMS_DOWN, ch.S_REMOVE_ANY):
        assert steps[i].expect.missing >= 1
    st = steps[ch.S_REMOVE_ANY]
    assert np.unique(st.ids).size < st.ids.size and st.expect.removed > 800


def test_batches(chain):
    scheme, init, steps, states = chain
    by_name = {st.name: st for st in steps}
    assert by_name["every_list"].touched == list(range(ch.NLIST))
    assert by_name["one_list"].touched == [ch.L_PREC] and (by_name["one_list"].list_nos == ch.L_PREC).all()
    assert by_name["empty"].kind == "add" and by_name["empty"].list_nos.size == 0 and by_name["empty"].touched == []
    assert by_name["fresh"].kind == by_name["last"].kind == "query"
    # a step leaves some lists alone: their ROC streams are copied, not encoded again
    for st in steps:
        if st.name not in ("every_list", "add_800", "remove_any"):
            assert len(st.touched) < ch.NLIST - 4
