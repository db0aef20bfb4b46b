"""CPU: the numpy port of the select0 rank (tests/ef_rank_ref.py, the algorithm of csrc/ef_rank_ref.h) against the statement of the
contract (np.searchsorted), at every entry, every entry +- 1, 0, u, u + 1, 2^32, 2^63 and 2^64 - 1, on every family of lists_ref and on
the designed lists; and the designed lists hold what they are named for."""
import numpy as np
import pytest

import ef_rank_ref as er
import lists_ref as lr


def check_list(ids, what, cap=None):
    im = er.Image(ids)
    q = er.queries(ids)
    if cap is not None and q.size > cap:  # (long lists: the structural queries and a sample of the rest)
        rng = np.random.default_rng(q.size)
        q = np.unique(np.concatenate([q[:8], q[-8:], rng.choice(q, cap, replace=False)]))
    ranks, found, _ = er.statement([ids], np.zeros(q.size, np.int64), q)
    for x, r, f in zip(q.tolist(), ranks.tolist(), found.tolist()):
        assert er.rank_image(im, x) == (r, f), f"{what}: x = {x}"
    return q.size


@pytest.mark.parametrize("name", lr.FAMILIES)
def test_port_equals_searchsorted_on_every_family(name):
    n = 0
    for i, ids in enumerate(lr.family(name)):
        n += check_list(ids, f"{name}[{i}]", cap=400)
    assert n > 0


@pytest.mark.parametrize("obj", ["short", "half"])
def test_port_on_the_object_lists_narrow_and_wide(obj):
    for i, ids in enumerate(lr.base_lists(obj) + lr.wide_lists(obj)):
        check_list(ids, f"{obj}[{i}]", cap=150)


def test_designed_lists_hold_what_they_are_named_for():
    er.check_designed(er.designed())


@pytest.mark.parametrize("name", sorted(er.designed()))
def test_port_equals_searchsorted_on_the_designed_lists(name):
    ids = er.designed()[name]
    assert check_list(ids, name) >= 4


def test_statement_rules():
    lists = [lr.u64([3, 3, 9]), np.zeros(0, np.uint64), lr.u64([1 << 40])]
    ln = np.array([0, 0, 0, 0, 1, 2, 2, -1, 3, -7, 5], np.int64)
    ids = lr.u64([0, 3, 4, 10, 5, 1 << 40, er.M64, 3, 3, 3, 3])
    r, f, inv = er.statement(lists, ln, ids)
    assert r.tolist() == [0, 0, 2, 3, 0, 0, 1, -1, -1, -1, -1] and f.tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0] and inv == 2
    c = er.count_range(lists, np.array([0, 0, 0, 1, -1, 4], np.int64), lr.u64([0, 3, 9, 0, 0, 0]), lr.u64([er.M64, 9, 3, 5, 9, 9]))
    assert c.tolist() == [3, 2, 0, 0, 0, 0]
    rows = np.array([[1, 2, -1], [-1, -1, -1], [0, 1, 2]], np.int32)
    assert er.has_edges(rows, [0, 0, 1, 2, 3, -1, 0], [2, 0, 0, 0, 0, 0, -1]).tolist() == [True, False, False, True, False, False, False]


def test_select_in_word_and_the_tie_rule():
    rng = np.random.default_rng(3)
    for w in [1, 1 << 63, er.M64, 0x8000000000000001] + [int(v) for v in rng.integers(1, 1 << 63, 50, dtype=np.uint64)]:
        pos = [i for i in range(64) if w >> i & 1]
        for k, p in enumerate(pos):
            assert er.select_in_word(w, k) == p
    # batches 1 and 2 hold ones only (4096 more elements in front of each following batch): they tie with batch 3 at 10 zeros, and the
    # zero number 10 is in the last of them
    hr = [0, 4086, 8182, 12278, 12300]
    assert [er.zeros_before_batch(k, v) for k, v in enumerate(hr)] == [0, 10, 10, 10, 4084]
    assert er.batch_of_zero(hr, 9) == 0 and er.batch_of_zero(hr, 10) == 3 and er.batch_of_zero(hr, 4083) == 3 and er.batch_of_zero(hr, 4084) == 4
