"""CPU: the numpy model of a subset (subset_ref.py) against a brute-force double loop written directly from the table of
include/vidc.h ("subset"), on random and adversarial objects; and the properties that make copy_subset_to the inverse of merge_from:
the parts of ID_MOD, INVLIST_FRACTION, INVLIST and of adjacent ID_RANGEs partition every list in order."""
import numpy as np
import pytest

import subset_ref as sr

TYPES = [sr.ID_RANGE, sr.ID_MOD, sr.ELEMENT_RANGE, sr.INVLIST_FRACTION, sr.INVLIST]


def brute(subset_type, a1, a2, off, ids):
    """entry i of list l is taken iff ... : one Python-integer test per entry -> (mask, new offsets, S)"""
    off = [int(x) for x in off]
    T = off[-1]
    mask, new_off, S = [], [0], []
    for l in range(len(off) - 1):
        n = off[l + 1] - off[l]
        for i in range(n):
            x = int(ids[off[l] + i])
            if subset_type == 0:
                t = a1 <= x < a2
            elif subset_type == 1:
                t = x % a1 == a2
            elif subset_type == 2:
                i1 = off[l + 1] * a1 // T - off[l] * a1 // T
                i2 = off[l + 1] * a2 // T - off[l] * a2 // T
                t = i1 <= i < i2
            elif subset_type == 3:
                t = n * a2 // a1 <= i < n * (a2 + 1) // a1
            else:
                t = a1 <= l < a2
            mask.append(int(t))
            if t:
                S.append(x)
        new_off.append(len(S))
    return np.array(mask, np.uint8), np.array(new_off, np.uint64), np.array(S, np.uint64)


def check(subset_type, a1, a2, off, ids):
    m = sr.subset(subset_type, a1, a2, off, ids)
    mask, new_off, S = brute(subset_type, a1, a2, off, ids)
    what = (subset_type, a1, a2)
    assert np.array_equal(m.mask, mask), what
    assert np.array_equal(m.offsets, new_off), what
    assert np.array_equal(m.ids, S), what
    assert m.n_taken == S.size == int(mask.sum())
    n = np.diff(np.asarray(off).astype(np.int64))
    n_new = np.diff(new_off.astype(np.int64))
    assert [sr.roc_class(int(a), int(b)) for a, b in zip(n, n_new)] == m.classes.tolist()
    return m


def obj(sizes, rng, hi=1 << 20):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return off, rng.integers(0, hi, int(off[-1]), dtype=np.uint64)


def args_for(subset_type, rng, nlist, T):
    if subset_type == 0:
        a, b = sorted(int(x) for x in rng.integers(0, 1 << 20, 2))
        return a, b
    if subset_type == 1:
        a1 = int(rng.integers(1, 9))
        return a1, int(rng.integers(0, a1))
    if subset_type == 2:
        a, b = sorted(int(x) for x in rng.integers(0, T + 1, 2))
        return a, b
    if subset_type == 3:
        a1 = int(rng.integers(1, 12))
        return a1, int(rng.integers(0, a1))
    a, b = (int(x) for x in rng.integers(0, nlist + 3, 2))
    return a, b


@pytest.mark.parametrize("subset_type", TYPES)
def test_random_objects(subset_type):
    rng = np.random.default_rng(100 + subset_type)
    for _ in range(60):
        nlist = int(rng.integers(1, 9))
        sizes = rng.integers(0, 12, nlist) * (rng.random(nlist) < 0.7)
        if sizes.sum() == 0:
            sizes[0] = 3
        off, ids = obj(sizes, rng)
        check(subset_type, *args_for(subset_type, rng, nlist, int(off[-1])), off, ids)


def test_element_range_bounds_can_cross():
    """offsets 0, 3, 4, 10 with a1 = 3, a2 = 4: list 1 gets i1 = 1, i2 = 0 and gives nothing"""
    off = np.array([0, 3, 4, 10], np.uint64)
    ids = np.arange(10, dtype=np.uint64)
    T = 10
    i1 = int(off[2]) * 3 // T - int(off[1]) * 3 // T
    i2 = int(off[2]) * 4 // T - int(off[1]) * 4 // T
    assert (i1, i2) == (1, 0)
    m = check(sr.ELEMENT_RANGE, 3, 4, off, ids)
    assert m.offsets[2] - m.offsets[1] == 0 and m.classes[1] == sr.EMPTY
    b1, b2 = sr.bounds(sr.ELEMENT_RANGE, 3, 4, off)
    assert b1[1] == 1 and b2[1] == 1  # (clamped: [i1, i1) is empty)


def test_element_range_takes_at_most_n_per_list_and_never_reads_past_a_list():
    rng = np.random.default_rng(7)
    for _ in range(40):
        nlist = int(rng.integers(1, 8))
        off, ids = obj(rng.integers(0, 9, nlist) + (rng.random(nlist) < 0.2) * 40, rng)
        T = int(off[-1])
        if not T:
            continue
        for a1 in range(0, T + 1, max(1, T // 7)):
            for a2 in range(a1, T + 1, max(1, T // 5)):
                i1, i2 = sr.bounds(sr.ELEMENT_RANGE, a1, a2, off)
                n = np.diff(off.astype(np.int64))
                assert (i2 <= n).all() and (i1 <= i2).all()
                check(sr.ELEMENT_RANGE, a1, a2, off, ids)


@pytest.mark.parametrize("subset_type", TYPES)
def test_empty_lists_empty_objects_and_equal_arguments(subset_type):
    rng = np.random.default_rng(9)
    off0 = np.zeros(5, np.uint64)
    none = np.zeros(0, np.uint64)
    a = {0: (3, 9), 1: (3, 1), 2: (0, 0), 3: (4, 2), 4: (1, 3)}[subset_type]
    m = check(subset_type, *a, off0, none)  # T = 0: an empty object for every type
    assert m.n_taken == 0 and not m.offsets.any() and (m.classes == sr.KEEP).all()
    off, ids = obj(np.array([0, 4, 0, 0, 7, 1, 0]), rng)
    check(subset_type, *a if subset_type != 2 else (2, 9), off, ids)
    if subset_type in (0, 2, 4):  # a1 == a2 takes nothing
        for v in (0, 5, 12):
            if subset_type != 2 or v <= 12:
                assert check(subset_type, v, v, off, ids).n_taken == 0
    if subset_type == 4:  # clamped and reversed list ranges
        assert check(4, 0, 2 ** 64 - 1, off, ids).n_taken == 12
        assert check(4, 5, 2, off, ids).n_taken == 0
        assert check(4, 6, 900, off, ids).n_taken == 0 and check(4, 4, 900, off, ids).n_taken == 8


def test_fraction_over_every_part_including_more_parts_than_entries():
    rng = np.random.default_rng(11)
    off, ids = obj(np.array([0, 1, 2, 3, 7, 64, 65]), rng)
    for a1 in (1, 2, 3, 4, 7, 8, 64, 66, 1000, 2 ** 32 - 1):
        parts = range(a1) if a1 <= 66 else (0, 1, a1 // 2, a1 - 2, a1 - 1)
        total = 0
        for a2 in parts:
            total += check(sr.INVLIST_FRACTION, a1, a2, off, ids).n_taken
        if a1 <= 66:
            assert total == ids.size


def test_wide_ids():
    """ids >= 2^32 and >= 2^63 compare and reduce on all 64 bits"""
    off = np.array([0, 4, 4, 9], np.uint64)
    ids = np.array([5, 2 ** 32, 2 ** 32 + 5, 2 ** 63, 2 ** 63 + 7, 2 ** 64 - 1, 2 ** 40 + 3, 7, 2 ** 32 - 1], np.uint64)
    for a1, a2 in ((0, 2 ** 32), (2 ** 32, 2 ** 63), (2 ** 63, 2 ** 64 - 1), (2 ** 32 + 1, 2 ** 63 + 8), (0, 2 ** 64 - 1), (2 ** 63 + 7, 2 ** 63 + 7)):
        check(sr.ID_RANGE, a1, a2, off, ids)
    for a1 in (1, 2, 3, 8, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 10 ** 12 + 39, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1):
        for a2 in {0, a1 - 1, a1 // 2, 5 % a1, 7 % a1, (2 ** 64 - 1) % a1}:
            check(sr.ID_MOD, a1, a2, off, ids)
        assert sr.mod_kind(a1) == (sr.MOD_MASK if a1 & (a1 - 1) == 0 else sr.MOD_U32 if a1 < 2 ** 32 else sr.MOD_U64)


def parts_partition(off, ids, parts):
    """the parts (Subset objects) partition every list in order: every position is in exactly one, and interleaving the parts by
    position gives the list back"""
    total = np.zeros(ids.size, np.int64)
    for p in parts:
        total += p.mask
        assert np.array_equal(p.ids, ids[p.mask == 1])  # order kept
    assert (total == 1).all()
    assert np.array_equal(sum(p.offsets.astype(np.int64) for p in parts), off.astype(np.int64))


def test_the_parts_partition_every_list():
    rng = np.random.default_rng(13)
    off, ids = obj(np.array([0, 1, 5, 64, 0, 130, 3]), rng)
    nlist = off.size - 1
    for a1 in (1, 2, 3, 5, 8):
        parts_partition(off, ids, [sr.subset(sr.ID_MOD, a1, r, off, ids) for r in range(a1)])
        parts_partition(off, ids, [sr.subset(sr.INVLIST_FRACTION, a1, r, off, ids) for r in range(a1)])
    cuts = [0, 2, 2, 5, nlist + 4]
    parts_partition(off, ids, [sr.subset(sr.INVLIST, a, b, off, ids) for a, b in zip(cuts[:-1], cuts[1:])])
    cuts = [0, 1000, 1 << 19, 1 << 19, 2 ** 64 - 1]  # (no id is 2^64 - 1)
    parts_partition(off, ids, [sr.subset(sr.ID_RANGE, a, b, off, ids) for a, b in zip(cuts[:-1], cuts[1:])])


def test_refusals():
    big = 2 ** 64 - 1
    assert sr.refusal(True, 0, 0, 0, 0) == sr.ERR_NULL
    for t in (-1, 5, 99):
        assert sr.refusal(False, t, 1, 0, 10) == sr.ERR_TYPE
    assert sr.refusal(False, 0, 9, 3, 10) == sr.OK and sr.refusal(False, 0, big, big, 0) == sr.OK
    assert sr.refusal(False, 1, 0, 0, 10) == sr.ERR_ARGS and sr.refusal(False, 1, 3, 3, 10) == sr.ERR_ARGS
    assert sr.refusal(False, 1, 1, 0, 10) == sr.OK and sr.refusal(False, 1, big, big - 1, 10) == sr.OK
    assert sr.refusal(False, 2, 4, 3, 10) == sr.ERR_ARGS and sr.refusal(False, 2, 3, 11, 10) == sr.ERR_ARGS
    assert sr.refusal(False, 2, 0, 10, 10) == sr.OK and sr.refusal(False, 2, 0, 0, 0) == sr.OK and sr.refusal(False, 2, 0, 1, 0) == sr.ERR_ARGS
    assert sr.refusal(False, 3, 0, 0, 10) == sr.ERR_ARGS and sr.refusal(False, 3, 2 ** 32, 0, 10) == sr.ERR_ARGS
    assert sr.refusal(False, 3, 4, 4, 10) == sr.ERR_ARGS and sr.refusal(False, 3, 2 ** 32 - 1, 2 ** 32 - 2, 10) == sr.OK
    assert sr.refusal(False, 4, 7, 2, 10) == sr.OK and sr.refusal(False, 4, big, big, 10) == sr.OK
