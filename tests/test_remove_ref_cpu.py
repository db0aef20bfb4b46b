"""CPU: the numpy model of a remove (tests/remove_ref.py) against a brute-force loop over the pairs, on tiny cases."""
import numpy as np
import pytest

import remove_ref as rr


def brute(off, ids, ln, rm):
    nlist = len(off) - 1
    lists = [list(ids[off[l]:off[l + 1]]) for l in range(nlist)]
    mask = [[0] * len(x) for x in lists]
    missing = invalid = 0
    for i, x in enumerate(rm):
        if ln is None:
            targets = range(nlist)
        elif ln[i] < 0:
            continue
        elif ln[i] >= nlist:
            invalid += 1
            continue
        else:
            targets = [ln[i]]
        hit = False
        for l in targets:
            for j, y in enumerate(lists[l]):
                if int(y) == int(x):
                    mask[l][j] = 1
                    hit = True
        missing += not hit
    out = [[y for y, m in zip(x, mk) if not m] for x, mk in zip(lists, mask)]
    new_off = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.uint64)
    flat = np.array([y for x in out for y in x], dtype=np.uint64)
    return new_off, flat, np.array([m for mk in mask for m in mk], dtype=np.uint8), missing, invalid


OFF = np.array([0, 4, 4, 7, 8, 12], np.uint64)
IDS = np.array([5, 9, 5, 2,  7, 9, 1,  3,  (1 << 40) + 5, 5, 6, 1 << 33], np.uint64)  # 5 twice in list 0; 9 and 5 in several lists

CASES = {
    "duplicates inside a list": ([0], [5]),
    "the same id in two lists, one named": ([2], [9]),
    "repeated pairs": ([0, 0, 0, 4, 4], [9, 9, 9, 6, 6]),
    "skipped and invalid list numbers": ([-1, 5, 7, -9, 0, 1 << 40], [5, 5, 5, 5, 2, 2]),
    "absent id, and a present id under the wrong list": ([0, 1, 3], [100, 5, 7]),
    "high and low halves": ([4, 4, 4], [5, (1 << 40) + 6, (1 << 41) + 5]),
    "everything removed": (np.repeat(np.arange(5), [4, 0, 3, 1, 4]), IDS),
    "nothing removed": ([], []),
    "an id that misses twice": ([3, 3], [4, 4]),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", ["pairs", "any"])
def test_model_equals_brute_force(name, mode):
    ln, rm = CASES[name]
    ln = None if mode == "any" else np.asarray(ln, np.int64)
    rm = np.asarray(rm, np.uint64)
    got = rr.remove(OFF, IDS, ln, rm)
    off, ids, mask, missing, invalid = brute(OFF.astype(np.int64), IDS, ln, rm)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.ids, ids)
    assert np.array_equal(got.mask, mask) and got.mask.dtype == np.uint8
    assert (got.missing, got.invalid) == (missing, invalid)
    assert got.removed == int(mask.sum()) == int(OFF[-1] - off[-1])


def test_the_cases_say_what_their_names_say():
    r = rr.remove(OFF, IDS, [0], [5])
    assert r.removed == 2 and np.array_equal(r.ids[:2], [9, 2])
    assert rr.remove(OFF, IDS, [2], [9]).removed == 1 and rr.remove(OFF, IDS, None, [9]).removed == 2
    r = rr.remove(OFF, IDS, [-1, 5, 7, -9, 0, 1 << 40], [5, 5, 5, 5, 2, 2])
    assert (r.removed, r.missing, r.invalid) == (1, 0, 3)
    r = rr.remove(OFF, IDS, [0, 1, 3], [100, 5, 7])
    assert (r.removed, r.missing) == (0, 3)
    r = rr.remove(OFF, IDS, [4, 4, 4], [5, (1 << 40) + 6, (1 << 41) + 5])
    assert (r.removed, r.missing) == (1, 2) and np.array_equal(r.ids[-3:], [(1 << 40) + 5, 6, 1 << 33])
    r = rr.remove(OFF, IDS, np.repeat(np.arange(5), [4, 0, 3, 1, 4]), IDS)
    assert r.removed == 12 and not r.offsets.any() and r.missing == 0
    r = rr.remove(OFF, IDS, [], [])
    assert r.removed == 0 and np.array_equal(r.offsets, OFF) and np.array_equal(r.ids, IDS)


def test_random_small_objects():
    rng = np.random.default_rng(5)
    for _ in range(60):
        nlist = int(rng.integers(0, 6))
        sizes = rng.integers(0, 7, nlist)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        ids = rng.integers(0, 12, int(off[-1])).astype(np.uint64)
        n = int(rng.integers(0, 15))
        ln = rng.integers(-2, nlist + 2, n).astype(np.int64)
        rm = rng.integers(0, 14, n).astype(np.uint64)
        for lists in (ln, None):
            got = rr.remove(off, ids, lists, rm)
            o, i, m, mi, iv = brute(off.astype(np.int64), ids, lists, rm)
            assert np.array_equal(got.offsets, o) and np.array_equal(got.ids, i) and np.array_equal(got.mask, m)
            assert (got.missing, got.invalid) == (mi, iv)
