"""CPU: the numpy model of locate (tests/locate_ref.py) against a brute-force double loop over every list and offset, on random and
adversarial batches: duplicates inside a list, one id in several lists, repeated pairs, negative and too-large list numbers, ids the
object cannot hold, empty lists and an empty batch."""
import numpy as np
import pytest

from locate_ref import locate


def brute(offsets, obj_ids, list_nos, ids, id_bits):
    """every pair walks every list and every offset, in ascending order, and stops at its first hit"""
    nlist = len(offsets) - 1
    labels, missing, invalid = [], 0, 0
    for i in range(len(ids)):
        lab, valid = -1, True
        if list_nos is not None and int(list_nos[i]) < 0:
            valid = False
        elif list_nos is not None and int(list_nos[i]) >= nlist:
            valid = False
            invalid += 1
        elif id_bits >= 64 or int(ids[i]) >> id_bits == 0:
            for l in range(nlist):
                if lab >= 0 or (list_nos is not None and l != int(list_nos[i])):
                    continue
                for o in range(int(offsets[l + 1]) - int(offsets[l])):
                    if int(obj_ids[int(offsets[l]) + o]) == int(ids[i]):
                        lab = (l << 32) | o
                        break
        labels.append(lab)
        missing += int(valid and lab < 0)
    return np.array(labels, np.int64).reshape(-1), missing, invalid


def _check(offsets, obj_ids, list_nos, ids, id_bits=64):
    got = locate(offsets, obj_ids, list_nos, ids, id_bits)
    exp = brute(offsets, obj_ids, list_nos, ids, id_bits)
    assert np.array_equal(got[0], exp[0]) and got[1:] == exp[1:], (got, exp)
    return got


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("any_list", [False, True])
def test_random_batches(seed, any_list):
    rng = np.random.default_rng(seed)
    nlist = int(rng.integers(1, 9))
    sizes = rng.integers(0, 12, nlist)
    sizes[rng.integers(0, nlist)] = 0  # an empty list
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    obj = rng.integers(0, 20, int(off[-1])).astype(np.uint64)  # a small universe: duplicates inside lists, ids in several lists
    n = int(rng.integers(0, 40))
    ids = rng.integers(0, 24, n).astype(np.uint64)
    ln = None if any_list else rng.integers(-2, nlist + 2, n).astype(np.int64)
    labels, missing, invalid = _check(off, obj, ln, ids)
    hit = labels >= 0
    assert np.array_equal(obj[off[labels[hit] >> 32].astype(np.int64) + (labels[hit] & 0xFFFFFFFF)], ids[hit])  # the defining property


def test_duplicates_take_the_smallest_label():
    off = np.array([0, 3, 3, 6], np.uint64)
    obj = np.array([7, 5, 7, 9, 7, 5], np.uint64)
    labels, missing, invalid = _check(off, obj, None, np.array([7, 5, 9, 7], np.uint64))
    assert labels.tolist() == [0, 1, 2 << 32, 0] and (missing, invalid) == (0, 0)
    labels, missing, invalid = _check(off, obj, np.array([2, 2, 0, 1, -1, 3], np.int64), np.array([7, 5, 9, 7, 7, 7], np.uint64))
    assert labels.tolist() == [(2 << 32) | 1, (2 << 32) | 2, -1, -1, -1, -1] and (missing, invalid) == (2, 1)


def test_repeated_pairs_each_count_and_share_a_label():
    off = np.array([0, 2], np.uint64)
    obj = np.array([4, 8], np.uint64)
    labels, missing, invalid = _check(off, obj, np.zeros(4, np.int64), np.array([8, 3, 8, 3], np.uint64))
    assert labels.tolist() == [1, -1, 1, -1] and (missing, invalid) == (2, 0)


def test_ids_the_object_cannot_hold_are_missing():
    off = np.array([0, 2], np.uint64)
    obj = np.array([1, 3], np.uint64)
    ids = np.array([3, 3 + (1 << 32), 1 << 40, 2 ** 64 - 1], np.uint64)
    for bits in (2, 32, 64):
        labels, missing, invalid = _check(off, obj, None, ids, bits)
        assert labels.tolist() == [1, -1, -1, -1] and (missing, invalid) == (3, 0)
    assert _check(off, np.array([1, 3 + (1 << 32)], np.uint64), None, ids, 64)[0].tolist() == [-1, 1, -1, -1]


def test_empty_batch_empty_lists_and_a_batch_without_a_valid_pair():
    off = np.array([0, 0, 0], np.uint64)
    obj = np.zeros(0, np.uint64)
    for ln in (None, np.zeros(0, np.int64)):
        labels, missing, invalid = _check(off, obj, ln, np.zeros(0, np.uint64))
        assert labels.size == 0 and (missing, invalid) == (0, 0)
    assert _check(off, obj, None, np.array([0, 1], np.uint64))[1:] == (2, 0)
    labels, missing, invalid = _check(off, obj, np.array([-1, 2, -7, 9], np.int64), np.arange(4, dtype=np.uint64))
    assert labels.tolist() == [-1] * 4 and (missing, invalid) == (0, 2)
