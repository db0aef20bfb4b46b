"""CPU: the numpy model of a merge (merge_ref.py) against a brute-force double loop, on random and adversarial pairs of objects:
empty lists on either or both sides, nlist 1, empty objects, a is b, add_id 0 and ntotal(a)."""
import numpy as np
import pytest

import merge_ref as mr


def _object(rng, sizes, hi=1 << 20):
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return off, rng.integers(0, hi, int(off[-1])).astype(np.uint64)


def _brute(a_off, a_ids, b_off, b_ids, add_id):
    """-> (offsets, ids, plain src, ascending src) list by list, entry by entry"""
    nlist = len(a_off) - 1
    off, ids, plain, asc = [0], [], [], []
    for l in range(nlist):
        M, S = [], []
        for p in range(int(a_off[l]), int(a_off[l + 1])):
            M.append(int(a_ids[p]))
            S.append(p)
        for p in range(int(b_off[l]), int(b_off[l + 1])):
            M.append((int(b_ids[p]) + add_id) % 2 ** 64)
            S.append(-p - 1)
        ids += M
        plain += S
        order = sorted(range(len(M)), key=lambda j: (M[j], j))
        asc += [S[j] for j in order]
        off.append(len(ids))
    return (np.array(off, np.uint64), np.array(ids, np.uint64), np.array(plain, np.int64).reshape(-1), np.array(asc, np.int64).reshape(-1))


def _pairs():
    rng = np.random.default_rng(4242)
    out = {}
    for name, sa, sb in (
        ("random", rng.integers(0, 40, 17), rng.integers(0, 40, 17)),
        ("one-sided", [0, 5, 0, 7, 0, 0, 3], [4, 0, 0, 2, 6, 0, 0]),
        ("nlist1", [9], [4]),
        ("nlist1-empty-a", [0], [4]),
        ("nlist1-empty-b", [9], [0]),
        ("empty-objects", [0, 0, 0], [0, 0, 0]),
        ("empty-b", [3, 0, 2], [0, 0, 0]),
        ("empty-a", [0, 0, 0], [1, 0, 8]),
        ("duplicates", [6, 6], [6, 6]),
    ):
        a, b = _object(rng, sa), _object(rng, sb)
        if name == "duplicates":
            b = (b[0], a[1].copy())
        out[name] = (a, b)
    a = _object(rng, rng.integers(0, 30, 11))
    out["a-is-b"] = (a, a)
    return out


PAIRS = _pairs()


@pytest.mark.parametrize("name", sorted(PAIRS))
@pytest.mark.parametrize("shift", ["zero", "ntotal"])
def test_model_is_the_double_loop(name, shift):
    (a_off, a_ids), (b_off, b_ids) = PAIRS[name]
    add_id = 0 if shift == "zero" else int(a_off[-1])
    m = mr.merge(a_off, a_ids, b_off, b_ids, add_id)
    off, ids, plain, asc = _brute(a_off, a_ids, b_off, b_ids, add_id)
    assert np.array_equal(m.offsets, off) and np.array_equal(m.ids, ids)
    assert np.array_equal(mr.src("plain", m), plain)
    assert np.array_equal(mr.src("ascending", m), asc)
    assert np.array_equal(mr.src("perm", m, mr.identity_perm(m)), plain)
    # every source position is named exactly once, and the gather through src rebuilds the ids
    for s in (plain, asc):
        assert sorted(s[s >= 0].tolist()) == list(range(a_ids.size)) and sorted((~s[s < 0]).tolist()) == list(range(b_ids.size))
        with np.errstate(over="ignore"):
            both = np.concatenate([a_ids, b_ids + np.uint64(add_id)])
        assert np.array_equal(both[np.where(s >= 0, s, a_ids.size + ~s)], ids if s is plain else np.concatenate(
            [np.sort(ids[int(off[l]):int(off[l + 1])]) for l in range(off.size - 1)] or [np.zeros(0, np.uint64)]))


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_roc_classes(name):
    (a_off, a_ids), (b_off, b_ids) = PAIRS[name]
    for add_id in (0, int(a_off[-1]) or 5):
        m = mr.merge(a_off, a_ids, b_off, b_ids, add_id)
        cls = mr.roc_classes(m, add_id)
        for l in range(m.nlist):
            a_n, b_n = int(a_off[l + 1] - a_off[l]), int(b_off[l + 1] - b_off[l])
            want = mr.KEEP_A if b_n == 0 else mr.KEEP_B if (a_n == 0 and add_id == 0) else mr.ENCODE
            assert cls[l] == want, (l, a_n, b_n, add_id)


def test_a_given_permutation():
    rng = np.random.default_rng(5)
    (a_off, a_ids), (b_off, b_ids) = PAIRS["random"]
    m = mr.merge(a_off, a_ids, b_off, b_ids, 7)
    off = m.offsets.astype(np.int64)
    perm = np.concatenate([rng.permutation(int(off[l + 1] - off[l])) for l in range(m.nlist)]).astype(np.uint32)
    s = mr.src("perm", m, perm)
    plain = mr.src("plain", m)
    for l in range(m.nlist):
        for q in range(int(off[l + 1] - off[l])):
            assert s[off[l] + q] == plain[off[l] + perm[off[l] + q]]


def test_refusals():
    big = 2 ** 32 - 1
    assert mr.refusal(True, 1, 2, 0, 1, 1, big, big) == mr.ERR_NULL
    assert mr.refusal(False, 1, 2, 0, 1, 1, big, big) == mr.ERR_NLIST
    assert mr.refusal(False, 2, 2, 0, 0, 1, big, big) == mr.ERR_DEVICE
    assert mr.refusal(False, 2, 2, 0, 1, 0, 0, 0) == mr.ERR_DEVICE
    assert mr.refusal(False, 2, 2, 0, 0, 0, big - 1, 1) == mr.ERR_NTOTAL
    assert mr.refusal(False, 2, 2, 0, 0, 0, big - 2, 1) == mr.OK
    assert mr.refusal(False, 0, 0, 3, 3, 3, 0, 0) == mr.OK
    assert mr.shift_overflows(2 ** 64 - 1, 1, 64) and not mr.shift_overflows(2 ** 64 - 2, 1, 64)
    assert mr.shift_overflows(2 ** 31 - 1, 1, 31) and not mr.shift_overflows(2 ** 31 - 2, 1, 31)
    assert mr.shift_overflows(255, 1, 8) and not mr.shift_overflows(254, 1, 8) and not mr.shift_overflows(0, 0, 0)


def test_roc_domain():
    a_off, b_off = np.array([0, 2, 2], np.uint64), np.array([0, 1, 2], np.uint64)
    a_ids, b_ids = np.array([1, 2], np.uint64), np.array([2 ** 31 - 1, 2 ** 31 - 1], np.uint64)
    m = mr.merge(a_off, a_ids, b_off, b_ids, 0)
    assert not mr.roc_domain_error(m, 0, b_ids)
    assert mr.roc_domain_error(mr.merge(a_off, a_ids, b_off, b_ids, 1), 1, b_ids)
    sizes_a, sizes_b = np.array([mr.ROC_MAX_LIST, 0], np.uint64), np.array([1, mr.ROC_MAX_LIST + 1], np.uint64)
    ao, bo = np.concatenate([[0], np.cumsum(sizes_a)]).astype(np.uint64), np.concatenate([[0], np.cumsum(sizes_b)]).astype(np.uint64)
    z = lambda o: np.zeros(int(o[-1]), np.uint64)
    assert mr.roc_domain_error(mr.merge(ao, z(ao), bo, z(bo), 0), 0, z(bo))  # list 0 re-encoded at MAX + 1 (list 1 is kept as it is)
