"""tests/append_ref.py pinned on the CPU: the merge against a per-list Python loop, the two facts about the ROC codec that the spliced
append rests on (checked with the CPU oracle), and the agreement with tests/contract_ref.py on the merged CSR."""
import numpy as np
import pytest

import append_ref as ar
import contract_ref as cr


def _brute(offsets, old, list_nos, add_ids):
    """the definition, list by list: M_l = old_l ++ batch entries of l in ascending i"""
    nlist = len(offsets) - 1
    lists = [list(old[int(offsets[l]):int(offsets[l + 1])]) for l in range(nlist)]
    rank, invalid = [], 0
    for l, x in zip(list_nos, add_ids):
        if l < 0:
            rank.append(-1)
        elif l >= nlist:
            rank.append(-1)
            invalid += 1
        else:
            rank.append(len(lists[l]) - int(offsets[l + 1] - offsets[l]))
            lists[l].append(x)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = np.array([x for li in lists for x in li], dtype=np.uint64)
    return off, flat, np.array(rank, np.int64), invalid


def _case(seed, nlist, ntotal, n_add, empty_every=0, only_list=None, bad=True):
    rng = np.random.default_rng(seed)
    lst = rng.integers(0, nlist, ntotal)
    if empty_every:
        lst = lst[lst % empty_every != 0]
    sizes = np.bincount(lst, minlength=nlist)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    old = rng.permutation(1 << 20)[: int(off[-1])].astype(np.uint64)
    ln = rng.integers(0, nlist, n_add).astype(np.int64) if only_list is None else np.full(n_add, only_list, np.int64)
    if bad and n_add >= 8:
        ln[rng.integers(0, n_add, n_add // 8)] = -1
        ln[rng.integers(0, n_add, n_add // 8)] = nlist + rng.integers(0, 5)
        ln[rng.integers(0, n_add)] = -(1 << 40)
    add = ((1 << 20) + rng.permutation(1 << 16)[:n_add]).astype(np.uint64)
    return off, old, ln, add


CASES = [
    dict(seed=1, nlist=7, ntotal=60, n_add=40),
    dict(seed=2, nlist=13, ntotal=200, n_add=90, empty_every=3),
    dict(seed=3, nlist=5, ntotal=30, n_add=0),
    dict(seed=4, nlist=9, ntotal=0, n_add=25),
    dict(seed=5, nlist=6, ntotal=50, n_add=33, only_list=4, bad=False),
    dict(seed=6, nlist=1, ntotal=10, n_add=12),
    dict(seed=7, nlist=40, ntotal=3, n_add=300),
]


@pytest.mark.parametrize("case", CASES, ids=[f"case{c['seed']}" for c in CASES])
def test_merge_matches_the_per_list_loop(case):
    off, old, ln, add = _case(**case)
    m = ar.merge(off, old, ln, add)
    b_off, b_flat, b_rank, b_invalid = _brute(off, old, ln.tolist(), add.tolist())
    assert np.array_equal(m.offsets, b_off) and np.array_equal(m.ids, b_flat)
    assert np.array_equal(m.rank, b_rank) and m.invalid == b_invalid
    assert np.array_equal(m.valid, b_rank >= 0)
    # labels of the input-order containers: |old_l| + rank, -1 for skipped pairs; translating them gives the batch ids back
    for kind in ("packed", "wt"):
        lab = ar.labels(kind, m)
        assert np.array_equal(lab < 0, ~m.valid)
        v = np.flatnonzero(m.valid)
        pos = m.offsets[(lab[v] >> 32)].astype(np.int64) + (lab[v] & 0xFFFFFFFF)
        assert np.array_equal(m.ids[pos], add[v])
        assert np.array_equal(ar.perm(kind, m), np.concatenate([np.arange(int(n)) for n in np.diff(m.offsets.astype(np.int64))] + [[]]))


def test_all_pairs_skipped_is_the_old_object():
    off, old, ln, add = _case(seed=8, nlist=5, ntotal=40, n_add=10, bad=False)
    ln[:] = [-1, 5, 6, -7, 5, -1, 99, -1, 5, 1 << 40]
    m = ar.merge(off, old, ln, add)
    assert np.array_equal(m.offsets, off) and np.array_equal(m.ids, old) and m.invalid == 6 and not m.valid.any()
    assert (ar.labels("ef", m) == -1).all()


def test_ef_labels_and_perm_are_the_stable_ascending_order():
    off, old, ln, add = _case(seed=9, nlist=6, ntotal=80, n_add=50)
    s_old = old.copy()  # an Elias-Fano object returns its lists ascending
    for l in range(6):
        s_old[int(off[l]):int(off[l + 1])].sort()
    m = ar.merge(off, s_old, ln, add)
    p = ar.perm("ef", m)
    lab = ar.labels("ef", m)
    o = m.offsets.astype(np.int64)
    for l in range(6):
        seg = m.ids[o[l]:o[l + 1]]
        assert np.array_equal(seg[p[o[l]:o[l + 1]]], np.sort(seg))
    v = np.flatnonzero(m.valid)
    dec = cr.ListRef("ef", m.offsets, m.ids).flat  # what the new object decodes to
    assert np.array_equal(dec[o[lab[v] >> 32] + (lab[v] & 0xFFFFFFFF)], add[v])


def _rand_list(rng, dup):
    u = int(rng.choice([50, 1000, 1 << 16, 1 << 20, (1 << 31) - 1]))
    n = int(rng.integers(1, min(u, 300)))
    if dup:
        ids = rng.integers(0, u, n).astype(np.uint64)
        ids[rng.integers(0, n)] = ids[0]
        return ids
    return rng.choice(u, n, replace=False).astype(np.uint64) if u <= (1 << 20) else np.unique(rng.integers(0, u, n)).astype(np.uint64)


@pytest.mark.parametrize("dup", [False, True], ids=["distinct", "duplicates"])
def test_roc_stream_depends_only_on_the_multiset(oracle, dup):
    """head, words and mt19937 draws of a list are the same for every input order: the stream of M_l is the stream of the union"""
    rng = np.random.default_rng(11 + dup)
    for _ in range(60):
        ids = _rand_list(rng, dup)
        prec = oracle.list_precision(ids)
        a = oracle.roc_encode(ids, prec)
        for other in (np.sort(ids), ids[rng.permutation(ids.size)]):
            b = oracle.roc_encode(other, prec)
            assert a["head"] == b["head"] and a["mt_draws"] == b["mt_draws"] and np.array_equal(a["words"], b["words"])


def test_roc_reencoding_a_decoded_distinct_list_gives_the_identity_permutation(oracle):
    """the permutation over M of a list the batch does not touch is the identity"""
    rng = np.random.default_rng(13)
    for _ in range(60):
        ids = _rand_list(rng, False)
        prec = oracle.list_precision(ids)
        e = oracle.roc_encode(ids, prec)
        dec = oracle.roc_decode(e["head"], e["words"], ids.size, prec, e["mt_draws"])[0]
        if not np.array_equal(np.sort(dec), np.sort(ids)):
            continue  # (the reference's power-of-two-maximum quirk: the list did not survive the codec)
        again = oracle.roc_encode(dec, oracle.list_precision(dec))
        assert np.array_equal(again["perm"], np.arange(ids.size))
        assert np.array_equal(ar.list_perm("roc", dec, oracle), np.arange(ids.size))


def test_roc_labels_invert_the_sampling_permutation(oracle):
    off, old, ln, add = _case(seed=14, nlist=5, ntotal=70, n_add=30)
    m = ar.merge(off, old, ln, add)
    lab = ar.labels("roc", m, oracle)
    p = ar.perm("roc", m, oracle)
    o = m.offsets.astype(np.int64)
    v = np.flatnonzero(m.valid)
    l, q = lab[v] >> 32, lab[v] & 0xFFFFFFFF
    assert np.array_equal(l, ln[v])
    assert np.array_equal(p[o[l] + q], m.old_n[l] + m.rank[v])  # the entry at offset q is the batch entry
    assert np.array_equal(m.ids[o[l] + p[o[l] + q]], add[v])


@pytest.mark.parametrize("kind", ["packed", "ef"])
def test_contract_ref_on_the_merged_csr_is_decode_then_concatenate(kind):
    """ListRef on the CSR of M == (what the old object decodes to) ++ batch, put into the container's order"""
    off, raw, ln, add = _case(seed=15, nlist=8, ntotal=120, n_add=70)
    old = cr.ListRef(kind, off, raw).flat  # the old object's own order
    m = ar.merge(off, old, ln, add)
    ref = cr.ListRef(kind, m.offsets, m.ids)
    o0, o1 = off.astype(np.int64), m.offsets.astype(np.int64)
    for l in range(8):
        cat = np.concatenate([old[o0[l]:o0[l + 1]], add[ln == l]])
        got, _ = ref.expected([l])
        assert np.array_equal(got, cat if kind == "packed" else np.sort(cat))
    flat, out_off = cr.expected_lists(kind, m.offsets, m.ids, None)
    assert np.array_equal(out_off, m.offsets) and flat.size == int(o1[-1])
