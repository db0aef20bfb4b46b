"""Re-balancing a sharded object on the GPU (vidc_rebalance_sharded, include/vidc.h "sharded lists"): the lists move to the map a fresh
encode would choose; packed bits and Elias-Fano are rebuilt from decode_all on the device, ROC lists move as streams.

Family F and the contexts are those of tests/test_gpu_shards.py (every context on device 0).  S is the sharded object of F; S1 is S after
an update that keeps the old map -- the skew batch (900 pairs into the lists of ONE shard) appended, or a third of shard 0's ids removed
(tests/rebalance_ref.py; tests/test_shards_rebalance_cpu.py checks that both change the map at 2, 3 and 8 shards) -- and U1 is the same
update on the unsharded object.  R = S1.rebalance(): its map, loads and moved_ids are the numpy model's; every shard is, word for word,
what the single-object encoder builds from the new cut of decode_all(S1); for ROC every list also equals its old owner's list in metadata
and words; every request answers as on S1 and as on U1; the permutation is the identity.
"""
import ctypes
import gc

import numpy as np
import pytest

import rebalance_ref as rr
from test_gpu_shards import (KINDS, NSHARDS, REQUEST, all_labels, assert_same_image, check_translate, csr, decode_all_guarded, dev, encode_s,
                             encode_u, gather_request, image, sum_d2h)
from test_gpu_shards_append import append_to, encode_single, shard_images
from test_shards_cpu import F_SIZES

pytestmark = pytest.mark.gpu

ARMS = ["append", "remove"]


def _torch():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctxs():
    """a home context and eight shard contexts, all on device 0"""
    L = _L()
    _torch().cuda.set_device(0)
    cs = [L.Context(0) for _ in range(9)]
    yield cs[8], cs[:8]
    for c in cs:
        c.synchronize()


@pytest.fixture(scope="module")
def F():
    return csr(F_SIZES)


def want_perm(kind):
    return kind != "packed"


def remove_from(obj, ln, ids, kind):
    from vector_db_id_compression_amd import removal

    torch = _torch()
    d_ln, d_ids = torch.from_numpy(np.ascontiguousarray(ln, dtype=np.int64)).cuda(), dev(ids)
    torch.cuda.synchronize()
    new, _ = removal.remove(obj, d_ln, d_ids, want_perm=want_perm(kind), removed=False)
    torch.cuda.synchronize()
    return new


def update(obj, kind, ns, arm, F):
    """the update that keeps the map (S -> S1, U -> U1)"""
    if arm == "append":
        return append_to(obj, *rr.skew_batch(ns), kind, labels=False, count=False)[0]
    return remove_from(obj, *rr.remove_batch(F[0], F[1], ns), kind)


def rebalance(S1, kind):
    _torch().cuda.synchronize()
    return S1.rebalance(want_perm=want_perm(kind))


def sizes_of(X):
    off = np.asarray(X.offsets).astype(np.int64)
    return off[1:] - off[:-1]


@pytest.fixture(scope="module")
def rebalanced(ctxs, F):
    """per (kind, nshards, arm), built once: U1, S1, R = S1.rebalance(), moved_ids, the numpy model, S1's decode_all and shard images
    before the call and what the contexts' d2h counters did across it"""
    home, shard_ctxs = ctxs
    off, ids = F
    cache = {}

    def get(kind, ns, arm):
        if (kind, None) not in cache:
            cache[(kind, None)] = encode_u(kind, off, ids)
        if (kind, ns, arm) not in cache:
            U1 = update(cache[(kind, None)], kind, ns, arm, F)
            S1 = update(encode_s(kind, off, ids, home, shard_ctxs[:ns]), kind, ns, arm, F)
            before = decode_all_guarded(S1)
            old_images = shard_images(kind, S1, with_perm=False)
            old_map = (np.array(S1.owner), np.array(S1.local_no), np.array(S1.loads))
            d2h = [home.d2h_bytes()] + [c.d2h_bytes() for c in shard_ctxs]
            R, moved = rebalance(S1, kind)
            d2h_after = [home.d2h_bytes()] + [c.d2h_bytes() for c in shard_ctxs]
            model = rr.Rebalance(sizes_of(S1), ns, old_map[0])
            cache[(kind, ns, arm)] = dict(U1=U1, S1=S1, R=R, moved=moved, model=model, before=before, old_images=old_images, old_map=old_map,
                                          d2h=d2h, d2h_after=d2h_after)
        return cache[(kind, ns, arm)]

    yield get
    cache.clear()


def identity_perm(sizes):
    return np.concatenate([np.arange(n) for n in sizes] + [np.zeros(0, np.int64)])


def check_requests(kind, R, others, sizes, ctxs, what):
    """every request on R returns what it returns on each of `others` (the old sharded object, the unsharded one)"""
    home, shard_ctxs = ctxs
    got_all = decode_all_guarded(R)
    ids_r, off_r = R.decode_lists(REQUEST)
    lists, slot, off_i = gather_request(sizes, np.random.default_rng(5))
    before = sum_d2h(home, shard_ctxs)
    got_gather = R.decode_gather(lists, slot, off_i)
    assert sum_d2h(home, shard_ctxs) - before == 8 * slot.size
    for O in others:
        assert np.array_equal(got_all, O.decode_all().cpu().numpy()), f"{what}: decode_all"
        ids_o, off_o = O.decode_lists(REQUEST)
        assert np.array_equal(off_r, off_o) and np.array_equal(ids_r.cpu().numpy(), ids_o.cpu().numpy()), f"{what}: decode_lists"
        assert np.array_equal(got_gather, O.decode_gather(lists, slot, off_i)), f"{what}: decode_gather"
    got, invalid = check_translate(others[-1], R, all_labels(sizes))
    assert invalid == 2 * len(sizes) + 4 and (got >= 0).sum() == int(np.sum(sizes)), f"{what}: translate_labels"
    if kind != "packed":
        assert np.array_equal(R.perm(), identity_perm(sizes)), f"{what}: the permutation is not the identity inside every list"


# ------------------------------------------------------------------------------------------------- 1. the map, loads, moved_ids, sizes
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_map_is_the_fresh_encodes_and_the_sizes_stay(rebalanced, kind, ns, arm):
    from vector_db_id_compression_amd.sharding import lpt_partition

    a = rebalanced(kind, ns, arm)
    R, S1, m = a["R"], a["S1"], a["model"]
    assert np.array_equal(R.owner, lpt_partition(sizes_of(S1), ns)), "the map is not the one a fresh encode chooses"
    assert np.array_equal(R.owner, m.new_owner) and np.array_equal(R.local_no, m.new_local)
    assert np.array_equal(R.loads, m.loads.astype(np.uint64)) and int(R.loads.sum()) == R.ntotal
    assert a["moved"] == m.moved_ids
    assert (a["moved"] > 0) == (ns > 1), "beyond one shard both updates change the map (tests/test_shards_rebalance_cpu.py)"
    assert R.nshards == ns and R.nlist == S1.nlist and R.ntotal == S1.ntotal == a["U1"].ntotal
    assert np.array_equal(R.offsets, S1.offsets)
    assert R.compressed_bytes == S1.compressed_bytes == a["U1"].compressed_bytes
    # the old object keeps its map
    owner, local, loads = a["old_map"]
    assert np.array_equal(S1.owner, owner) and np.array_equal(S1.local_no, local) and np.array_equal(S1.loads, loads)
    assert np.array_equal(owner, rr.f_owner(ns))


# ------------------------------------------------------------------------------------------------------------------ 2. shard parity
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_shard_is_the_single_object_of_the_new_cut(rebalanced, kind, ns, arm):
    a = rebalanced(kind, ns, arm)
    R, m = a["R"], a["model"]
    off = np.asarray(R.offsets).astype(np.int64)
    ids = a["before"].view(np.uint64)
    got = shard_images(kind, R)
    for d, mine in enumerate(m.new_lists):
        what = f"{kind}, {ns} shards, {arm}, shard {d}"
        if mine.size == 0:
            assert got[d] is None, "a shard that owns no list holds no object"
            continue
        cut = np.concatenate([ids[off[l]: off[l + 1]] for l in mine])
        loff = np.concatenate([[0], np.cumsum(m.sizes[mine])]).astype(np.uint64)
        single = encode_single(kind, loff, cut, 14)  # (packed: the object's width is kept)
        want = image(kind, single)
        if kind != "packed":
            want["perm"] = single.perm()
            assert np.array_equal(want["perm"], identity_perm(m.sizes[mine])), what
        assert_same_image(got[d], want, what)
        if kind == "packed":
            assert R.shard(d).bits == 14


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("ns", NSHARDS)
def test_a_roc_list_is_its_old_owners_list(rebalanced, ns, arm):
    """all five metadata values and every word, list by list through both maps"""
    a = rebalanced("roc", ns, arm)
    m, old, new = a["model"], a["old_images"], shard_images("roc", a["R"], with_perm=False)

    def word_off(img):
        return np.concatenate([[0], np.cumsum(img["nwords"], dtype=np.int64)])

    for l in range(rr.NLIST):
        so, ko, sn, kn = int(m.old_owner[l]), int(m.old_local[l]), int(m.new_owner[l]), int(m.new_local[l])
        for key in ("sizes", "precision", "heads", "nwords", "mt_draws"):
            assert old[so][key][ko] == new[sn][key][kn], f"list {l}: {key}"
        wo, wn = word_off(old[so]), word_off(new[sn])
        assert np.array_equal(old[so]["words"][wo[ko]: wo[ko + 1]], new[sn]["words"][wn[kn]: wn[kn + 1]]), f"list {l}: words"


# ----------------------------------------------------------------------------------------------------------------------- 3. requests
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_requests_answer_as_on_the_old_object_and_as_on_the_unsharded_one(ctxs, rebalanced, kind, ns, arm):
    a = rebalanced(kind, ns, arm)
    assert set(a["R"].owner[REQUEST]) == set(range(ns))
    check_requests(kind, a["R"], [a["S1"], a["U1"]], a["model"].sizes, ctxs, f"{kind}, {ns} shards, {arm}")


# ------------------------------------------------------------------------------------------------------ 4. residency, immutability
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_no_id_payload_crosses_pcie_and_the_old_object_is_untouched(rebalanced, kind, ns, arm):
    a = rebalanced(kind, ns, arm)
    regroups = sum(mine.size > 0 for mine in a["model"].new_lists) if kind == "roc" else 0
    grown = [y - x for x, y in zip(a["d2h"], a["d2h_after"])]
    assert min(grown) >= 0 and sum(grown) <= 8 * regroups, "a context's vidc_ctx_d2h_bytes moved by more than the word-total read-backs"
    assert np.array_equal(decode_all_guarded(a["S1"]), a["before"])
    for s, (got, want) in enumerate(zip(shard_images(kind, a["S1"], with_perm=False), a["old_images"])):
        assert (got is None) == (want is None)
        if got is not None:
            assert_same_image(got, want, f"the old object's shard {s}")


@pytest.mark.parametrize("kind", KINDS)
def test_either_object_may_be_destroyed_first(ctxs, rebalanced, F, kind):
    home, shard_ctxs = ctxs
    a = rebalanced(kind, 3, "append")
    want = a["before"]
    S1 = update(encode_s(kind, F[0], F[1], home, shard_ctxs[:3]), kind, 3, "append", F)
    R, _ = rebalance(S1, kind)
    del R
    gc.collect()
    assert np.array_equal(decode_all_guarded(S1), want), "the old object after the new one was dropped"
    R, moved = rebalance(S1, kind)
    del S1
    gc.collect()
    assert moved == a["moved"]
    assert np.array_equal(decode_all_guarded(R), want), "the new object after the old one was dropped"
    check_translate(a["U1"], R, all_labels(a["model"].sizes))


# ------------------------------------------------------------------------------------------------------------------- 5. chaining
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_second_rebalance_moves_nothing(rebalanced, kind, ns):
    a = rebalanced(kind, ns, "append")
    R2, moved = rebalance(a["R"], kind)
    assert moved == 0
    assert np.array_equal(R2.owner, a["R"].owner) and np.array_equal(R2.local_no, a["R"].local_no) and np.array_equal(R2.loads, a["R"].loads)
    for s, (got, want) in enumerate(zip(shard_images(kind, R2), shard_images(kind, a["R"]))):
        assert (got is None) == (want is None)
        if got is not None:
            assert_same_image(got, want, f"{kind}, {ns} shards: shard {s} of the second rebalance")


@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("kind", KINDS)
def test_append_rebalance_append_is_the_unsharded_double_append(ctxs, rebalanced, kind, ns):
    a = rebalanced(kind, ns, "append")
    ln, add = rr.second_batch()
    U2, lab_u, inv_u = append_to(a["U1"], ln, add, kind)
    N2, lab_n, inv_n = append_to(a["R"], ln, add, kind)
    assert inv_n == inv_u == 0 and np.array_equal(lab_n, lab_u)
    assert np.array_equal(N2.owner, a["R"].owner), "an append keeps the re-balanced map"
    sizes = a["model"].sizes + np.bincount(ln, minlength=rr.NLIST)
    assert np.array_equal(sizes_of(N2), sizes)
    home, shard_ctxs = ctxs
    assert np.array_equal(decode_all_guarded(N2), U2.decode_all().cpu().numpy())
    ids_u, off_u = U2.decode_lists(REQUEST)
    ids_n, off_n = N2.decode_lists(REQUEST)
    assert np.array_equal(off_n, off_u) and np.array_equal(ids_n.cpu().numpy(), ids_u.cpu().numpy())
    check_translate(U2, N2, all_labels(sizes))
    lists, slot, off_i = gather_request(sizes, np.random.default_rng(5))
    assert np.array_equal(N2.decode_gather(lists, slot, off_i), U2.decode_gather(lists, slot, off_i))
    if kind != "packed":
        assert np.array_equal(N2.perm(), U2.perm())


# --------------------------------------------------------------------------------------------------------- 6. shards without lists
@pytest.mark.parametrize("kind", KINDS)
def test_five_lists_at_eight_shards(ctxs, kind):
    """three shards own nothing before and after; the batch grows the empty list past every other, so owners change"""
    from vector_db_id_compression_amd.sharding import DeviceShards, lpt_partition

    home, shard_ctxs = ctxs
    sizes = np.array([4, 0, 9, 1, 1])
    off, ids = csr(sizes, seed=7)
    ids = 17 + 2 * ids  # (odd: no list's largest id is a power of two, where the reference ROC codec is lossy)
    ln = np.array([1] * 30 + [4, 4], np.int64)
    add = 101 + 2 * np.arange(ln.size, dtype=np.uint64)
    args = {"bits": 8} if kind == "packed" else {"want_perm": True}
    U1 = append_to(encode_single(kind, off, ids, 8), ln, add, kind, bits=8 if kind == "packed" else None)[0]
    S = DeviceShards.encode(kind, off, dev(ids), ctxs=shard_ctxs, home=home, **args)
    S1 = append_to(S, ln, add, kind)[0]
    R, moved = rebalance(S1, kind)
    m = rr.Rebalance(sizes + np.bincount(ln, minlength=5), 8, lpt_partition(sizes, 8))
    assert np.array_equal(R.owner, m.new_owner) and np.array_equal(R.local_no, m.new_local) and moved == m.moved_ids > 0
    assert np.array_equal(R.loads, m.loads.astype(np.uint64))
    for s in range(8):
        assert (R.shard(s) is None) == (m.new_lists[s].size == 0)
    assert sum(R.shard(s) is None for s in range(8)) == 3 and sum(S1.shard(s) is None for s in range(8)) == 3
    assert R.compressed_bytes == U1.compressed_bytes
    want = U1.decode_all().cpu().numpy()
    assert np.array_equal(decode_all_guarded(R), want) and np.array_equal(decode_all_guarded(S1), want)
    check_translate(U1, R, all_labels(m.sizes))
    if kind != "packed":
        assert np.array_equal(R.perm(), identity_perm(m.sizes))


# ----------------------------------------------------------------------------------------------------------------------- 7. errors
def test_another_home_context_is_refused(ctxs, rebalanced):
    home, shard_ctxs = ctxs
    L = _L()
    a = rebalanced("roc", 2, "append")
    out, moved = ctypes.c_void_p(1), ctypes.c_uint64(77)
    st = L.lib().vidc_rebalance_sharded(shard_ctxs[0].h, a["S1"].h, 0, ctypes.byref(out), ctypes.byref(moved))
    assert st == -1 and out.value is None and moved.value == 77 and b"home" in L.lib().vidc_last_error()
    assert np.array_equal(decode_all_guarded(a["S1"]), a["before"])


# ---------------------------------------------------------------------------------------------------------------- 8. second device
@pytest.mark.parametrize("kind", KINDS)
def test_a_shard_on_a_second_device(rebalanced, F, kind):
    """the far-source path of the ROC re-balance (a temporary object on the source's context, its clone on the destination's) and the
    far shards of the rebuild: needs two GPUs, so it has never run"""
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    L = _L()
    torch.cuda.set_device(0)
    home = L.Context(0)
    shard_ctxs = [L.Context(0), L.Context(1), L.Context(1)]
    a = rebalanced(kind, 3, "append")
    S1 = update(encode_s(kind, F[0], F[1], home, shard_ctxs), kind, 3, "append", F)
    R, moved = rebalance(S1, kind)
    assert moved == a["moved"] and np.array_equal(R.owner, a["model"].new_owner)
    assert np.array_equal(decode_all_guarded(R), a["U1"].decode_all().cpu().numpy())
    check_translate(a["U1"], R, all_labels(a["model"].sizes))
    for s, (got, want) in enumerate(zip(shard_images(kind, R), shard_images(kind, a["R"]))):
        assert_same_image(got, want, f"{kind}, two devices: shard {s}")
