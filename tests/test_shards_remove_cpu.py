"""CPU: removing from a sharded object (vidc_remove_sharded_dev, include/vidc.h) without a device -- the symbol is declared, listed and
exported; the argument checks return VIDC_ERR_INVALID before any device work; the inputs of the GPU tests (family G, batches P and A, the
emptying batch) have the properties those tests count on; and the statements of the contract agree in numpy: the cut of the global
model's survivors by the OLD map is every shard's own model, the inverse cut of the shards' masks is the global mask, the OR-join of the
shards' per-pair found flags gives the global missing count -- which the SUM of the shards' own missing counts does not."""
import ctypes
import os
import re

import numpy as np
import pytest

import remove_ref as rr
from test_shards_append_cpu import NLIST, NTOTAL, cut, ln_valid, route
from test_shards_cpu import F_SIZES, plan_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "vidc_remove_sharded_dev"
NSHARDS = [1, 2, 3, 8]
UNIVERSE = 4096
EMPTIED = 8  # the list batch P empties completely (128 ids)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def family_g(kind="packed", seed=23):
    """family G: the sizes of family F; list l holds a seeded sample WITHOUT replacement of its size from 0 .. 4095, in sample order
    (ascending for Elias-Fano).  Ids repeat across lists and across shards, never inside a list."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(F_SIZES, np.int64))]).astype(np.uint64)
    lists = [rng.permutation(UNIVERSE)[:n].astype(np.uint64) for n in F_SIZES]
    if kind == "ef":
        lists = [np.sort(l) for l in lists]
    return off, np.concatenate(lists)


def lists_of(off, ids):
    off = np.asarray(off).astype(np.int64)
    return [ids[off[l]: off[l + 1]] for l in range(off.size - 1)]


def batch_p():
    """pairs mode, about 600 pairs: up to 12 entries of every non-empty list, all of list EMPTIED, 60 pairs whose id sits only in
    ANOTHER list, 30 negative list numbers, 30 list numbers >= nlist, 40 repeats of earlier pairs -- shuffled"""
    rng = np.random.default_rng(29)
    off, ids = family_g()
    L = lists_of(off, ids)
    ln, rm = [], []
    for l, li in enumerate(L):
        take = li if l == EMPTIED else rng.permutation(li)[: min(li.size, 12)]
        ln += [l] * take.size
        rm += take.tolist()
    everywhere = np.unique(ids)
    n = 0
    while n < 60:  # an id that some list holds and list l does not
        l, x = int(rng.integers(0, NLIST)), int(everywhere[rng.integers(0, everywhere.size)])
        if x not in L[l]:
            ln.append(l)
            rm.append(x)
            n += 1
    ln += rng.integers(-5, 0, 30).tolist() + rng.integers(NLIST, NLIST + 9, 29).tolist() + [1 << 40]
    rm += rng.integers(0, UNIVERSE, 60).tolist()
    ln, rm = np.asarray(ln, np.int64), np.asarray(rm, np.uint64)
    again = rng.integers(0, ln.size, 40)
    ln, rm = np.concatenate([ln, ln[again]]), np.concatenate([rm, rm[again]])
    order = rng.permutation(ln.size)
    return ln[order], rm[order]


def held_by(ns):
    """bool[ns, 4096]: shard s of ns holds id x in some list"""
    off, ids = family_g()
    L = lists_of(off, ids)
    _, owner, _, _ = plan_model(F_SIZES, ns)
    held = np.zeros((ns, UNIVERSE), bool)
    for l, li in enumerate(L):
        held[owner[l], li.astype(np.int64)] = True
    return held


def batch_a():
    """any-list mode, about 300 ids: per shard count 2 / 3 / 8, 25 ids held by some shards and absent from others; 170 ids drawn from
    0 .. 4095; 24 ids of no list (4096 ..) and one >= 2^32; 30 repeats -- shuffled"""
    rng = np.random.default_rng(31)
    rm = []
    for ns in (2, 3, 8):
        held = held_by(ns)
        partial = np.flatnonzero(held.any(0) & ~held.all(0))
        rm += rng.permutation(partial)[:25].tolist()
    rm += rng.integers(0, UNIVERSE, 170).tolist()
    rm += (UNIVERSE + np.arange(24)).tolist() + [(1 << 32) + 7]
    rm = np.asarray(rm, np.uint64)
    rm = np.concatenate([rm, rm[rng.integers(0, 75, 10)], rm[rng.integers(245, 270, 10)], rm[rng.integers(0, rm.size, 10)]])
    return rng.permutation(rm)


def batch_empty():
    """any-list mode: every id a list of G can hold -- the whole object goes"""
    return np.random.default_rng(37).permutation(UNIVERSE).astype(np.uint64)


def roc_safe(off, ids):
    """no list has a power-of-two maximum, where the reference ROC codec is lossy under VIDC_PREC_REFERENCE (include/vidc.h)"""
    for li in lists_of(off, ids):
        if li.size and int(li.max()) > 0 and int(li.max()) & (int(li.max()) - 1) == 0:
            return False
    return True


def pair_found(off, ids, ln, rm):
    """the found byte of every pair for ONE object: 1 iff the pair is valid for it (pairs mode: 0 <= list < nlist) and its id sits in
    that list (any-list mode: in any list)"""
    rm = np.asarray(rm, np.uint64)
    if ln is None:
        return np.isin(rm, ids)
    L = lists_of(off, ids)
    return np.array([0 <= l < len(L) and x in L[l] for l, x in zip(ln.tolist(), rm.tolist())], bool)


def inverse_cut(segs_per_shard, masks, ntotal):
    """the global mask from the shards' masks: the cut segments (global start, shard start, count) read the other way round"""
    out = np.full(ntotal, 0xA5, np.uint8)
    for segs, m in zip(segs_per_shard, masks):
        for src, dst, cnt in segs:
            out[src: src + cnt] = m[dst: dst + cnt]
    return out


# ------------------------------------------------------------------------------------------------------------------- the symbol
def test_remove_symbol_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    assert NEW in declared
    assert "vidc_sharded_remove_dev" not in declared, "the name tests/test_remove_abi_cpu.py pins out"
    dll = ctypes.CDLL(build.build())
    assert NEW in _lib.EXPORTED_SYMBOLS and hasattr(dll, NEW)
    assert not any(hasattr(dll, s) for s in ("packed_remove", "ef_remove", "roc_remove")), "the internal entry points are C++ symbols"
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    assert "no sharded one" not in hdr


def test_argument_checks_need_no_device():
    """NULL home / object / out, NULL ids with n_rm > 0, n_rm >= 2^32 - 1: VIDC_ERR_INVALID, *out == NULL, "remove" in the message.
    Neither the context nor the object is looked into before these checks have passed, so addresses of plain host memory stand in."""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    INVALID = -1
    fake = [ctypes.create_string_buffer(4096) for _ in range(4)]
    home, obj, ln, ids = (ctypes.addressof(b) for b in fake)

    def rem(home_, obj_, n, ln_, ids_, with_out=True):
        out = ctypes.c_void_p(1)
        st = L.vidc_remove_sharded_dev(home_, obj_, n, ln_, ids_, 0, 0, ctypes.byref(out) if with_out else None, None, None, None)
        if with_out:
            assert out.value is None, "*out must be NULL on an error"
        assert b"remove" in L.vidc_last_error()
        return st

    assert rem(None, obj, 4, ln, ids) == INVALID
    assert rem(home, None, 4, ln, ids) == INVALID
    assert rem(home, obj, 4, ln, ids, with_out=False) == INVALID
    assert rem(home, obj, 4, ln, None) == INVALID
    assert rem(home, obj, 4, None, None) == INVALID
    assert b"NULL" in L.vidc_last_error()
    for n in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
        assert rem(home, obj, n, ln, ids) == INVALID
        assert rem(home, obj, n, None, ids) == INVALID
        assert b"2^32 - 1" in L.vidc_last_error()


def test_without_a_gpu_the_python_calls_fail_like_the_single_object_remove():
    import torch

    from vector_db_id_compression_amd import _lib, removal
    from vector_db_id_compression_amd.sharding import DeviceShards

    S = DeviceShards(None, None, [], 0)
    with pytest.raises(TypeError, match="unknown codec arguments"):  # (`bits` is the append's: a remove keeps the width)
        S.remove(None, np.arange(3, dtype=np.uint64), bits=3)
    if torch.cuda.is_available():
        return  # (with a device the calls run: tests/test_gpu_shards_remove.py)
    for call in (lambda: S.remove(None, np.arange(3, dtype=np.uint64)), lambda: removal.remove(S, None, np.arange(3, dtype=np.uint64))):
        with pytest.raises(_lib.VidcError, match="no HIP device: remove needs"):
            call()


# ------------------------------------------------------------------------------------------------------------------- the inputs
def test_family_g_is_what_the_gpu_tests_count_on():
    for kind in ("packed", "ef"):
        off, ids = family_g(kind)
        assert int(off[-1]) == NTOTAL == ids.size and off.size == NLIST + 1 and int(ids.max()) < UNIVERSE
        for li in lists_of(off, ids):
            assert np.unique(li).size == li.size, "an id repeats inside a list"
            if kind == "ef":
                assert (np.diff(li.astype(np.int64)) > 0).all()
        assert roc_safe(off, ids)
    a, b = family_g("packed")[1], family_g("ef")[1]
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.sort(b))
    # ids repeat across lists, and across shards at every shard count
    assert np.unique(a).size < a.size
    for ns in (2, 3, 8):
        assert (held_by(ns).sum(0) > 1).sum() > 1000


def test_batch_p_is_what_the_gpu_tests_count_on():
    off, ids = family_g()
    ln, rm = batch_p()
    assert ln.size == rm.size and 550 <= ln.size <= 650
    assert np.count_nonzero(ln < 0) >= 30 and np.count_nonzero(ln >= NLIST) >= 30
    g = rr.remove(off, ids, ln, rm)
    assert g.invalid == np.count_nonzero(ln >= NLIST)
    assert g.missing >= 60, "pairs whose id sits only in another list, and the random ids behind the skipped list numbers' places"
    L = lists_of(off, ids)
    other = [0 <= l < NLIST and x not in L[l] and x in ids for l, x in zip(ln.tolist(), rm.tolist())]
    assert sum(other) >= 60
    pairs = ln * (1 << 33) + rm.astype(np.int64)
    assert np.unique(pairs).size <= pairs.size - 40, "repeated pairs"
    new_sizes = (g.offsets[1:] - g.offsets[:-1]).astype(np.int64)
    assert F_SIZES[EMPTIED] == 128 and new_sizes[EMPTIED] == 0
    assert np.array_equal(new_sizes == 0, (np.asarray(F_SIZES) <= 12) | (np.arange(NLIST) == EMPTIED))  # (and the lists of up to 12 ids)
    _, owner, _, _ = plan_model(F_SIZES, 8)
    lost = np.asarray(F_SIZES) - new_sizes
    assert all(lost[owner == s].sum() > 0 for s in range(8)), "at 8 shards every shard loses something"
    assert 300 < g.removed < 500 and roc_safe(g.offsets, g.ids)


def test_batch_a_is_what_the_gpu_tests_count_on():
    off, ids = family_g()
    rm = batch_a()
    assert 280 <= rm.size <= 320
    for ns in (2, 3, 8):
        held = held_by(ns)
        small = rm[rm < UNIVERSE].astype(np.int64)
        partial = np.unique(small[held[:, small].any(0) & ~held[:, small].all(0)])
        assert partial.size >= 20, f"{ns} shards: ids held by some shards and absent from others"
    nowhere = np.unique(rm[~np.isin(rm, ids)])
    assert nowhere.size >= 20 and int(nowhere.max()) >= 2 ** 32 and np.count_nonzero(nowhere >= UNIVERSE) >= 20
    vals, counts = np.unique(rm, return_counts=True)
    rep = vals[counts > 1]
    assert np.isin(rep, ids).any() and (~np.isin(rep, ids)).any(), "repeats of both kinds"
    g = rr.remove(off, ids, None, rm)
    assert g.invalid == 0 and g.missing == np.count_nonzero(~np.isin(rm, ids)) >= 25 and roc_safe(g.offsets, g.ids)
    assert 0 < g.removed < NTOTAL


def test_the_emptying_batch_removes_the_whole_object():
    off, ids = family_g()
    g = rr.remove(off, ids, None, batch_empty())
    assert g.removed == NTOTAL and g.ids.size == 0 and not g.offsets.any() and g.missing == UNIVERSE - np.unique(ids).size


# ---------------------------------------------------------------------------------------------------------------- the contract
@pytest.mark.parametrize("ns", NSHARDS)
@pytest.mark.parametrize("mode", ["pairs", "any", "empty"])
def test_the_statements_of_the_contract_agree(mode, ns):
    off, ids = family_g()
    ln, rm = batch_p() if mode == "pairs" else (None, batch_a() if mode == "any" else batch_empty())
    g = rr.remove(off, ids, ln, rm)
    _, owner, local, shards = plan_model(F_SIZES, ns)
    new_sizes = (g.offsets[1:] - g.offsets[:-1]).astype(np.int64)
    masks, found, missing_sum = [], np.zeros(rm.size, bool), 0
    for s, (mine, loff, _) in enumerate(shards):
        routed = None if ln is None else route(ln, owner, local, s)
        mine_ids = cut(off, ids, mine)
        ms = rr.remove(loff.astype(np.uint64), mine_ids, routed, rm)
        assert ms.invalid == 0, "a shard sees valid or negative local numbers only"
        assert np.array_equal(ms.offsets.astype(np.int64), np.concatenate([[0], np.cumsum(new_sizes[mine])]))
        assert np.array_equal(ms.ids, cut(g.offsets, g.ids, mine)), f"shard {s} of {ns}"
        f = pair_found(loff, mine_ids, routed, rm)
        valid_here = np.ones(rm.size, bool) if routed is None else routed >= 0
        assert ms.missing == np.count_nonzero(valid_here & ~f), "the found bytes are the shard's own missing count, pair by pair"
        masks.append(ms.mask)
        found |= f
        missing_sum += ms.missing
    assert np.array_equal(inverse_cut([sg for _, _, sg in shards], masks, NTOTAL), g.mask)
    valid = np.ones(rm.size, bool) if ln is None else ln_valid(ln)
    assert np.count_nonzero(valid & ~found) == g.missing, "the OR-join of the found flags"
    if mode == "pairs":
        assert missing_sum == g.missing, "in pairs mode exactly one shard judges a pair"
    elif ns > 1:
        assert missing_sum != g.missing, "a join that sums the shards' own counts must be wrong here"
    else:
        assert missing_sum == g.missing
