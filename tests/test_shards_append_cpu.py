"""CPU: appending to a sharded object (vidc_sharded_append_dev / vidc_sharded_loads, include/vidc.h) without a device -- the symbols are
declared, listed and exported; the argument checks return VIDC_ERR_INVALID before any device work; batch B of the GPU tests has the
properties those tests count on; the two statements of the contract (the cut of the merged lists by the OLD map == every shard's cut
merged with the pairs routed to it) agree in numpy; shardplan::make_plan_for_owner is built with g++ as a stand-alone program and compared
with values computed here, once more under -fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import append_ref as ar
from test_shards_cpu import F_SIZES, plan_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vidc_sharded_append_dev", "vidc_sharded_loads"]
NSHARDS = [1, 2, 3, 8]
NLIST, NTOTAL = 37, 15404


def family_f(seed=15):
    """family F as tests/test_gpu_shards.py builds it: a seeded permutation of 0 .. ntotal - 1 cut in list order"""
    off = np.concatenate([[0], np.cumsum(np.asarray(F_SIZES, np.int64))]).astype(np.uint64)
    return off, np.random.default_rng(seed).permutation(int(off[-1])).astype(np.uint64)


def batch_b():
    rng = np.random.default_rng(17)
    ln = rng.integers(-2, 40, 700)
    ids = 15404 + rng.permutation(700)
    return ln.astype(np.int64), ids.astype(np.uint64)


def batch_c():
    """the second batch of the chaining test: 280 valid pairs and 20 skipped ones, ids behind those of batch B"""
    rng = np.random.default_rng(18)
    ln = rng.integers(0, NLIST, 300).astype(np.int64)
    skip = rng.permutation(300)[:20]
    ln[skip[:10]], ln[skip[10:]] = -1, NLIST + 3
    ids = np.zeros(300, np.uint64)
    ids[ln_valid(ln)] = 16104 + rng.permutation(280)
    ids[~ln_valid(ln)] = 17000 + np.arange(20)
    return ln, ids


def ln_valid(ln):
    return (ln >= 0) & (ln < NLIST)


def route(ln, owner, local, s):
    """the local list numbers shard s sees: local_no where it owns the list, -1 elsewhere"""
    ok = ln_valid(ln)
    out = np.full(ln.size, -1, np.int64)
    mine = ok & (owner[np.where(ok, ln, 0)] == s)
    out[mine] = local[ln[mine]]
    return out


def cut(off, ids, mine):
    off = np.asarray(off, np.int64)
    return np.concatenate([ids[off[l]: off[l + 1]] for l in mine]) if len(mine) else np.zeros(0, np.uint64)


def test_append_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    assert {d for d in declared if d.startswith("vidc_sharded_")} == set(NEW)
    dll = ctypes.CDLL(build.build())
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays


def test_argument_checks_need_no_device():
    """NULL home / object / out, a NULL array with n_add > 0, n_add >= 2^32 - 1: VIDC_ERR_INVALID and *out == NULL.  Neither the context
    nor the object is looked into before these checks have passed, so addresses of plain host memory stand in for them."""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    INVALID = -1
    fake = [ctypes.create_string_buffer(4096) for _ in range(4)]
    home, obj, ln, ids = (ctypes.addressof(b) for b in fake)

    def app(home_, obj_, n, ln_, ids_, with_out=True):
        out = ctypes.c_void_p(1)
        st = L.vidc_sharded_append_dev(home_, obj_, n, ln_, ids_, 0, 0, ctypes.byref(out) if with_out else None, None, None)
        if with_out:
            assert out.value is None, "*out must be NULL on an error"
        return st

    assert app(None, obj, 4, ln, ids) == INVALID
    assert app(home, None, 4, ln, ids) == INVALID
    assert app(home, obj, 4, ln, ids, with_out=False) == INVALID
    assert app(home, obj, 4, None, ids) == INVALID
    assert app(home, obj, 4, ln, None) == INVALID
    assert b"NULL" in L.vidc_last_error()
    for n in (2 ** 32 - 1, 2 ** 32, 2 ** 40):
        assert app(home, obj, n, ln, ids) == INVALID
        assert b"2^32 - 1" in L.vidc_last_error()
    loads = np.zeros(8, np.uint64)
    assert L.vidc_sharded_loads(None, _lib.ptr(loads)) == INVALID
    assert L.vidc_sharded_loads(obj, None) == INVALID
    assert not loads.any()


def test_batch_b_is_what_the_gpu_tests_count_on():
    from vector_db_id_compression_amd import _lib

    ln, ids = batch_b()
    assert ln.size == ids.size == 700
    assert np.count_nonzero(ln < 0) == 45 and np.count_nonzero(ln >= NLIST) == 41
    per_list = np.bincount(ln[ln_valid(ln)], minlength=NLIST)
    assert per_list.size == NLIST and per_list.min() >= 10 and per_list.max() <= 26
    for l in range(NLIST):  # interleaved: no list's pairs sit next to one another as one run
        at = np.flatnonzero(ln == l)
        assert at[-1] - at[0] >= at.size
    _, owner, _, _ = plan_model(F_SIZES, 8)
    assert set(owner[ln[ln_valid(ln)]]) == set(range(8))
    assert int(ids.max()) == 16103 and int(ids.min()) == NTOTAL and np.unique(ids).size == 700
    assert _lib.lib().vidc_packed_bits_for(NTOTAL) == 14 and int(ids.max()) < 2 ** 14
    ln2, ids2 = batch_c()
    assert np.count_nonzero(ln_valid(ln2)) == 280 and np.array_equal(np.sort(ids2[ln_valid(ln2)]), 16104 + np.arange(280))


@pytest.mark.parametrize("ns", NSHARDS)
def test_the_two_statements_of_the_contract_agree(ns):
    """cutting M by the OLD owner map == merging each shard's cut with its routed, local-numbered pairs; the shards' labels, joined with
    the global list numbers, are M's labels; the loads are the sums of the owned lists' merged sizes"""
    off, ids = family_f()
    ln, add = batch_b()
    m = ar.merge(off, ids, ln, add)
    assert m.invalid == 41 and int(m.offsets[-1]) == NTOTAL + 700 - 45 - 41
    _, owner, local, shards = plan_model(F_SIZES, ns)
    sizes_new = (m.offsets[1:] - m.offsets[:-1]).astype(np.int64)
    want_lab = ar.labels("packed", m)
    joined = np.full(ln.size, -1, np.int64)
    for s, (mine, loff, _) in enumerate(shards):
        ms = ar.merge(loff.astype(np.uint64), cut(off, ids, mine), route(ln, owner, local, s), add)
        assert ms.invalid == 0, "a shard sees valid or negative local numbers only"
        assert np.array_equal(ms.offsets.astype(np.int64), np.concatenate([[0], np.cumsum(sizes_new[mine])]))
        assert np.array_equal(ms.ids, cut(m.offsets, m.ids, mine)), f"shard {s} of {ns}"
        lab = ar.labels("packed", ms)
        here = lab >= 0
        assert not (here & (joined >= 0)).any()
        joined[here] = (ln[here] << 32) | (lab[here] & 0xFFFFFFFF)
        assert np.array_equal(lab[here] >> 32, local[ln[here]])
    assert np.array_equal(joined, want_lab)


# ------------------------------------------------------------------------------------------------ the plan program
def owner_model(sizes, ns, owner):
    """plan_model for a GIVEN owner: local numbers, and per shard (lists, local offsets, cut segments)"""
    sizes = np.asarray(sizes, np.int64)
    owner = np.asarray(owner, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    local = np.zeros(sizes.size, np.int64)
    shards = []
    for s in range(ns):
        mine = np.nonzero(owner == s)[0]
        local[mine] = np.arange(mine.size)
        loff = np.concatenate([[0], np.cumsum(sizes[mine])]).astype(np.int64)
        nz = sizes[mine] > 0
        segs = np.stack([off[mine][nz], loff[:-1][nz], sizes[mine][nz]], 1) if mine.size else np.zeros((0, 3), np.int64)
        shards.append((mine, loff, segs))
    return local, shards


def _fmt(*parts):
    out = []
    for p in parts:
        out.extend(str(int(x)) for x in np.asarray(p).reshape(-1))
    return " ".join(out)


def owner_case(sizes, ns, owner, is_lpt):
    local, shards = owner_model(sizes, ns, owner)
    line = ["OWNER", _fmt(ns, len(sizes), sizes, owner, int(is_lpt), local)]
    for mine, loff, segs in shards:
        line.append(_fmt(mine.size, mine, loff, segs.shape[0], segs, loff[-1]))
    return " ".join(line)


@pytest.fixture(scope="module")
def owner_cases_file(tmp_path_factory):
    from vector_db_id_compression_amd.sharding import lpt_partition

    rng = np.random.default_rng(17)
    ln, add = batch_b()
    off, ids = family_f()
    grown = (ar.merge(off, ids, ln, add).offsets[1:] - ar.merge(off, ids, ln, add).offsets[:-1]).astype(np.int64)
    lines = []
    for ns in NSHARDS:
        _, owner, local, shards = plan_model(F_SIZES, ns)
        # the LPT owner: the numpy model for a given owner is plan_model, and make_plan is make_plan_for_owner of it
        got_local, got_shards = owner_model(F_SIZES, ns, owner)
        assert np.array_equal(got_local, local)
        for (a, b, c), (d, e, f) in zip(shards, got_shards):
            assert np.array_equal(a, d) and np.array_equal(b, e) and np.array_equal(c, f)
        lines.append(owner_case(F_SIZES, ns, owner, True))
        # what an append re-plans with: the OLD owner and the grown lists (no longer the LPT owner of those sizes in general)
        lines.append(owner_case(grown, ns, owner, np.array_equal(lpt_partition(grown, ns), owner)))
    # deliberately unbalanced owners, empty shards included
    n = len(F_SIZES)
    lines.append(owner_case(F_SIZES, 8, np.zeros(n, np.int64), False))                      # everything on shard 0, seven empty shards
    lines.append(owner_case(F_SIZES, 8, np.full(n, 7, np.int64), False))                   # everything on the last shard
    lines.append(owner_case(F_SIZES, 4, np.where(np.arange(n) == 14, 3, 1), False))        # shards 0 and 2 empty, the 3000-id list alone
    lines.append(owner_case(F_SIZES, 3, np.where(np.asarray(F_SIZES) == 0, 2, 0), False))  # a shard of empty lists only, an empty shard
    lines.append(owner_case([0, 0, 0], 3, [2, 2, 0], False))
    lines.append(owner_case([], 2, [], True))
    for _ in range(300):
        nlist = int(rng.integers(1, 80))
        sizes = rng.integers(0, 3000, nlist) * (rng.random(nlist) < 0.8)
        ns = int(rng.integers(1, 9))
        lines.append(owner_case(sizes, ns, rng.integers(0, ns, nlist), False))
        lines.append(owner_case(sizes, ns, lpt_partition(sizes, ns), True))
    path = tmp_path_factory.mktemp("shard_plan_owner") / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), len(lines)


@pytest.mark.parametrize("sanitize", [False, True])
def test_shard_plan_for_owner_program(tmp_path, owner_cases_file, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path, ncases = owner_cases_file
    exe = str(tmp_path / "shard_plan_owner_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "shard_plan_owner_test.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and f"shard plan for owner ok: {ncases} cases" in out.stdout, out.stdout + out.stderr
