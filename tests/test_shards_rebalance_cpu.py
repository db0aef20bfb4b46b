"""CPU: vidc_roc_regroup and vidc_rebalance_sharded (include/vidc.h) without a device -- the symbols are declared, listed and exported and
sit in neither pinned prefix set; the argument checks return VIDC_ERR_INVALID with *out == NULL before any device work; the batches the
GPU tests skew family F with change the map; shardplan::regroup_plan is built with g++ as a stand-alone program and compared with the
numpy model (tests/rebalance_ref.py), once more under -fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rebalance_ref as rr
from test_shards_cpu import F_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vidc_roc_regroup", "vidc_rebalance_sharded"]
NSHARDS = [1, 2, 3, 8]
INVALID = -1


def test_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    dll = ctypes.CDLL(build.build())
    for sym in NEW:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    assert not NEW[1].startswith(("vidc_shards_", "vidc_sharded_")), "those two sets are pinned by the sharding tests"
    assert "vidc_rebalance_sharded" in hdr.split("sharded lists (several contexts, one process)")[1]
    assert "vidc_roc_regroup" in hdr.split("sharded lists (several contexts, one process)")[0]
    assert "full re-encode" not in hdr, "the append's advice points to the re-balance now"
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays
    from vector_db_id_compression_amd import codecs
    from vector_db_id_compression_amd.sharding import DeviceShards

    assert callable(codecs.roc_regroup) and callable(DeviceShards.rebalance)
    assert not hasattr(codecs.RocLists, "regroup"), "the method set of the list classes is pinned (tests/test_gpu_call_contract.py)"


def test_regroup_argument_checks_need_no_device():
    """The table is checked against nsrc and the source pointers before any source is looked into, and the sources (zeroed host memory
    stands in: no list, device 0) before the device is touched."""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    fake = [ctypes.create_string_buffer(4096) for _ in range(3)]
    ctx, a, b = (ctypes.addressof(x) for x in fake)
    sn = np.array([0, 1, 0], np.uint32)
    ln = np.zeros(3, np.uint64)

    def call(ctx_, nsrc, srcs, m, sn_, ln_, with_out=True):
        arr = None if srcs is None else (ctypes.c_void_p * max(len(srcs), 1))(*srcs)
        out = ctypes.c_void_p(1)
        st = L.vidc_roc_regroup(ctx_, nsrc, arr, m, _lib.ptr(sn_), _lib.ptr(ln_), 0, ctypes.byref(out) if with_out else None)
        if with_out:
            assert out.value is None, "*out must be NULL on an error"
        return st

    assert call(None, 2, [a, b], 3, sn, ln) == INVALID
    assert call(ctx, 2, None, 3, sn, ln) == INVALID
    assert call(ctx, 2, [a, b], 3, sn, ln, with_out=False) == INVALID
    assert call(ctx, 2, [a, b], 3, None, ln) == INVALID
    assert call(ctx, 2, [a, b], 3, sn, None) == INVALID
    assert b"NULL" in L.vidc_last_error()
    for nsrc in (0, 9, -1):
        assert call(ctx, nsrc, [a, b] + [a] * 7, 3, sn, ln) == INVALID
        assert b"nsrc" in L.vidc_last_error()
    assert call(ctx, 1, [a, b], 3, sn, ln) == INVALID  # src_no 1 with one source
    assert b"names source 1 of 1" in L.vidc_last_error()
    assert call(ctx, 2, [a, None], 3, sn, ln) == INVALID  # a NULL source that is named
    assert b"which is NULL" in L.vidc_last_error()
    assert call(ctx, 2, [a, b], 2 ** 32, sn, ln) == INVALID
    # a list number outside its source (the zeroed stand-in holds no list)
    assert call(ctx, 2, [a, b], 3, sn, ln) == INVALID
    assert b"names list 0 of source 0, which holds 0" in L.vidc_last_error()


def test_rebalance_argument_checks_need_no_device():
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    fake = [ctypes.create_string_buffer(4096) for _ in range(2)]
    home, obj = (ctypes.addressof(x) for x in fake)

    def call(home_, obj_, with_out=True):
        out, moved = ctypes.c_void_p(1), ctypes.c_uint64(77)
        st = L.vidc_rebalance_sharded(home_, obj_, 0, ctypes.byref(out) if with_out else None, ctypes.byref(moved))
        if with_out:
            assert out.value is None, "*out must be NULL on an error"
        assert moved.value == 77, "moved_ids is written on success only"
        return st

    assert call(None, obj) == INVALID
    assert call(home, None) == INVALID
    assert call(home, obj, with_out=False) == INVALID
    assert b"NULL" in L.vidc_last_error()
    assert call(home, obj) == INVALID  # a foreign home: the zeroed stand-in was built with no context
    assert b"not the home context" in L.vidc_last_error()


# ------------------------------------------------------------------------------------------------ the batches of the GPU tests
@pytest.mark.parametrize("ns", NSHARDS)
def test_the_skew_batch_changes_the_map(ns):
    ln, ids = rr.skew_batch(ns)
    old = rr.f_owner(ns)
    assert ln.size == ids.size == 900 and np.unique(ids).size == 900 and int(ids.min()) == rr.NTOTAL and int(ids.max()) < 2 ** 14
    assert (old[ln] == rr.skew_shard(ns)).all(), "every pair goes to a list of one shard"
    m = rr.Rebalance(rr.grown_sizes(ns), ns, old)
    assert int(m.sizes.sum()) == rr.NTOTAL + 900 and int(m.loads.sum()) == rr.NTOTAL + 900
    if ns == 1:
        assert m.moved_ids == 0 and np.array_equal(m.new_owner, old)
        return
    assert not np.array_equal(m.new_owner, old) and m.moved_ids > 0
    arrive, leave = m.arrivals_and_departures()
    assert arrive.max() >= 1 and leave.max() >= 1, "a list arrives at some shard and a list leaves some shard"
    # the same for the remove of a third of shard 0's ids
    from test_shards_append_cpu import family_f

    off, f_ids = family_f()
    rln, rids = rr.remove_batch(off, f_ids, ns)
    shrunk = rr.shrunk_sizes(off, ns)
    assert np.array_equal(np.bincount(rln, minlength=rr.NLIST), np.asarray(F_SIZES) - shrunk) and (old[rln] == 0).all()
    assert np.unique(rids).size == rids.size
    r = rr.Rebalance(shrunk, ns, old)
    assert not np.array_equal(r.new_owner, old) and r.moved_ids > 0


def test_rows_of_the_model_name_every_list_once():
    m = rr.Rebalance(rr.grown_sizes(3), 3, rr.f_owner(3))
    seen = np.zeros(rr.NLIST, np.int64)
    for d, (src, lst) in enumerate(m.rows):
        for s, k, g in zip(src, lst, m.new_lists[d]):
            assert m.old_lists[s][k] == g
            seen[g] += 1
    assert (seen == 1).all()


# ------------------------------------------------------------------------------------------------ the plan program
def _fmt(*parts):
    out = []
    for p in parts:
        out.extend(str(int(x)) for x in np.asarray(p).reshape(-1))
    return " ".join(out)


def regroup_case(sizes, ns, old_owner):
    m = rr.Rebalance(sizes, ns, old_owner)
    line = ["REGROUP", _fmt(ns, len(m.sizes), m.sizes, m.old_owner, m.new_owner, m.moved_ids)]
    for d, (src, lst) in enumerate(m.rows):
        line.append(_fmt(src.size, src, lst, m.loads[d]))
    return " ".join(line)


@pytest.fixture(scope="module")
def regroup_cases_file(tmp_path_factory):
    from vector_db_id_compression_amd.sharding import lpt_partition

    rng = np.random.default_rng(31)
    lines = []
    for ns in NSHARDS:
        lines.append(regroup_case(rr.grown_sizes(ns), ns, rr.f_owner(ns)))
        lines.append(regroup_case(F_SIZES, ns, rr.f_owner(ns)))  # a map that does not change
    five = np.array([4, 0, 9, 1, 1])
    lines.append(regroup_case(five, 8, lpt_partition(five, 8)))
    lines.append(regroup_case(five + [0, 30, 0, 0, 2], 8, lpt_partition(five, 8)))  # shards without lists before and after
    lines.append(regroup_case([], 2, []))
    for _ in range(1000):
        nlist = int(rng.integers(1, 120))
        sizes = np.minimum(rng.zipf(1.3, nlist), 5000) * (rng.random(nlist) < 0.9)
        ns = int(rng.integers(1, 9))
        old = lpt_partition(sizes, ns) if rng.random() < 0.7 else rng.integers(0, ns, nlist)
        drift = sizes + rng.integers(0, 400, nlist) * (rng.random(nlist) < 0.3)
        lines.append(regroup_case(drift, ns, old))
    path = tmp_path_factory.mktemp("shard_regroup") / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), len(lines)


@pytest.mark.parametrize("sanitize", [False, True])
def test_shard_regroup_program(tmp_path, regroup_cases_file, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path, ncases = regroup_cases_file
    exe = str(tmp_path / "shard_regroup_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "shard_regroup_test.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and f"shard regroup ok: {ncases} cases" in out.stdout, out.stdout + out.stderr
