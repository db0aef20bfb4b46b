"""CPU: vidc_shards (include/vidc.h) without a device -- the symbols are declared, listed and exported; the argument checks return
VIDC_ERR_INVALID before any device work; the host plan (csrc/shard_plan.h) is built with g++ as a stand-alone program and compared with
values computed here from sharding.lpt_partition and numpy, once more under -fsanitize=address,undefined."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 1024  # shardplan::SHARD_COPY_UNIT

# family F of the GPU tests: 37 lists, 15 404 ids
F_SIZES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 0, 1023, 1024, 1025, 3000, 7, 0, 5, 64, 64, 64, 1, 1, 255, 256, 257, 511, 512, 513, 0,
           2047, 2048, 2049, 31, 32, 33, 0]

SHARDS = ["vidc_shards_encode", "vidc_shards_encode_dev", "vidc_shards_destroy", "vidc_shards_count", "vidc_shards_kind",
          "vidc_shards_nlist", "vidc_shards_ntotal", "vidc_shards_compressed_bytes", "vidc_shards_map", "vidc_shards_offsets",
          "vidc_shards_shard", "vidc_shards_shard_ctx", "vidc_shards_decode_all", "vidc_shards_decode_lists",
          "vidc_shards_translate_labels_dev", "vidc_shards_decode_gather", "vidc_shards_perm"]


def test_shards_symbols_declared_listed_and_exported():
    from vector_db_id_compression_amd import _lib, build

    hdr = open(os.path.join(ROOT, "include", "vidc.h")).read()
    declared = set(re.findall(r"\b(vidc_[a-z0-9_]+)\s*\(", hdr))
    assert {d for d in declared if d.startswith("vidc_shards_")} == set(SHARDS)
    dll = ctypes.CDLL(build.build())
    for sym in SHARDS:
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        assert hasattr(dll, sym), sym
    for name, val in (("VIDC_KIND_PACKED", 0), ("VIDC_KIND_EF", 1), ("VIDC_KIND_ROC", 2), ("VIDC_SHARDS_MAX", 8)):
        assert re.search(rf"#define {name}\s+{val}\b", hdr), name
        assert getattr(_lib, name) == val
    assert _lib.lib().vidc_version() == 100  # the ABI grows, its version stays


def test_argument_checks_need_no_device():
    """NULL arguments, nshards 0 or 9, a repeated context, an unknown kind: VIDC_ERR_INVALID.  The contexts are never looked into before
    these checks have passed, so addresses of plain host memory stand in for them."""
    from vector_db_id_compression_amd import _lib

    L = _lib.lib()
    INVALID, UNSUPPORTED = -1, -6
    fake = [ctypes.create_string_buffer(64) for _ in range(10)]
    addr = [ctypes.addressof(b) for b in fake]
    home = addr[9]
    off = np.array([0, 2, 5], np.uint64)
    ids = ctypes.addressof(ctypes.create_string_buffer(64))

    def ctxs(*a):
        return (ctypes.c_void_p * len(a))(*a)

    def enc(home_, n, arr, kind, offsets, d_ids, with_out=True):
        out = ctypes.c_void_p(1)
        st = L.vidc_shards_encode(home_, n, arr, kind, 0, 0, 2, offsets, d_ids, ctypes.byref(out) if with_out else None)
        if with_out:
            assert out.value is None, "*out must be NULL on an error"
        return st

    two = ctxs(addr[0], addr[1])
    assert enc(None, 2, two, 0, _lib.ptr(off), ids) == INVALID
    assert enc(home, 2, None, 0, _lib.ptr(off), ids) == INVALID
    assert enc(home, 2, two, 0, None, ids) == INVALID
    assert enc(home, 2, two, 0, _lib.ptr(off), ids, with_out=False) == INVALID
    assert enc(home, 2, ctxs(addr[0], None), 0, _lib.ptr(off), ids) == INVALID
    assert b"NULL" in L.vidc_last_error()
    assert enc(home, 0, two, 0, _lib.ptr(off), ids) == INVALID
    assert enc(home, 9, ctxs(*addr[:9]), 0, _lib.ptr(off), ids) == INVALID
    assert b"nshards" in L.vidc_last_error()
    assert enc(home, 3, ctxs(addr[0], addr[1], addr[0]), 0, _lib.ptr(off), ids) == INVALID
    assert b"same context" in L.vidc_last_error()
    for kind in (-1, 4, 99):
        assert enc(home, 2, two, kind, _lib.ptr(off), ids) == INVALID
        assert b"kind" in L.vidc_last_error()
    # the wavelet tree is a known kind, and refused
    assert enc(home, 2, two, _lib.VIDC_KIND_WT, _lib.ptr(off), ids) == UNSUPPORTED
    # the device-offsets form makes the same checks
    out = ctypes.c_void_p(1)
    assert L.vidc_shards_encode_dev(home, 9, ctxs(*addr[:9]), 0, 0, 0, 2, ids, 5, ids, ctypes.byref(out)) == INVALID and out.value is None
    assert L.vidc_shards_encode_dev(None, 2, two, 0, 0, 0, 2, ids, 5, ids, ctypes.byref(out)) == INVALID
    # requests and accessors on NULL
    assert L.vidc_shards_decode_all(None, None, None) == INVALID
    assert L.vidc_shards_decode_lists(None, None, 0, None, None, None) == INVALID
    assert L.vidc_shards_translate_labels_dev(None, None, 0, None, None, None) == INVALID
    assert L.vidc_shards_decode_gather(None, None, 0, None, 0, None, None, None) == INVALID
    assert L.vidc_shards_perm(None, None, None) == INVALID
    assert L.vidc_shards_count(None) == 0 and L.vidc_shards_kind(None) == -1
    assert L.vidc_shards_shard(None, 0) is None and L.vidc_shards_shard_ctx(None, 0) is None
    L.vidc_shards_destroy(None)


# ------------------------------------------------------------------------------------------------ the plan program
def plan_model(sizes, ns):
    """owner, local numbers, and per shard (lists, local offsets, cut segments) from lpt_partition and numpy"""
    from vector_db_id_compression_amd.sharding import lpt_partition

    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    owner = lpt_partition(sizes, ns)
    local = np.zeros(sizes.size, np.int64)
    shards = []
    for s in range(ns):
        mine = np.nonzero(owner == s)[0]
        local[mine] = np.arange(mine.size)
        loff = np.concatenate([[0], np.cumsum(sizes[mine])]).astype(np.int64)
        nz = sizes[mine] > 0
        segs = np.stack([off[mine][nz], loff[:-1][nz], sizes[mine][nz]], 1) if mine.size else np.zeros((0, 3), np.int64)
        shards.append((mine, loff, segs))
    return off, owner, local, shards


def _fmt(*parts):
    out = []
    for p in parts:
        out.extend(str(int(x)) for x in np.asarray(p).reshape(-1))
    return " ".join(out)


def plan_case(sizes, ns):
    off, owner, local, shards = plan_model(sizes, ns)
    line = ["PLAN", _fmt(ns, len(sizes), sizes, owner, local)]
    for mine, loff, segs in shards:
        line.append(_fmt(mine.size, loff, segs.shape[0], segs, int(((segs[:, 2] + UNIT - 1) // UNIT).sum())))
    return " ".join(line)


def route_case(sizes, ns, req):
    off, owner, local, shards = plan_model(sizes, ns)
    sizes = np.asarray(sizes, np.int64)
    req = np.asarray(req, np.int64)
    out_off = np.concatenate([[0], np.cumsum(sizes[req])]).astype(np.int64)
    line = ["ROUTE", _fmt(ns, sizes.size, sizes, req.size, req, out_off)]
    for s in range(ns):
        items = np.nonzero(owner[req] == s)[0]
        n = sizes[req[items]]
        staged = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        nz = n > 0
        segs = np.stack([staged[:-1][nz], out_off[items][nz], n[nz]], 1) if items.size else np.zeros((0, 3), np.int64)
        line.append(_fmt(items.size, local[req[items]], segs.shape[0], segs, staged[-1]))
    return " ".join(line)


def gather_case(sizes, ns, req, slot, offs, rc=0, bad=0):
    off, owner, local, shards = plan_model(sizes, ns)
    req, slot, offs = (np.asarray(a, np.int64) for a in (req, slot, offs))
    line = ["GATHER", _fmt(ns, len(sizes), sizes, req.size, req, slot.size, slot, offs, rc, bad)]
    if rc == 0:
        slot_local = np.zeros(req.size, np.int64)
        for s in range(ns):
            mentions = np.nonzero(owner[req] == s)[0]
            slot_local[mentions] = np.arange(mentions.size)
        for s in range(ns):
            mentions = np.nonzero(owner[req] == s)[0]
            items = np.nonzero(owner[req[slot]] == s)[0]
            line.append(_fmt(mentions.size, local[req[mentions]], items.size, slot_local[slot[items]], offs[items], items))
    return " ".join(line)


def zipf_sizes(rng):
    nlist = int(rng.integers(1, 121))
    w = 1.0 / np.arange(1, nlist + 1) ** rng.uniform(0.5, 1.5)
    sizes = rng.multinomial(int(rng.integers(0, 40000)), w / w.sum())
    return rng.permutation(sizes)


@pytest.fixture(scope="module")
def cases_file(tmp_path_factory):
    rng = np.random.default_rng(15)
    lines = [plan_case(F_SIZES, ns) for ns in (1, 2, 3, 8)]
    lines.append(plan_case([4, 0, 9, 1, 1], 8))
    lines.append(plan_case([3000], 2))
    lines.append(plan_case([0, 0, 0], 3))
    lines.append(plan_case([], 2))
    for _ in range(1000):
        lines.append(plan_case(zipf_sizes(rng), int(rng.integers(1, 9))))
    # a routed request: lists of every shard, repeats, the empty lists, the 3000-id list
    req = [14, 0, 36, 14, 5, 5, 10, 31, 1, 2, 3, 29, 12, 35, 16, 20, 19, 18, 32, 14]
    for ns in (1, 2, 3, 8):
        lines.append(route_case(F_SIZES, ns, req))
        lines.append(route_case(F_SIZES, ns, rng.integers(0, len(F_SIZES), 200)))
    lines.append(route_case([4, 0, 9, 1, 1], 8, [1, 2, 2, 0, 4, 3, 1]))
    lines.append("BADLIST " + _fmt(3, len(F_SIZES), F_SIZES, 4, [1, 2, 37, 99], 2))
    # gather: every mention is a slot of its owner's request; items go to the owner of their slot
    g_req = [14, 5, 14, 31, 12, 3]
    g_slot = [0, 2, 1, 3, 4, 5, 0, 0, 2, 4]
    g_off = [2999, 0, 63, 2047, 1023, 2, 17, 17, 1500, 0]
    for ns in (1, 2, 3, 8):
        lines.append(gather_case(F_SIZES, ns, g_req, g_slot, g_off))
    lines.append(gather_case(F_SIZES, 3, [14, 40], [0], [0], rc=1, bad=1))
    lines.append(gather_case(F_SIZES, 3, g_req, [0, 6], [0, 0], rc=2, bad=1))       # a slot outside the request
    lines.append(gather_case(F_SIZES, 3, g_req, [0, 1, 5], [0, 63, 3], rc=2, bad=2))  # an offset equal to the list's size
    path = tmp_path_factory.mktemp("shard_plan") / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), len(lines)


def test_family_f_is_what_the_gpu_tests_count_on():
    from vector_db_id_compression_amd.sharding import lpt_partition

    sizes = np.asarray(F_SIZES, np.int64)
    assert sizes.size == 37 and sizes.sum() == 15404
    assert np.bincount(lpt_partition(sizes, 8), minlength=8).min() >= 1
    assert np.bincount(lpt_partition(sizes, 2), weights=sizes, minlength=2).tolist() == [7702, 7702]


@pytest.mark.parametrize("sanitize", [False, True])
def test_shard_plan_program(tmp_path, cases_file, sanitize):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    path, ncases = cases_file
    exe = str(tmp_path / "shard_plan_test")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:  # a stand-alone host program: the sanitizer runtimes are linked into it
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([gxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "shard_plan_test.cpp")])
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0 and f"shard plan ok: {ncases} cases" in out.stdout, out.stdout + out.stderr
