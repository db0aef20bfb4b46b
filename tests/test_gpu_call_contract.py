"""The host frame of the C-ABI entry points (include/vidc.h), pinned from outside: what ctx.last_kernel_ms holds after a call, the lazy
host mirror of device offsets, what a rejected request leaves behind (status, vidc_last_error text, untouched outputs), the d2h
accounting of get / select, and the public surface of the four list classes of codecs.py.

Every expectation was read off the library before its entry points shared one host-call scaffold (csrc/host_call.h) and the file
passed against that library first (VIDC_LIBRARY).  The shapes are the smallest that reach every branch of the frame: six lists of
[0, 1, 513, 0, 64, 70] ids (513 crosses the 512-id chunk; leading and interior empty lists; a permutation of 0 .. ntotal - 1, ascending
per list, so the wavelet tree accepts it), graph objects of 5 rows x K = 8, compact rows at K = 8 and at K = 66 (the wide decoder).
The error cases go through the C-ABI with poisoned, guarded buffers (tests/contract_ref.py); nothing here tries to make a kernel fault.
"""
import inspect
import math
import threading

import numpy as np
import pytest

import contract_ref as cr

gpu = pytest.mark.gpu

VIDC_OK, VIDC_ERR_INVALID = 0, -1
SIZES = [0, 1, 513, 0, 64, 70]
NLIST = len(SIZES)
OFFSETS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
NTOTAL = int(OFFSETS[-1])
KINDS = ["packed", "ef", "wt", "roc"]
GETTERS = {"packed": "vidc_packed_get", "ef": "vidc_ef_get", "wt": "vidc_wt_select"}
GET_PREFIX = {"packed": "packed get", "ef": "ef get", "wt": "wt select"}
#: ctx.last_kernel_ms after decode_lists of lists that are all empty.  packed / wt return before any launch and store 0; Elias-Fano
#: and ROC both launch over the (empty) lists and report the time (read off the library before the shared scaffold).
EMPTY_LISTS_MS = {"packed": "zero", "wt": "zero", "ef": "positive", "roc": "positive"}


def _torch():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def ptr(x):
    return _L().ptr(x)


def last_error():
    return _L().lib().vidc_last_error().decode()


def make_ids():
    ids = np.random.default_rng(7).permutation(NTOTAL).astype(np.uint64)
    for l in range(NLIST):
        a, b = int(OFFSETS[l]), int(OFFSETS[l + 1])
        ids[a:b] = np.sort(ids[a:b])
    return ids


def build(kind, offsets, ids):
    c = _codecs()
    if kind == "packed":
        return c.PackedLists.encode(offsets, ids)
    if kind == "ef":
        return c.EfLists.encode(offsets, ids)
    if kind == "wt":
        return c.WaveletTreeLists.build(offsets, ids)
    return c.RocLists.encode(offsets, ids)


def make_rows(N, K, seed):
    """degrees 0, 1, K (or N when N < K) and values between; distinct ids below N inside a row"""
    rng = np.random.default_rng(seed)
    rows = np.full((N, K), -1, np.int32)
    top = min(N, K)
    deg = rng.integers(0, top + 1, N)
    deg[:3] = [0, 1, top]
    for i in range(N):
        rows[i, : deg[i]] = rng.choice(N, int(deg[i]), replace=False)
    return rows


class World:
    """the objects and references every test of this file shares (built once; nothing changes them)"""

    def __init__(self, oracle):
        torch = _torch()
        self.ctx = _L().default_context()
        self.ids = make_ids()
        self.d_ids = torch.from_numpy(self.ids.view(np.int64)).cuda()
        self.d_off = torch.from_numpy(OFFSETS.view(np.int64)).cuda()
        self.ref = {k: cr.ListRef(k, OFFSETS, self.ids, oracle) for k in KINDS}
        self.host = {k: build(k, OFFSETS, self.d_ids) for k in KINDS}
        self.dev = {k: build(k, self.d_off, self.d_ids) for k in KINDS}


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def ms_ok(ms):
    return math.isfinite(ms) and ms > 0


# ================================================================================================== ctx.last_kernel_ms
@gpu
@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_last_kernel_ms_lists(world, kind, src):
    ctx = world.ctx
    obj = build(kind, OFFSETS if src == "host" else world.d_off, world.d_ids)
    ms = ctx.last_kernel_ms()
    print(f"{kind}/{src}: encode {ms} ms")
    assert ms_ok(ms)
    out = obj.decode_all()
    ms = ctx.last_kernel_ms()
    print(f"{kind}/{src}: decode_all {ms} ms")
    assert ms_ok(ms)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), world.ref[kind].expected(None)[0])
    # only empty lists
    out, out_off = obj.decode_lists([0, 3, 0])
    ms = ctx.last_kernel_ms()
    print(f"{kind}/{src}: decode_lists(empty lists) {ms} ms")
    assert out.numel() == 0 and not out_off.any()
    if EMPTY_LISTS_MS[kind] == "zero":
        assert ms == 0.0
    else:
        assert ms_ok(ms)
    # non-empty lists (an empty one among them, one twice)
    req = [2, 0, 5, 2, 1]
    out, out_off = obj.decode_lists(req)
    ms = ctx.last_kernel_ms()
    print(f"{kind}/{src}: decode_lists {ms} ms")
    assert ms_ok(ms)
    exp, exp_off = world.ref[kind].expected(req)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), exp)
    np.testing.assert_array_equal(out_off, exp_off)


@gpu
@pytest.mark.parametrize("kind", ["ef", "roc"])
def test_last_kernel_ms_graph(world, oracle, kind):
    rows = make_rows(5, 8, 11)
    cls = _codecs().EfLists if kind == "ef" else _codecs().RocLists
    g = cls.encode_rows(rows)
    assert ms_ok(world.ctx.last_kernel_ms())
    ref = cr.RowRef(kind, rows, oracle)
    for nodes in (None, [4, 0, 2, 2]):
        out, counts = g.decode_rows(nodes)
        assert ms_ok(world.ctx.last_kernel_ms())
        exp, exp_cnt = ref.expected(nodes, 8)
        np.testing.assert_array_equal(out.cpu().numpy(), exp)
        np.testing.assert_array_equal(counts, exp_cnt)


# ====================================================================================================== compact rows
@gpu
@pytest.mark.parametrize("with_counts", [True, False])
@pytest.mark.parametrize("N,K", [(5, 8), (70, 66)])
def test_compact_decode_rows(world, N, K, with_counts):
    rows = make_rows(N, K, 100 + K)
    obj = _codecs().CompactRows.encode_rows(rows)
    assert ms_ok(world.ctx.last_kernel_ms())
    ref = cr.RowRef("compact", rows)
    for nodes in (None, [N - 1, 0, 2, 2, 1]):
        nd = None if nodes is None else np.asarray(nodes, np.uint64)
        m = N if nodes is None else nd.size
        whole, view = cr.guarded((m, K), np.int32, device="cuda")
        cwhole, cview = cr.guarded(m, np.uint32)
        st = _L().lib().vidc_compact_rows_decode(world.ctx.h, obj.h, m, ptr(nd), ptr(view), ptr(cview) if with_counts else None)
        assert st == VIDC_OK, last_error()
        assert ms_ok(world.ctx.last_kernel_ms())
        exp, exp_cnt = ref.expected(nodes, K)
        cr.assert_guards_intact(whole, view, "rows")
        cr.assert_view_equals(view, exp, "rows")
        if with_counts:
            cr.assert_guards_intact(cwhole, cview, "counts")
            cr.assert_view_equals(cview, exp_cnt, "counts")
        else:
            cr.assert_untouched(cwhole, cview, "counts")


# ========================================================================================== host mirror of the offsets
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_offsets_of_device_built_object(world, kind):
    obj = world.dev[kind]
    first = obj.offsets
    np.testing.assert_array_equal(first, OFFSETS)
    assert obj.offsets is first
    assert obj.ntotal == NTOTAL


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_offsets_first_read_from_two_threads(world, kind):
    obj = build(kind, world.d_off, world.d_ids)
    gate = threading.Barrier(2)
    got = [None, None]

    def read(i):
        gate.wait()
        got[i] = np.array(obj.offsets, copy=True)

    threads = [threading.Thread(target=read, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for g in got:
        np.testing.assert_array_equal(g, OFFSETS)
    np.testing.assert_array_equal(obj.offsets, OFFSETS)


# ================================================================================================== rejected requests
@gpu
@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_decode_lists_rejects_list_number_nlist(world, kind, src):
    obj = (world.host if src == "host" else world.dev)[kind]
    ln = np.array([2, NLIST, 1], np.uint64)
    whole, view = cr.guarded(NTOTAL, np.uint64, device="cuda")
    owhole, oview = cr.guarded(ln.size + 1, np.uint64)
    fn = getattr(_L().lib(), f"vidc_{kind}_decode_lists")
    st = fn(world.ctx.h, obj.h, ln.size, ptr(ln), ptr(view), ptr(oview))
    assert st == VIDC_ERR_INVALID
    assert last_error() == (f"list number {NLIST} out of range" if kind == "roc" else "list number out of range")
    cr.assert_untouched(whole, view, "d_out")
    cr.assert_guards_intact(owhole, oview, "out_offsets")  # (the prefix in front of the bad entry may have been written)


@gpu
@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("kind", list(GETTERS))
def test_get_rejects_and_m0(world, kind, src):
    obj = (world.host if src == "host" else world.dev)[kind]
    fn = getattr(_L().lib(), GETTERS[kind])
    before = world.ctx.d2h_bytes()
    for ln, of, bad in (([2, 4, 1], [0, 64, 0], (4, 64)),        # offset == the list's length
                        ([2, 0, 1], [5, 0, 0], (0, 0)),          # an empty list has no offset 0
                        ([2, NLIST, 1], [0, 0, 0], (NLIST, 0))):  # list number == nlist
        ln, of = np.array(ln, np.uint64), np.array(of, np.uint64)
        whole, view = cr.guarded(ln.size, np.int64)
        st = fn(world.ctx.h, obj.h, ln.size, ptr(ln), ptr(of), ptr(view))
        assert st == VIDC_ERR_INVALID
        assert last_error() == f"{GET_PREFIX[kind]}: (list {bad[0]}, offset {bad[1]}) out of range"
        cr.assert_untouched(whole, view, "ids_out")
    ln, of = np.array([2], np.uint64), np.array([0], np.uint64)
    whole, view = cr.guarded(1, np.int64)
    assert fn(world.ctx.h, obj.h, 0, ptr(ln), ptr(of), ptr(view)) == VIDC_OK
    assert fn(world.ctx.h, obj.h, 0, None, None, None) == VIDC_OK
    cr.assert_untouched(whole, view, "ids_out")
    assert world.ctx.d2h_bytes() == before


@gpu
@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("kind", list(GETTERS))
def test_get_every_item(world, kind, src):
    obj = (world.host if src == "host" else world.dev)[kind]
    ln = np.repeat(np.arange(NLIST, dtype=np.uint64), SIZES)
    of = np.concatenate([np.arange(n, dtype=np.uint64) for n in SIZES])
    m = ln.size
    assert m == NTOTAL
    whole, view = cr.guarded(m, np.int64)
    before = world.ctx.d2h_bytes()
    st = getattr(_L().lib(), GETTERS[kind])(world.ctx.h, obj.h, m, ptr(ln), ptr(of), ptr(view))
    assert st == VIDC_OK, last_error()
    assert world.ctx.d2h_bytes() - before == 8 * m
    cr.assert_guards_intact(whole, view, "ids_out")
    cr.assert_view_equals(view, world.ref[kind].flat.view(np.int64), "ids_out")  # (list-major request = the flat reference)
    # the wrapper of codecs.py gives the same
    got = obj.select(ln, of) if kind == "wt" else obj.get(ln, of)
    np.testing.assert_array_equal(got, world.ref[kind].flat.view(np.int64))


# ======================================================================================= public surface of codecs.py (no GPU)
#: public attribute -> "property" or str(inspect.signature(...)), generated from the classes before they shared a base class
SURFACE = {
    "EfLists": {
        "append": "(self, list_nos, ids, want_perm=False, labels=True, invalid=None)",
        "compressed_bytes": "property",
        "decode_all": "(self, out=None)",
        "decode_gather": "(self, list_nos, item_slot, item_off)",
        "decode_lists": "(self, list_nos)",
        "decode_rows": "(self, nodes, K=None, want_counts=True)",
        "encode": "(offsets, ids, want_perm=False, ctx=None)",
        "encode_rows": "(rows, ctx=None)",
        "export": "(self, list_no)",
        "get": "(self, list_nos, offs)",
        "info": "(self)",
        "load": "(path, ctx=None)",
        "ntotal": "property",
        "offsets": "property",
        "perm": "(self)",
        "save": "(self, path)",
        "translate_labels": "(self, labels, out=None, invalid=None)",
    },
    "PackedLists": {
        "append": "(self, list_nos, ids, bits=None, labels=True, invalid=None)",
        "bits": "property",
        "bits_for": "(ntotal)",
        "compressed_bytes": "property",
        "decode_all": "(self, out=None)",
        "decode_gather": "(self, list_nos, item_slot, item_off)",
        "decode_lists": "(self, list_nos)",
        "encode": "(offsets, ids, bits=None, ctx=None)",
        "export_bytes": "(self, list_no)",
        "get": "(self, list_nos, offs)",
        "load": "(path, ctx=None)",
        "ntotal": "property",
        "offsets": "property",
        "save": "(self, path)",
        "translate_labels": "(self, labels, out=None, invalid=None)",
    },
    "RocLists": {
        "all_words": "(self)",
        "append": "(self, list_nos, ids, precision_mode=-1, want_perm=False, labels=True, invalid=None)",
        "compressed_bytes": "property",
        "decode_all": "(self, out=None)",
        "decode_gather": "(self, list_nos, item_slot, item_off)",
        "decode_lists": "(self, list_nos)",
        "decode_rows": "(self, nodes, K=None, want_counts=True)",
        "encode": "(offsets, ids, precision_mode=-1, want_perm=False, ctx=None)",
        "encode_rows": "(rows, precision_mode=-1, ctx=None)",
        "from_streams": "(offsets, precisions, heads, nwords, words_concat, mt_draws=None, ctx=None)",
        "info": "(self)",
        "last_decode_handed_back": "property",
        "last_decode_nonclean": "property",
        "load": "(path, ctx=None)",
        "nlist": "property",
        "ntotal": "property",
        "offsets": "property",
        "perm": "(self)",
        "save": "(self, path)",
        "total_words": "property",
        "translate_labels": "(self, labels, out=None, invalid=None)",
        "words": "(self, list_no, nwords=None)",
    },
    "WaveletTreeLists": {
        "append": "(self, list_nos, ids, labels=True, invalid=None)",
        "build": "(offsets, ids, wt_type=0, ctx=None)",
        "decode_all": "(self, out=None)",
        "decode_gather": "(self, list_nos, item_slot, item_off)",
        "decode_lists": "(self, list_nos)",
        "levels": "property",
        "ntotal": "property",
        "offsets": "property",
        "select": "(self, list_nos, offs)",
        "size_in_bytes": "property",
        "translate_labels": "(self, labels, out=None, invalid=None)",
    },
}


def test_public_surface_of_the_list_classes():
    codecs = _codecs()
    for cname, want in SURFACE.items():
        cls = getattr(codecs, cname)
        got = {}
        for name in dir(cls):
            if name.startswith("_"):
                continue
            got[name] = "property" if isinstance(inspect.getattr_static(cls, name), property) else str(inspect.signature(getattr(cls, name)))
        assert got == want, cname
    off = np.array([0, 2], np.uint64)
    r = codecs.RocLists(None, None, off)  # (three positional arguments; a None handle is never released)
    assert r.offsets is off
    for cname in ("PackedLists", "EfLists", "WaveletTreeLists"):
        o = getattr(codecs, cname)(None, None, off)
        assert o.offsets is off and o.ntotal == 2
        o = getattr(codecs, cname)(None, None, None, 1, 2)
        assert o.ntotal == 2
