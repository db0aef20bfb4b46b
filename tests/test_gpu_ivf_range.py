"""The IVF range search on the device (vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev, ivf_range.range_scan_device /
range_search_device) against the numpy model (tests/ivf_range_ref.py).  Data are integer grids, so slot limits, D and labels are
compared element for element.  Calls go through the C-ABI into guarded, poisoned buffers; the d2h counter moves by 8 for a count
that returns its total and not at all otherwise; the inputs are the same before and after.  Radii, designed objects and the one-CU
batches are the ones the CPU tests hold to their purpose."""
import ctypes

import numpy as np
import pytest

import contract_ref as cr
import ivf_range_ref as rr
import ivf_scan_ref as ir
from test_ivf_range_ref_cpu import FORMS, NPROBES

pytestmark = pytest.mark.gpu

INVALID = -1


def _t():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


class Dev:
    """the inputs of a call on the device, the codes between guard bands of their own.  misalign: bytes the code array is shifted
    by; offsets: damaged offsets in the place of the object's; over: arguments replaced in the calls."""

    def __init__(self, o, ctx, xq, probes, misalign=0, offsets=None, over=None):
        torch, lib = _t(), _L()
        self.o, self.ctx, self.xq, self.probes = o, ctx, np.asarray(xq, np.float32), np.asarray(probes, np.int64)
        self.nq, self.nprobe = self.probes.shape
        self.nslots = self.nq * self.nprobe
        self.code_bytes = o["codes"].size
        self.pad = 4096 + misalign
        self.band = torch.full((self.pad + self.code_bytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
        codes = self.band[self.pad: self.pad + self.code_bytes]
        codes.copy_(torch.from_numpy(o["codes"].reshape(-1).copy()))
        assert codes.data_ptr() % 16 == misalign % 16
        self.off_np = np.asarray(o["offsets"] if offsets is None else offsets, dtype=np.uint64)
        self.off = torch.from_numpy(self.off_np.view(np.int64).copy()).cuda()
        self.cb = torch.from_numpy(o["codebooks"].copy()).cuda() if o["M"] else None
        self.qt = torch.from_numpy(np.ascontiguousarray(self.xq).copy()).cuda()
        self.pt = torch.from_numpy(np.ascontiguousarray(self.probes).copy()).cuda()
        self.a = dict(ctx=ctx.h, nlist=o["nlist"], off=lib.ptr(self.off), ntotal=o["ntotal"],
                      codes=lib.ptr(codes) if self.code_bytes else lib.ptr(self.band), kind=o["kind"], d=o["d"], M=o["M"], cb=lib.ptr(self.cb),
                      nq=self.nq, xq=lib.ptr(self.qt), nprobe=self.nprobe, probes=lib.ptr(self.pt))
        self.a.update(over or {})
        self.what = f"kind={o['kind']} d={o['d']} M={o['M']} nq={self.nq} nprobe={self.nprobe} misalign={misalign} {over}"

    def _head(self, radius):
        a = self.a
        return (a["ctx"], a["nlist"], a["off"], a["ntotal"], a["codes"], a["kind"], a["d"], a["M"], a["cb"], a["nq"], a["xq"], a["nprobe"],
                a["probes"], float(radius))

    def _call(self, fn, args, moved, status):
        torch, lib = _t(), _L()
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d2h = self.ctx.d2h_bytes()
        torch.cuda.synchronize()
        st = fn(*args)
        torch.cuda.synchronize()
        assert st == status, (self.what, st, lib.lib().vidc_last_error())
        assert self.ctx.d2h_bytes() - d2h == moved, f"{self.what}: the d2h counter moved by {self.ctx.d2h_bytes() - d2h}, not {moved}"
        if status:
            assert b"range" in lib.lib().vidc_last_error(), lib.lib().vidc_last_error()
        band = self.band.cpu().numpy()
        assert (band[:self.pad] == 0x5A).all() and (band[self.pad + self.code_bytes:] == 0x5A).all(), f"{self.what}: the bands around the codes changed"
        assert np.array_equal(band[self.pad: self.pad + self.code_bytes], self.o["codes"].reshape(-1)), f"{self.what}: the codes changed"
        assert np.array_equal(self.off.cpu().numpy().view(np.uint64), self.off_np) and np.array_equal(self.pt.cpu().numpy(), self.probes)
        assert np.array_equal(self.qt.cpu().numpy(), self.xq), f"{self.what}: the queries changed"

    def count(self, radius, want_total=True, status=0):
        """-> (slot_lims uint64 [nq * nprobe + 1], total or None); on a refusal nothing is written.  A total that is returned moves
        the d2h counter by 8, except at nq == 0, where nothing is read back"""
        lib = _L()
        w, v = cr.guarded((self.nslots + 1,), np.int64, device="cuda")
        total = ctypes.c_uint64(0xDEAD)
        self._call(lib.lib().vidc_ivf_range_count_dev, (*self._head(radius), self.a.get("lims", lib.ptr(v)), ctypes.byref(total) if want_total else None),
                   8 if want_total and not status and self.nq else 0, status)
        if status:
            cr.assert_untouched(w, v, self.what)
            assert total.value == 0xDEAD
            return None
        cr.assert_guards_intact(w, v, f"{self.what}: slot_lims")
        lims = v.cpu().numpy().view(np.uint64).copy()
        if want_total:
            assert total.value == int(lims[-1]), f"{self.what}: total {total.value}, slot_lims ends at {int(lims[-1])}"
        return lims, (int(total.value) if want_total else None)

    def fill(self, radius, lims, capacity, status=0, over=None):
        """-> (D float32 [capacity], labels int64 [capacity]): what the call left in poisoned arrays"""
        torch, lib = _t(), _L()
        lt = torch.from_numpy(np.asarray(lims, np.uint64).view(np.int64).copy()).cuda()
        wD, vD = cr.guarded((max(capacity, 1),), np.int32, device="cuda")
        wL, vL = cr.guarded((max(capacity, 1),), np.int64, device="cuda")
        a = dict(lims=lib.ptr(lt), capacity=capacity, D=lib.ptr(vD), labels=lib.ptr(vL))
        a.update(over or {})
        self._call(lib.lib().vidc_ivf_range_fill_dev, (*self._head(radius), a["lims"], a["capacity"], a["D"], a["labels"]), 0, status)
        assert np.array_equal(lt.cpu().numpy().view(np.uint64), np.asarray(lims, np.uint64)), f"{self.what}: the slot limits changed"
        if status or capacity == 0:
            cr.assert_untouched(wD, vD, self.what)
            cr.assert_untouched(wL, vL, self.what)
            return np.zeros(0, np.float32), np.zeros(0, np.int64)
        cr.assert_guards_intact(wD, vD, f"{self.what}: D")
        cr.assert_guards_intact(wL, vL, f"{self.what}: labels")
        return vD.view(torch.float32).cpu().numpy().copy(), vL.cpu().numpy().copy()


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("slot_lims", "D", "labels")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, not {w.shape}"
        bad = np.flatnonzero(g.view(np.uint64 if g.itemsize == 8 else np.uint32) != w.view(np.uint64 if w.itemsize == 8 else np.uint32))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.size} elements)"


def check(dev, radius, want=None, want_total=True):
    """count, fill at the exact capacity -> the model, element for element"""
    o = dev.o
    want = rr.model(o["offsets"], o["vecs"], dev.xq, dev.probes, radius) if want is None else want
    lims, total = dev.count(radius, want_total=want_total)
    D, L = dev.fill(radius, lims, int(lims[-1]))
    assert_equal((lims, D, L), want, f"{dev.what} radius={radius}")


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


@pytest.mark.parametrize("d,M", FORMS)
def test_designed_objects_through_the_abi(ctx, d, M):
    """list sizes around the trip, invalid and repeated probes, an empty slot between two full ones: every d of FLAT, every (M, dsub)
    of PQ8, every radius of the list"""
    dev = Dev(ir.obj(d, M), ctx, ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS)
    for radius in rr.radii(d, M):
        check(dev, radius)
    check(dev, rr.equal_radius(d, M), want_total=False)  # no total: nothing comes back to the host


@pytest.mark.parametrize("M", (0, 4))
def test_every_nprobe(ctx, M):
    o = ir.obj(4, M)
    for nprobe in NPROBES:
        dev = Dev(o, ctx, ir.queries(4, 3), ir.probe_rows(3, nprobe))
        for radius in (rr.equal_radius(4, M) + 0.5, float("inf")):
            check(dev, radius)


def tiled(want, idx, nprobe):
    """the model's answer for the queries idx of a batch whose distinct queries gave `want`"""
    lims, D, L = want
    lims = lims.astype(np.int64)
    counts = np.diff(lims).reshape(-1, nprobe)[idx].reshape(-1)
    seg = [(int(lims[q * nprobe]), int(lims[(q + 1) * nprobe])) for q in range(lims.size // nprobe)]
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), np.concatenate([D[seg[q][0]:seg[q][1]] for q in idx]),
            np.concatenate([L[seg[q][0]:seg[q][1]] for q in idx]))


def test_alignment_and_batches_on_both_sides_of_the_cut(ctx):
    """a FLAT code array 4 bytes off (the scalar-load path) and PQ codes 4, 1 and 8 bytes off (narrower code loads); nq = 1, 2, 3 with
    16 probes, so that the row is cut, and a batch above the resident wavefronts: one piece per query, several items per wavefront"""
    for d in (4, 20, 128):
        dev = Dev(ir.obj(d), ctx, ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, misalign=4)
        for radius in (rr.equal_radius(d), float("inf")):
            check(dev, radius)
    for mis in (4, 1, 8):
        dev = Dev(ir.obj(128, 16), ctx, ir.queries(128, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, misalign=mis)
        for radius in (rr.equal_radius(128, 16), float("inf")):
            check(dev, radius)
    num_cu = ctx.num_cu()
    for d, M in ((4, 0), (128, 16)):
        o = ir.obj(d, M)
        resident = ir.plan_resident(num_cu, rr.plan_lds(o["kind"], 16, d, M))
        big = resident + 5
        rows, xq = ir.probe_rows(3, 16), ir.queries(d, 3)
        radius = rr.equal_radius(d, M) + 0.5
        want = rr.model(o["offsets"], o["vecs"], xq, rows, radius)
        for nq in (1, 2, 3):
            assert ir.plan_pieces(nq, 16, resident) > 1
            check(Dev(o, ctx, xq[:nq], rows[:nq]), radius, want=tiled(want, np.arange(nq), 16))
        assert ir.plan_pieces(big, 16, resident) == 1
        idx = np.arange(big) % 3
        check(Dev(o, ctx, xq[idx], rows[idx]), radius, want=tiled(want, idx, 16))


@pytest.fixture(scope="module")
def small():
    """a context created under VIDC_NUM_CU=1, pool poison on, running on torch's stream (the idiom of tests/test_gpu_ivf_scan.py)"""
    lib, torch = _L(), _t()
    torch.cuda.set_device(0)
    mp = pytest.MonkeyPatch()
    mp.setenv("VIDC_NUM_CU", "1")
    c = lib.Context(0)
    mp.undo()
    assert c.num_cu() == 1
    c.set_pool_poison(True)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    torch.cuda.synchronize()
    c.close()


@pytest.mark.parametrize("kind", sorted(rr.ONE_CU))
def test_one_cu_context_wavefronts_go_round(small, kind):
    """every wavefront takes several items; the hit counts come from scratch that was handed out full of 0xFF, so a slot whose
    count nobody wrote would show in the slot limits"""
    b = rr.ONE_CU[kind]
    o = ir.obj(b["d"], b["M"])
    rows, xq = ir.probe_rows(8, b["nprobe"]), ir.queries(b["d"], 8)
    for radius in (rr.equal_radius(b["d"], b["M"]) + 0.5, float("inf")):
        want = rr.model(o["offsets"], o["vecs"], xq, rows, radius)
        for nq in (b["nq_cut"], b["nq_whole"], b["nq_cut"]):  # (the second cut call gets the first one's block back from the cache)
            idx = (np.arange(nq) * 3) % 8
            check(Dev(o, small, xq[idx], rows[idx]), radius, want=tiled(want, idx, b["nprobe"]))


@pytest.mark.parametrize("d,M", ((4, 0), (128, 16)))
def test_the_write_bound(ctx, d, M):
    o, xq, rows = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS
    dev = Dev(o, ctx, xq, rows)
    args = (o["offsets"], o["vecs"], xq, rows)
    eq = rr.equal_radius(d, M)
    lims, D, L = rr.model(*args, eq + 0.5)
    total = int(lims[-1])
    # a capacity below the total: the prefix is exact, nothing lies behind it (the arrays end there, between guards)
    widths = np.diff(lims.astype(np.int64))
    s = int(np.flatnonzero(widths > 2)[-1])
    middle = int(lims[s]) + int(widths[s]) // 2
    assert 0 < int(lims[s]) < middle < int(lims[s + 1]) <= total
    for cap in (total - 1, middle, 1, 0):
        gD, gL = dev.fill(eq + 0.5, lims, cap)
        assert rr.same_bits(gD, D[:cap]) and rr.same_bits(gL, L[:cap]), f"capacity {cap}"
    # a capacity above the total: the tail stays poison
    gD, gL = dev.fill(eq + 0.5, lims, total + 7)
    assert rr.same_bits(gD[:total], D) and rr.same_bits(gL[:total], L)
    assert rr.same_bits(gD[total:], np.full(7, rr.POISON_D, np.float32)) and (gL[total:] == rr.POISON_L).all()
    # slot limits counted at a smaller radius: every slot holds its first hits; at a larger radius: the tail of a slot is poison
    small_lims = rr.model(*args, eq - 0.5)[0]
    big_lims = rr.model(*args, np.inf)[0]
    assert 0 < int(small_lims[-1]) < total < int(big_lims[-1])
    for other in (small_lims, big_lims):
        for cap in (int(other[-1]), int(other[-1]) // 2):
            want = rr.fill_model(*args, eq + 0.5, other, cap)
            got = dev.fill(eq + 0.5, other, cap)
            assert rr.same_bits(got[0], want[0]) and rr.same_bits(got[1], want[1]), f"slot limits of another radius, capacity {cap}"
    wD = rr.fill_model(*args, eq + 0.5, big_lims, int(big_lims[-1]))[0]
    assert (wD.view(np.uint32) == 0xA5A5A5A5).sum() == int(big_lims[-1]) - total  # (the untouched tails exist)
    # slot limits that are no prefix sum at all: decreasing, huge, all zero -- nothing is written, the guards hold
    for junk in (lims[::-1].copy(), lims + np.uint64(2 ** 63), np.zeros_like(lims)):
        want = rr.fill_model(*args, eq + 0.5, junk, total)
        got = dev.fill(eq + 0.5, junk, total)
        assert rr.same_bits(got[0], want[0]) and rr.same_bits(got[1], want[1])
    # all ones: a place wraps round 2^64 and lands inside [0, capacity), for several slots at once -- what is written there is not
    # stated, only that the guards hold (checked by fill)
    dev.fill(eq + 0.5, np.full_like(lims, np.uint64(2 ** 64 - 1)), total)
    check(dev, eq + 0.5)


def test_damaged_offsets(ctx):
    """offsets that decrease, or that exceed ntotal: both calls return VIDC_OK, nothing outside the codes is read or written that the
    guard bands could show, and the context still works"""
    for d, M in ((4, 0), (128, 16)):
        o = ir.obj(d, M)
        off = np.asarray(o["offsets"]).copy()
        xq = ir.queries(d, len(ir.EDGE_ROWS))
        for bad in (off[::-1].copy(), off + np.uint64(o["ntotal"]), np.where(np.arange(off.size) % 2, np.uint64(2 ** 63), off),
                    np.full_like(off, np.uint64(2 ** 64 - 1))):
            dev = Dev(o, ctx, xq, ir.EDGE_ROWS, offsets=bad)
            lims, total = dev.count(np.inf)
            assert total <= ir.EDGE_ROWS.size * o["ntotal"] and (np.diff(lims.astype(np.int64)) >= 0).all()
            dev.fill(np.inf, lims, total)
            dev.fill(np.inf, lims, total // 2)
        check(Dev(o, ctx, xq, ir.EDGE_ROWS), np.inf)


def test_cross_check_with_the_scan(ctx):
    """radius = +inf on queries with at most 256 candidates: sorted by (distance, label), the range result is vidc_ivf_scan_dev's at
    k = 256 -- the same distances bit for bit, the same labels"""
    from test_gpu_ivf_scan import call_abi

    for d, M in ((4, 0), (20, 0), (128, 16), (4, 4)):
        o = ir.obj(d, M)
        keep = [q for q, r in enumerate(ir.EDGE_ROWS) if sum(ir.EDGE_SIZES[l] for l in ir.valid_lists(r, o["nlist"])) <= 256]
        assert len(keep) >= 8
        rows, xq = ir.EDGE_ROWS[keep], ir.queries(d, len(ir.EDGE_ROWS))[keep]
        sD, sL, _ = call_abi(o, ctx, xq, rows, 256)
        dev = Dev(o, ctx, xq, rows)
        lims, total = dev.count(np.inf)
        D, L = dev.fill(np.inf, lims, total)
        nprobe = rows.shape[1]
        for q in range(len(keep)):
            a, b = int(lims[q * nprobe]), int(lims[(q + 1) * nprobe])
            order = np.lexsort((L[a:b], D[a:b]))
            n = b - a
            assert n == int((sL[q] >= 0).sum()), (d, M, q)
            assert rr.same_bits(D[a:b][order], sD[q, :n]) and np.array_equal(L[a:b][order], sL[q, :n]), (d, M, q)


def test_refusals_and_empty_calls_on_a_live_context(ctx):
    o, xq, rows = ir.obj(128, 16), ir.queries(128, 5), ir.probe_rows(5, 3)
    lims = rr.model(o["offsets"], o["vecs"], xq, rows, np.inf)[0]
    for kw in (dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049),
               dict(ntotal=2 ** 32), dict(nlist=2 ** 31), dict(kind=2), dict(M=0), dict(M=65), dict(M=3), dict(cb=None), dict(nq=2 ** 32 - 1),
               dict(lims=None)):
        dev = Dev(o, ctx, xq, rows, over=kw)
        dev.count(1.0, status=INVALID)
        dev.fill(np.inf, lims, int(lims[-1]), status=INVALID, over=dict(lims=None) if "lims" in kw else None)
    dev = Dev(o, ctx, xq, rows)
    dev.fill(np.inf, lims, int(lims[-1]), status=INVALID, over=dict(D=None))
    dev.fill(np.inf, lims, int(lims[-1]), status=INVALID, over=dict(labels=None))
    dev.fill(np.inf, lims, 0, over=dict(D=None, labels=None))  # capacity == 0: VIDC_OK, nothing written
    # nq == 0: the count writes slot_lims[0] = 0 and the total, the fill launches nothing
    empty = Dev(o, ctx, xq[:0], rows[:0])
    l0, total = empty.count(np.inf)
    assert l0.tolist() == [0] and total == 0
    empty.fill(np.inf, l0, 4)
    assert np.array_equal(empty.fill(np.inf, l0, 4)[1], np.full(4, rr.POISON_L))
    check(dev, np.inf)
    none = ir.obj(4, 0, sizes=(0, 0, 0))  # no codes at all: every slot is empty
    dn = Dev(none, ctx, ir.queries(4, 3), ir.probe_rows(3, 3, nlist=3))
    ln, tn = dn.count(np.inf)
    assert tn == 0 and not ln.any()
    dn.fill(np.inf, ln, 0)


# ------------------------------------------------------------------------------------------------ the Python layer
CONTAINERS = ("array", "packed", "roc", "ef", "wt", "rocseg")


@pytest.mark.parametrize("pq", (False, True), ids=("flat", "pq"))
@pytest.mark.parametrize("container", CONTAINERS)
def test_range_search_device(container, pq):
    """lims equals the model's; per query the multiset of (D, id) equals a numpy brute force over the stored vectors and their ids;
    the labels translate back to those ids"""
    from test_gpu_ivf_scan import make_index
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd import ivf_range
    from vector_db_id_compression_amd.invlists import to_csr

    torch = _t()
    s = ir.shape("distinct")
    idx = make_index("distinct", pq, "array" if container == "rocseg" else container)
    if container == "rocseg":
        idx.replace_invlists(ci.CompressedIDInvertedListsROCSegmented(idx.invlists))
    xq, n = s["xq"][:24], 1500
    # the stored vectors by id (the raw ones, or what their PQ codes decode to) and the list of every id, from the container's ids
    stored = idx._decode_codes(idx._encode_dev(torch.from_numpy(s["x"][:n].copy()).cuda())).cpu().numpy() if pq else s["x"][:n]
    off, codes = idx._device_lists()
    il = idx.invlists
    ids_all = il.get_ids_all().cpu().numpy().view(np.int64) if hasattr(il, "get_ids_all") else to_csr(il)[1].view(np.int64)
    assert np.array_equal(np.sort(ids_all), np.arange(n))
    assign = np.empty(n, np.int64)
    assign[ids_all] = np.searchsorted(np.asarray(off, np.int64), np.arange(n), side="right") - 1
    probes = torch.cdist(torch.from_numpy(xq.copy()).cuda(), idx.centroids).topk(idx.nprobe, largest=False).indices.cpu().numpy()
    radius = float(np.median(ir.l2(stored[np.isin(assign, probes[0])], xq[0]))) + 0.5
    want_lims = rr.model(off, idx._decode_codes(codes).cpu().numpy(), xq, probes, radius)[0]
    lims, D, I = ivf_range.range_search_device(idx, xq, radius)
    assert lims.is_cuda and D.is_cuda and I.is_cuda and (lims.dtype, D.dtype, I.dtype) == (torch.int64, torch.float32, torch.int64)
    lims, D, I = lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()
    assert np.array_equal(lims, want_lims[::idx.nprobe].astype(np.int64)) and lims[-1] == D.size == I.size and D.size > len(xq)
    for q in range(len(xq)):
        ids = np.flatnonzero(np.isin(assign, probes[q]))
        dist = ir.l2(stored[ids], xq[q])
        hit = dist < np.float32(radius)
        want = sorted(zip(dist[hit].tolist(), ids[hit].tolist()))
        got = sorted(zip(D[lims[q]:lims[q + 1]].tolist(), I[lims[q]:lims[q + 1]].tolist()))
        assert got == want, f"{container} pq={pq} query {q}: {len(got)} results, {len(want)} expected"
    # the labels of range_scan_device, given the same probes, translate to the same ids
    l2_, D2, labels = ivf_range.range_scan_device(idx, torch.from_numpy(xq.copy()).cuda(), radius, probes=torch.from_numpy(probes).cuda())
    assert np.array_equal(l2_.cpu().numpy(), lims) and np.array_equal(D2.cpu().numpy(), D)
    if hasattr(il, "translate_labels"):
        back = il.translate_labels(labels).cpu().numpy()
    else:
        lab = labels.cpu().numpy()
        back = to_csr(il)[1].view(np.int64)[np.asarray(off, np.int64)[lab >> 32] + (lab & 0xFFFFFFFF)]
    assert np.array_equal(back, I)
    # radii without results
    for r in (0.0, float("nan")):
        l0, D0, I0 = ivf_range.range_search_device(idx, xq, r)
        assert not l0.cpu().numpy().any() and l0.numel() == len(xq) + 1 and D0.numel() == 0 and I0.numel() == 0
