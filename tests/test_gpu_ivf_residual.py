"""Residual PQ in the IVF scan and range search on the device (vidc_ivf_scan_residual_dev, vidc_ivf_range_count_residual_dev /
vidc_ivf_range_fill_residual_dev, IVFIndex(..., by_residual=True)) against the numpy model (tests/ivf_residual_ref.py) and against the
per-query torch scan (IVFIndex._scan).  Data are integer grids with d * (3R)^2 < 2^24, so D, labels, stats and slot limits are compared
element for element, ties included; one test runs float data against a written-out error bound.  Calls through the C-ABI write into
guarded, poisoned buffers; the d2h counter moves only by the 8 bytes of a count that returns its total; the inputs are held."""
import ctypes

import numpy as np
import pytest

import contract_ref as cr
import ivf_range_ref as rr
import ivf_residual_ref as rs
import ivf_scan_ref as ir

pytestmark = pytest.mark.gpu


def _t():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


class Dev:
    """the inputs of a call on the device, the codes between guard bands of their own.  misalign: bytes the code array is shifted
    by; offsets: damaged offsets in the place of the object's."""

    def __init__(self, o, ctx, xq, probes, misalign=0, offsets=None):
        torch, lib = _t(), _L()
        self.o, self.ctx, self.xq, self.probes = o, ctx, np.ascontiguousarray(xq, np.float32), np.ascontiguousarray(probes, np.int64)
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
        self.cb = torch.from_numpy(o["codebooks"].copy()).cuda()
        self.cent = torch.from_numpy(o["centroids"].copy()).cuda()
        self.qt = torch.from_numpy(self.xq.copy()).cuda()
        self.pt = torch.from_numpy(self.probes.copy()).cuda()
        self.head = (ctx.h, o["nlist"], lib.ptr(self.off), o["ntotal"], lib.ptr(codes), o["d"], o["M"], lib.ptr(self.cb), lib.ptr(self.cent),
                     self.nq, lib.ptr(self.qt), self.nprobe, lib.ptr(self.pt))
        self.what = f"d={o['d']} M={o['M']} nq={self.nq} nprobe={self.nprobe} misalign={misalign}"

    def _call(self, fn, args, moved):
        torch, lib = _t(), _L()
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        d2h = self.ctx.d2h_bytes()
        torch.cuda.synchronize()
        st = fn(*args)
        torch.cuda.synchronize()
        assert st == 0, (self.what, st, lib.lib().vidc_last_error())
        assert self.ctx.d2h_bytes() - d2h == moved, f"{self.what}: the d2h counter moved by {self.ctx.d2h_bytes() - d2h}, not {moved}"
        band = self.band.cpu().numpy()
        assert (band[:self.pad] == 0x5A).all() and (band[self.pad + self.code_bytes:] == 0x5A).all(), f"{self.what}: the bands around the codes changed"
        assert np.array_equal(band[self.pad: self.pad + self.code_bytes], self.o["codes"].reshape(-1)), f"{self.what}: the codes changed"
        assert np.array_equal(self.off.cpu().numpy().view(np.uint64), self.off_np) and np.array_equal(self.pt.cpu().numpy(), self.probes)
        assert np.array_equal(self.qt.cpu().numpy(), self.xq) and np.array_equal(self.cent.cpu().numpy(), self.o["centroids"])
        assert np.array_equal(self.cb.cpu().numpy(), self.o["codebooks"]), f"{self.what}: the codebooks changed"

    def scan(self, k, want_stats=True):
        """-> (D, labels, stats) numpy"""
        torch, lib = _t(), _L()
        wD, vD = cr.guarded((self.nq, k), np.int32, device="cuda")
        wL, vL = cr.guarded((self.nq, k), np.int64, device="cuda")
        wS, vS = cr.guarded((self.nq, 2), np.int32, device="cuda")
        self._call(lib.lib().vidc_ivf_scan_residual_dev, (*self.head, k, lib.ptr(vD), lib.ptr(vL), lib.ptr(vS) if want_stats else None), 0)
        for w, v, name in ((wD, vD, "D"), (wL, vL, "labels"), (wS, vS, "stats")):
            cr.assert_guards_intact(w, v, f"{self.what} k={k}: {name}")
        if not want_stats:
            cr.assert_untouched(wS, vS, self.what)
        return vD.view(torch.float32).cpu().numpy().copy(), vL.cpu().numpy().copy(), vS.cpu().numpy().view(np.uint32).copy()

    def count(self, radius, want_total=True):
        """-> slot_lims uint64 [nq * nprobe + 1]; a total that is returned moves the d2h counter by 8"""
        lib = _L()
        w, v = cr.guarded((self.nslots + 1,), np.int64, device="cuda")
        total = ctypes.c_uint64(0xDEAD)
        self._call(lib.lib().vidc_ivf_range_count_residual_dev, (*self.head, float(radius), lib.ptr(v), ctypes.byref(total) if want_total else None),
                   8 if want_total else 0)
        cr.assert_guards_intact(w, v, f"{self.what}: slot_lims")
        lims = v.cpu().numpy().view(np.uint64).copy()
        assert total.value == (int(lims[-1]) if want_total else 0xDEAD), f"{self.what}: total {total.value}, slot_lims ends at {int(lims[-1])}"
        return lims

    def fill(self, radius, lims, capacity):
        """-> (D float32 [capacity], labels int64 [capacity]): what the call left in poisoned arrays"""
        torch, lib = _t(), _L()
        lt = torch.from_numpy(np.asarray(lims, np.uint64).view(np.int64).copy()).cuda()
        wD, vD = cr.guarded((max(capacity, 1),), np.int32, device="cuda")
        wL, vL = cr.guarded((max(capacity, 1),), np.int64, device="cuda")
        self._call(lib.lib().vidc_ivf_range_fill_residual_dev, (*self.head, float(radius), lib.ptr(lt), capacity, lib.ptr(vD), lib.ptr(vL)), 0)
        assert np.array_equal(lt.cpu().numpy().view(np.uint64), np.asarray(lims, np.uint64)), f"{self.what}: the slot limits changed"
        if capacity == 0:
            cr.assert_untouched(wD, vD, self.what)
            cr.assert_untouched(wL, vL, self.what)
            return np.zeros(0, np.float32), np.zeros(0, np.int64)
        cr.assert_guards_intact(wD, vD, f"{self.what}: D")
        cr.assert_guards_intact(wL, vL, f"{self.what}: labels")
        return vD.view(torch.float32).cpu().numpy().copy(), vL.cpu().numpy().copy()

    def range(self, radius, want_total=True):
        """count, then fill at the exact capacity -> (slot_lims, D, labels)"""
        lims = self.count(radius, want_total)
        return (lims, *self.fill(radius, lims, int(lims[-1])))


def assert_equal(got, want, what, names=("D", "labels", "stats")):
    for g, w, name in zip(got, want, names):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, not {w.shape}"
        bad = np.argwhere(g.view(np.uint64 if g.itemsize == 8 else np.uint32) != w.view(np.uint64 if w.itemsize == 8 else np.uint32))
        assert bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} elements)"


RANGE = ("slot_lims", "D", "labels")


def scan_model(o, xq, probes, k):
    return ir.model(o["offsets"], o["vecs"], xq, probes, k)


def range_model(o, xq, probes, radius):
    return rr.model(o["offsets"], o["vecs"], xq, probes, radius)


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


@pytest.mark.parametrize("d,M", rs.FORMS)
def test_designed_objects_through_the_abi(ctx, d, M):
    """list sizes around the trip, an empty list, short lists against k, invalid (-1, nlist, 2^40) and repeated probes"""
    o, xq = rs.obj(d, M), rs.queries(d, len(rs.EDGE_ROWS))
    dev = Dev(o, ctx, xq, rs.EDGE_ROWS)
    assert_equal(dev.scan(64), scan_model(o, xq, rs.EDGE_ROWS, 64), f"d={d} M={M} k=64")
    assert_equal(dev.scan(10, want_stats=False)[:2], scan_model(o, xq, rs.EDGE_ROWS, 10)[:2], f"d={d} M={M} k=10, no stats")
    for i, radius in enumerate(rs.radii(d, M)):
        assert_equal(dev.range(radius, want_total=i != 1), range_model(o, xq, rs.EDGE_ROWS, radius), f"d={d} M={M} radius={radius}", RANGE)


def test_misaligned_codes_small_batches_and_wide_calls(ctx):
    """codes 1, 4 and 8 bytes off (narrower code loads); nq = 1, 2, 3 with 16 probes, so that the row is cut, and the same rows in a
    batch above the resident slots (one piece per query); nprobe = 1024 with k = 256 once"""
    o, xq = rs.obj(128, 16), rs.queries(128, len(rs.EDGE_ROWS))
    for mis in (1, 4, 8):
        dev = Dev(o, ctx, xq, rs.EDGE_ROWS, misalign=mis)
        assert_equal(dev.scan(64), scan_model(o, xq, rs.EDGE_ROWS, 64), f"misaligned by {mis}")
        assert_equal(dev.range(rs.radii(128, 16)[1]), range_model(o, xq, rs.EDGE_ROWS, rs.radii(128, 16)[1]), f"misaligned by {mis}", RANGE)
    num_cu = ctx.num_cu()
    rows, xq = ir.probe_rows(3, 16), rs.queries(128, 3)
    want, rwant = scan_model(o, xq, rows, 20), [range_model(o, xq[:nq], rows[:nq], rs.radii(128, 16)[1]) for nq in (1, 2, 3)]
    for resident, kk in ((rs.plan_resident(num_cu, rs.plan_lds(20, 16, 128, 16)), 20), (rs.plan_resident(num_cu, rs.plan_lds(0, 16, 128, 16)), 0)):
        for nq in (1, 2, 3):
            assert rs.plan_pieces(nq, 16, resident) > 1
            dev = Dev(o, ctx, xq[:nq], rows[:nq])
            if kk:
                assert_equal(dev.scan(20), [w[:nq] for w in want], f"nq={nq}")
            else:
                assert_equal(dev.range(rs.radii(128, 16)[1]), rwant[nq - 1], f"nq={nq}", RANGE)
        big = resident + 5
        assert rs.plan_pieces(big, 16, resident) == 1
        idx = np.arange(big) % 3
        dev = Dev(o, ctx, xq[idx], rows[idx])
        if kk:
            assert_equal(dev.scan(20), [w[idx] for w in want], f"nq={big}")
        else:
            lims, D, L = dev.range(rs.radii(128, 16)[1])
            l3, D3, L3 = rwant[2]  # the three rows' slots, hits and labels: the batch repeats them
            per = np.diff(l3.astype(np.int64)).reshape(3, 16)[idx].reshape(-1)
            seg = [slice(int(l3[r * 16]), int(l3[(r + 1) * 16])) for r in range(3)]
            tiled = (np.concatenate([[0], np.cumsum(per)]).astype(np.uint64), np.concatenate([D3[seg[r]] for r in idx]),
                     np.concatenate([L3[seg[r]] for r in idx]))
            assert_equal((lims, D, L), tiled, f"range nq={big}", RANGE)
    o4 = rs.obj(4, 4)
    wide, xq2 = ir.probe_rows(2, 1024), rs.queries(4, 2)
    dev = Dev(o4, ctx, xq2, wide)
    assert_equal(dev.scan(256), scan_model(o4, xq2, wide, 256), "nprobe=1024 k=256")
    assert_equal(dev.range(rs.radii(4, 4)[1]), range_model(o4, xq2, wide, rs.radii(4, 4)[1]), "nprobe=1024", RANGE)


@pytest.fixture(scope="module")
def small():
    """a context created under VIDC_NUM_CU=1, pool poison on, running on torch's stream (the idiom of tests/test_gpu_small_grid.py)"""
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


def test_one_cu_context_slots_go_round(small):
    """every slot takes several items; the runs and counts of a call come from scratch that was handed out full of 0xFF"""
    b = rs.ONE_CU
    o = rs.obj(b["d"], b["M"])
    rows, xq = ir.probe_rows(8, b["nprobe"]), rs.queries(b["d"], 8)
    radius = rs.radii(b["d"], b["M"])[1]
    want = scan_model(o, xq, rows, b["k"])
    for nq in (b["nq_cut"], b["nq_whole"], b["nq_cut"]):  # (the second cut call gets the first one's block back from the cache)
        idx = (np.arange(nq) * 3) % 8
        dev = Dev(o, small, xq[idx], rows[idx])
        assert_equal(dev.scan(b["k"]), [w[idx] for w in want], f"one CU nq={nq}")
        assert_equal(dev.range(radius), range_model(o, xq[idx], rows[idx], radius), f"one CU range nq={nq}", RANGE)


def test_damaged_offsets(ctx):
    """offsets that decrease, or that exceed ntotal, under rows that hold probes of -1, nlist and 2^40: the calls return, the guard
    bands hold, and the context still works"""
    o, xq = rs.obj(128, 16), rs.queries(128, len(rs.EDGE_ROWS))
    assert {-1, o["nlist"], 2 ** 40} <= set(rs.EDGE_ROWS.reshape(-1).tolist())
    off = np.asarray(o["offsets"]).copy()
    for bad in (off[::-1].copy(), off + np.uint64(o["ntotal"]), np.where(np.arange(off.size) % 2, np.uint64(2 ** 63), off),
                np.full_like(off, np.uint64(2 ** 64 - 1))):
        dev = Dev(o, ctx, xq, rs.EDGE_ROWS, offsets=bad)
        got = dev.scan(64)
        assert (got[2][:, 1] <= len(ir.EDGE_SIZES) * o["ntotal"]).all()
        lims = dev.count(np.inf)
        dev.fill(np.inf, lims, int(lims[-1]))
        dev.fill(np.inf, lims, int(lims[-1]) // 2)
    dev = Dev(o, ctx, xq, rs.EDGE_ROWS)
    assert_equal(dev.scan(64), scan_model(o, xq, rs.EDGE_ROWS, 64), "after the damaged calls")


def test_float_data(ctx):
    """normal vectors, codebooks and centroids.  With r computed in float32 by numpy and the rest in float64 the kernel's distance
    is within (d + M + 2) * 2^-23 relative of the exact value: every term is non-negative, and the bound covers the roundings of the
    d differences and squares, the d additions inside the entries and the M additions of the entries."""
    rng = np.random.default_rng(5)
    sizes, d, M, nq = (100, 0, 257, 64, 1, 5, 300), 24, 6, 7
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n, nlist = int(off[-1]), len(sizes)
    cb = rng.normal(size=(M, 256, d // M)).astype(np.float32)
    cent = rng.normal(size=(nlist, d)).astype(np.float32)
    cent[6] = cent[5]
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    codes[int(off[6]): int(off[6]) + 5] = codes[int(off[5]): int(off[6])]  # the 5-code list again, at the head of the 300-code list
    o = dict(offsets=off, ntotal=n, nlist=nlist, codes=codes, codebooks=cb, centroids=cent, d=d, M=M)
    xq = rng.normal(size=(nq, d)).astype(np.float32)
    probes = np.tile(np.array([[6, 4, 2, 0, 3, 1, 5]], np.int64), (nq, 1))
    lists = rs.list_of_rows(off, n)
    r = (xq[:, None, :] - cent[lists][None, :, :]).astype(np.float32)  # [nq, n, d], float32 as the kernel's
    exact = ((r.astype(np.float64) - rs.decode(codes, cb).astype(np.float64)[None]) ** 2).sum(2)
    bound = (d + M + 2) * 2.0 ** -23
    dev = Dev(o, ctx, xq, probes)
    for k in (10, 256):
        D, L, st = dev.scan(k)
        assert (st == [7, n]).all() and (L >= 0).all()
        pos = off[(L >> 32)].astype(np.int64) + (L & 0xFFFFFFFF)
        ex = np.take_along_axis(exact, pos, 1)
        assert (np.abs(D.astype(np.float64) - ex) <= bound * ex).all(), float((np.abs(D - ex) / ex).max())
        for q in range(nq):
            assert len(set(L[q].tolist())) == k and all((D[q, i], L[q, i]) < (D[q, i + 1], L[q, i + 1]) for i in range(k - 1))
            assert D[q, -1] <= np.sort(exact[q])[k - 1] * (1 + bound)  # nothing clearly better was left out
    # every range hit's distance is the scan's for the same label, bit for bit (k = 256: every hit below the radius is in the scan)
    radius = float(D[:, 200].min())
    lims, rD, rL = dev.range(radius)
    assert rD.size >= 200 * 1 and (rD < np.float32(radius)).all()
    for q in range(nq):
        mine = {int(l): b for l, b in zip(L[q], D[q].view(np.uint32))}
        a, b = int(lims[q * 7]), int(lims[(q + 1) * 7])
        assert b - a == int((D[q] < np.float32(radius)).sum())
        assert all(mine[int(l)] == bits for l, bits in zip(rL[a:b], rD[a:b].view(np.uint32)))
    # identical code rows in the 5-code and the 300-code list, equal centroids: identical bits (all candidates: radius +inf)
    lims, rD, rL = dev.range(np.inf)
    assert rD.size == nq * n
    bits = [{int(l): b for l, b in zip(rL[q * n:(q + 1) * n], rD[q * n:(q + 1) * n].view(np.uint32))} for q in range(nq)]
    assert all(bits[q][(5 << 32) | i] == bits[q][(6 << 32) | i] for q in range(nq) for i in range(5))
    # a cut call and an uncut one: the same bits
    resident = rs.plan_resident(ctx.num_cu(), rs.plan_lds(10, 7, d, M))
    assert rs.plan_pieces(nq, 7, resident) == 4
    big = resident + 3
    idx = np.arange(big) % nq
    cutD, cutL, _ = dev.scan(10)
    D1, L1, _ = Dev(o, ctx, xq[idx], probes[idx]).scan(10)
    assert_equal((D1, L1), (cutD[idx], cutL[idx]), "the uncut call against the cut one")


# ------------------------------------------------------------------------------------------------ IVFIndex(..., by_residual=True)
CONTAINERS = ("array", "packed", "roc", "ef", "wt")


def make_index(name, container, by_residual=True):
    """an IVFIndex over a shape's vectors with grid centroids and grid PQ codebooks, its lists in the given container"""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch, s = _t(), rs.shape(name)
    idx = IVFIndex(s["d"], s["nlist"], ("PQ", s["M"]), by_residual=by_residual)
    idx.centroids = torch.from_numpy(s["centroids"].copy()).cuda()
    idx.pq = torch.from_numpy(s["codebooks"].copy()).cuda()
    idx.add(s["x"][:1500].copy())
    cls = {"packed": ci.CompressedIDInvertedListsPackedBits, "roc": ci.CompressedIDInvertedListsFenwickTree,
           "ef": ci.CompressedIDInvertedListsEliasFano, "wt": ci.CompressedIDInvertedListsWaveletTree}.get(container)
    if cls is not None:
        idx.replace_invlists(cls(idx.invlists))
    idx.nprobe, idx.parallel_mode = s["nprobe"], 3
    return idx


def compare_with_the_model_and_the_parent(idx, s, what):
    torch = _t()
    from vector_db_id_compression_amd import ivf_range
    from vector_db_id_compression_amd.invlists import to_csr

    k, xq = s["k"], s["xq"]
    off, codes = idx._device_lists()
    vecs = rs.stored(off, codes.cpu().numpy(), s["codebooks"], s["centroids"])  # decoded residual + centroid, from the index's own codes
    probes = torch.cdist(torch.from_numpy(xq.copy()).cuda(), idx.centroids).topk(idx.nprobe, largest=False).indices
    pn = probes.cpu().numpy()
    want = ir.model(off, vecs, xq, pn, k)
    free = ir.tie_free(off, vecs, xq, pn, k)
    D, labels = idx.scan_device(xq, k)
    assert D.is_cuda and labels.is_cuda and D.dtype == torch.float32 and labels.dtype == torch.int64
    assert_equal((D.cpu().numpy(), labels.cpu().numpy()), want[:2], f"{what}: scan_device against the model")
    D2, labels2 = idx.scan_device(torch.from_numpy(xq.copy()).cuda(), k, probes=probes)  # given probes are used as they are
    assert torch.equal(D2, D) and torch.equal(labels2, labels)
    pD, pL = idx._scan(xq, k)
    assert np.array_equal(D.cpu().numpy(), pD), f"{what}: D differs from _scan"
    assert np.array_equal(labels.cpu().numpy()[free], pL[free]), f"{what}: labels differ from _scan on tie-free queries"
    sD, sI = idx.search_device(xq, k)
    assert sD.is_cuda and sI.is_cuda and torch.equal(sD, D)
    rD, rI = idx.search_defer_id_decoding(xq, k)
    assert np.array_equal(sD.cpu().numpy(), rD) and np.array_equal(sI.cpu().numpy()[free], rI[free]), f"{what}: search_device against the parent"
    il = idx.invlists
    ids = il.get_ids_all().cpu().numpy().view(np.int64) if hasattr(il, "get_ids_all") else to_csr(il)[1].view(np.int64)
    off64 = np.asarray(off, np.int64)
    wl = want[1]
    wI = np.where(wl >= 0, ids[off64[np.maximum(wl, 0) >> 32] + (np.maximum(wl, 0) & 0xFFFFFFFF)], -1)
    assert np.array_equal(sI.cpu().numpy(), wI), f"{what}: ids differ from the model's labels translated"
    # the range search, ids included: a radius that lets some of every query's top k through
    radius = float(np.median(want[0][np.isfinite(want[0])]))
    wlims, wD, wL = rr.model(off, vecs, xq, pn, radius)
    lims, gD, gI = ivf_range.range_search_device(idx, xq, radius)
    assert 0 < wD.size and np.array_equal(lims.cpu().numpy().view(np.uint64), wlims[::idx.nprobe])
    assert_equal((gD.cpu().numpy(), gI.cpu().numpy()), (wD, ids[off64[wL >> 32] + (wL & 0xFFFFFFFF)]), f"{what}: range_search_device", ("D", "ids"))
    # reconstruct_batch: the decoded residual plus the centroid, exactly
    pick = np.arange(0, ids.size, 29)
    got = idx.reconstruct_batch(torch.from_numpy(ids[pick].copy()).cuda() if hasattr(il, "locate_batch") else ids[pick]).cpu().numpy()
    assert np.array_equal(got, vecs[pick]), f"{what}: reconstruct_batch"
    return int(free.sum())


@pytest.mark.parametrize("container", CONTAINERS)
def test_index_by_residual(container):
    s = rs.shape("distinct")
    idx = make_index("distinct", container)
    assert compare_with_the_model_and_the_parent(idx, s, container) * 2 >= s["nq"]
    # codes_all moves: add, remove, add
    torch = _t()
    idx.add(s["x"][1500:1800].copy())
    if container != "wt":  # (a wavelet tree holds a permutation: no removal)
        assert idx.remove_ids(torch.arange(100, 400, 3, dtype=torch.int64).cuda() if container != "array" else np.arange(100, 400, 3)) == 100
    idx.add(s["x"][1800:].copy())
    compare_with_the_model_and_the_parent(idx, s, f"{container} after add / remove / add")
    compare_with_the_model_and_the_parent(make_index("ties", container), rs.shape("ties"), f"{container} ties")


def test_the_flag_is_part_of_an_index_and_raw_pq_is_untouched():
    torch = _t()
    s = rs.shape("distinct")
    res, raw = make_index("distinct", "array"), make_index("distinct", "array", by_residual=False)
    with pytest.raises(ValueError, match="by_residual"):
        res.merge_from(raw)
    with pytest.raises(ValueError, match="by_residual"):
        raw.copy_subset_to(res, 0, 0, 10)
    assert not torch.equal(res._device_lists()[1], raw._device_lists()[1])  # (the residual was encoded, not the vector)
    # the control: the raw-PQ index on the same data gives what the raw model gives
    off, codes = raw._device_lists()
    vecs = rs.decode(codes.cpu().numpy(), s["codebooks"])
    probes = torch.cdist(torch.from_numpy(s["xq"].copy()).cuda(), raw.centroids).topk(raw.nprobe, largest=False).indices
    D, labels = raw.scan_device(s["xq"], s["k"])
    assert_equal((D.cpu().numpy(), labels.cpu().numpy()), ir.model(off, vecs, s["xq"], probes.cpu().numpy(), s["k"])[:2], "raw PQ")
