"""The IVF list scan on the device (vidc_ivf_scan_dev, IVFIndex.scan_device / search_device) against the numpy model
(tests/ivf_scan_ref.py) and against the per-query torch scan it stands beside (IVFIndex._scan).  Data are integer grids, so D, labels
and stats are compared element for element, ties included.  Calls that go through the C-ABI directly write into guarded, poisoned
buffers; the d2h counter does not move; the inputs are the same before and after.  Shapes, designed objects and the one-CU batches are
the ones the CPU tests hold to their purpose."""
import numpy as np
import pytest

import contract_ref as cr
import ivf_scan_ref as ir
from test_ivf_scan_abi_cpu import ONE_CU
from test_ivf_scan_ref_cpu import DIMS, KS, NPROBES, PQ_FORMS

pytestmark = pytest.mark.gpu

INVALID = -1


def _t():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


def call_abi(o, ctx, xq, probes, k, want_stats=True, status=0, misalign=0, offsets=None, over=None):
    """the C call into guarded buffers -> (D, labels, stats) numpy; guards, inputs and the d2h counter are checked.  status != 0: the
    call must return it, name "scan" and write nothing.  misalign: bytes the code array is shifted by.  The codes lie between guard
    bands of their own.  over: arguments replaced in the call (nlist, ntotal, kind, d, M, nprobe, and None for an array)."""
    torch, lib = _t(), _L()
    nq, nprobe = probes.shape
    code_bytes = o["codes"].size
    pad = 4096 + misalign
    band = torch.full((pad + code_bytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    codes = band[pad: pad + code_bytes]
    codes.copy_(torch.from_numpy(o["codes"].reshape(-1).copy()))
    assert codes.data_ptr() % 16 == misalign % 16
    off_np = np.asarray(o["offsets"] if offsets is None else offsets, dtype=np.uint64)
    off = torch.from_numpy(off_np.view(np.int64).copy()).cuda()
    cb = torch.from_numpy(o["codebooks"].copy()).cuda() if o["M"] else None
    qt = torch.from_numpy(np.ascontiguousarray(xq, dtype=np.float32).copy()).cuda()
    pt = torch.from_numpy(np.ascontiguousarray(probes, dtype=np.int64).copy()).cuda()
    wD, vD = cr.guarded((nq, max(k, 1)), np.int32, device="cuda")
    wL, vL = cr.guarded((nq, max(k, 1)), np.int64, device="cuda")
    wS, vS = cr.guarded((nq, 2), np.int32, device="cuda")
    a = dict(nlist=o["nlist"], off=lib.ptr(off), ntotal=o["ntotal"], codes=lib.ptr(codes) if code_bytes else lib.ptr(band), kind=o["kind"],
             d=o["d"], M=o["M"], cb=lib.ptr(cb), nq=nq, xq=lib.ptr(qt), nprobe=nprobe, probes=lib.ptr(pt), k=k, D=lib.ptr(vD),
             labels=lib.ptr(vL), stats=lib.ptr(vS) if want_stats else None)
    a.update(over or {})
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d2h = ctx.d2h_bytes()
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_scan_dev(ctx.h, a["nlist"], a["off"], a["ntotal"], a["codes"], a["kind"], a["d"], a["M"], a["cb"], a["nq"], a["xq"],
                                     a["nprobe"], a["probes"], a["k"], a["D"], a["labels"], a["stats"])
    torch.cuda.synchronize()
    what = f"kind={o['kind']} d={o['d']} M={o['M']} nq={nq} nprobe={nprobe} k={k} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    assert ctx.d2h_bytes() == d2h, f"{what}: the scan moved payload to the host"
    bandh = band.cpu().numpy()
    assert (bandh[:pad] == 0x5A).all() and (bandh[pad + code_bytes:] == 0x5A).all(), f"{what}: the bands around the codes changed"
    assert np.array_equal(bandh[pad: pad + code_bytes], o["codes"].reshape(-1)), f"{what}: the codes changed"
    assert np.array_equal(off.cpu().numpy().view(np.uint64), off_np) and np.array_equal(pt.cpu().numpy(), probes), f"{what}: inputs changed"
    assert np.array_equal(qt.cpu().numpy(), np.asarray(xq, dtype=np.float32)), f"{what}: the queries changed"
    if status:
        assert b"scan" in lib.lib().vidc_last_error(), lib.lib().vidc_last_error()
        for w, v in ((wD, vD), (wL, vL), (wS, vS)):
            cr.assert_untouched(w, v, what)
        return None
    for w, v, name in ((wD, vD, "D"), (wL, vL, "labels"), (wS, vS, "stats")):
        cr.assert_guards_intact(w, v, f"{what}: {name}")
    if not want_stats:
        cr.assert_untouched(wS, vS, what)
    return vD.view(torch.float32).cpu().numpy().copy(), vL.cpu().numpy().copy(), vS.cpu().numpy().view(np.uint32).copy()


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("D", "labels", "stats")):
        w = np.asarray(w)
        bad = np.argwhere(np.asarray(g) != w)
        assert np.asarray(g).shape == w.shape and bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} elements)"


def check(o, ctx, xq, probes, k, what, **kw):
    assert_equal(call_abi(o, ctx, xq, probes, k, **kw), ir.model(o["offsets"], o["vecs"], xq, probes, k), what)


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


FORMS = [(d, 0) for d in DIMS] + [(M * dsub, M) for M, dsub in PQ_FORMS]


@pytest.mark.parametrize("d,M", FORMS)
def test_designed_objects_through_the_abi(ctx, d, M):
    """list sizes around the trip, short lists against k, invalid and repeated probes: every d of FLAT, every (M, dsub) of PQ8"""
    o, xq = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS))
    check(o, ctx, xq, ir.EDGE_ROWS, 64, f"d={d} M={M}")
    got = call_abi(o, ctx, xq, ir.EDGE_ROWS, 10, want_stats=False)  # no stats array
    assert_equal(got[:2], ir.model(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, 10)[:2], f"d={d} M={M} no stats")


@pytest.mark.parametrize("M", (0, 4))
def test_every_k_and_every_nprobe(ctx, M):
    o, xq = ir.obj(4, M), ir.queries(4, len(ir.EDGE_ROWS))
    for k in KS:
        check(o, ctx, xq, ir.EDGE_ROWS, k, f"M={M} k={k}")
    for nprobe in NPROBES:
        check(o, ctx, ir.queries(4, 6), ir.probe_rows(6, nprobe), 20, f"M={M} nprobe={nprobe}")
    check(o, ctx, ir.queries(4, 2), ir.probe_rows(2, 1024), 256, f"M={M} nprobe=1024 k=256")


@pytest.mark.parametrize("name", sorted(ir.SHAPES))
def test_shapes_through_the_abi(ctx, name):
    s = ir.shape(name)
    assert_equal(call_abi(s, ctx, s["xq"], s["probes"], s["k"]), ir.expected(name), name)


def test_alignment_and_small_batches(ctx):
    """a FLAT code array 4 bytes off (the scalar-load path) and PQ codes 4 and 1 bytes off (narrower code loads); nq = 1, 2, 3 with 16
    probes, so that the row is cut, and the same probes in a batch large enough for one piece per query"""
    for d in (4, 20, 128):
        check(ir.obj(d), ctx, ir.queries(d, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, 64, f"FLAT d={d} misaligned", misalign=4)
    for mis in (4, 1, 8):
        check(ir.obj(128, 16), ctx, ir.queries(128, len(ir.EDGE_ROWS)), ir.EDGE_ROWS, 64, f"PQ misaligned by {mis}", misalign=mis)
    num_cu = ctx.num_cu()
    for d, M in ((4, 0), (128, 16)):
        o = ir.obj(d, M)
        resident = ir.plan_resident(num_cu, ir.plan_lds(o["kind"], 20, 16, d, M))
        big = resident + 5
        rows, xq = ir.probe_rows(3, 16), ir.queries(d, 3)
        want = ir.model(o["offsets"], o["vecs"], xq, rows, 20)
        for nq in (1, 2, 3):
            assert ir.plan_pieces(nq, 16, resident) > 1
            assert_equal(call_abi(o, ctx, xq[:nq], rows[:nq], 20), [w[:nq] for w in want], f"M={M} nq={nq}")
        assert ir.plan_pieces(big, 16, resident) == 1
        idx = np.arange(big) % 3
        assert_equal(call_abi(o, ctx, xq[idx], rows[idx], 20), [w[idx] for w in want], f"M={M} nq={big}")


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


@pytest.mark.parametrize("kind", sorted(ONE_CU))
def test_one_cu_context_slots_go_round(small, kind):
    """every slot takes several items; the runs of a cut call come from scratch that was handed out full of 0xFF"""
    b = ONE_CU[kind]
    o = ir.obj(b["d"], b["M"])
    rows, xq = ir.probe_rows(8, b["nprobe"]), ir.queries(b["d"], 8)
    want = ir.model(o["offsets"], o["vecs"], xq, rows, b["k"])
    for nq in (b["nq_cut"], b["nq_whole"], b["nq_cut"]):  # (the second cut call gets the first one's block back from the cache)
        idx = (np.arange(nq) * 3) % 8
        assert_equal(call_abi(o, small, xq[idx], rows[idx], b["k"]), [w[idx] for w in want], f"{kind} one CU nq={nq}")


def test_damaged_offsets(ctx):
    """offsets that decrease, or that exceed ntotal: the call returns, nothing outside the codes is read or written that the guard
    bands could show, and the context still works"""
    for d, M in ((4, 0), (128, 16)):
        o = ir.obj(d, M)
        off = np.asarray(o["offsets"]).copy()
        xq = ir.queries(d, len(ir.EDGE_ROWS))
        for bad in (off[::-1].copy(), off + np.uint64(o["ntotal"]), np.where(np.arange(off.size) % 2, np.uint64(2 ** 63), off),
                    np.full_like(off, np.uint64(2 ** 64 - 1))):
            got = call_abi(o, ctx, xq, ir.EDGE_ROWS, 64, offsets=bad)
            assert got is not None and (got[2][:, 1] <= len(ir.EDGE_SIZES) * o["ntotal"]).all()
        check(o, ctx, xq, ir.EDGE_ROWS, 64, f"M={M} after the damaged calls")


def test_refusals_on_a_live_context(ctx):
    o, xq = ir.obj(128, 16), ir.queries(128, 5)
    rows = ir.probe_rows(5, 3)
    for kw in (dict(off=None), dict(codes=None), dict(xq=None), dict(probes=None), dict(D=None), dict(labels=None), dict(k=0), dict(k=257),
               dict(nprobe=0), dict(nprobe=1025), dict(d=0), dict(d=2049), dict(ntotal=2 ** 32), dict(nlist=2 ** 31), dict(kind=2),
               dict(M=0), dict(M=65), dict(M=3), dict(cb=None)):
        k = kw.pop("k", 20)
        call_abi(o, ctx, xq, rows, k, status=INVALID, over=kw)
    lib = _L()
    assert lib.lib().vidc_ivf_scan_dev(ctx.h, 8, None, 0, None, 0, 4, 0, None, 0, None, 3, None, 20, None, None, None) == 0  # nq == 0
    check(o, ctx, xq, rows, 20, "after the refusals")
    empty = ir.obj(4, 0, sizes=(0, 0, 0))  # no codes at all: every result is padding
    D, L, st = call_abi(empty, ctx, ir.queries(4, 3), ir.probe_rows(3, 3, nlist=3), 5)
    assert np.isinf(D).all() and (L == -1).all() and (st[:, 1] == 0).all()


def test_float_data(ctx):
    """random float vectors: the order is (distance, label) on the kernel's own distances, which are the float32 sum within the
    summation bound of the exact value"""
    rng = np.random.default_rng(5)
    sizes, d, k = (100, 0, 257, 64, 1), 24, 10
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    for M in (0, 6):
        if M:
            cb = rng.normal(size=(M, 256, d // M)).astype(np.float32)
            codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
            vecs = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)
        else:
            cb, vecs = None, rng.normal(size=(n, d)).astype(np.float32)
            codes = vecs.view(np.uint8).reshape(n, 4 * d).copy()
        o = dict(offsets=off, ntotal=n, nlist=len(sizes), codes=codes, vecs=vecs, codebooks=cb, d=d, M=M, kind=ir.PQ8 if M else ir.FLAT)
        xq = rng.normal(size=(7, d)).astype(np.float32)
        probes = np.tile(np.array([[4, 2, 0, 3]], np.int64), (7, 1))
        D, L, st = call_abi(o, ctx, xq, probes, k)
        assert (st == [4, n]).all() and (L >= 0).all()
        pos = off[(L >> 32)].astype(np.int64) + (L & 0xFFFFFFFF)
        exact = ((vecs[pos].astype(np.float64) - xq[:, None, :].astype(np.float64)) ** 2).sum(2)
        # float32 sum of d squares of float32 differences: (d + 2) roundings of 2^-24 relative each, all terms non-negative
        assert (np.abs(D.astype(np.float64) - exact) <= (d + 2) * 2.0 ** -23 * exact).all()
        for q in range(7):
            assert len(set(L[q].tolist())) == k and all((D[q, i], L[q, i]) < (D[q, i + 1], L[q, i + 1]) for i in range(k - 1))
            allx = ((vecs.astype(np.float64) - xq[q].astype(np.float64)) ** 2).sum(1)
            assert D[q, -1] <= np.sort(allx)[k - 1] * (1 + (d + 2) * 2.0 ** -23)  # nothing clearly better was left out


# ------------------------------------------------------------------------------------------------ against the per-query torch scan
CONTAINERS = ("array", "packed", "roc", "ef", "wt")


def make_index(name, pq, container):
    """an IVFIndex over a shape's vectors with grid centroids (and grid PQ codebooks), its lists in the given container"""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch, s = _t(), ir.shape(name)
    M = 0 if not pq else (4 if s["d"] == 16 else 2)
    idx = IVFIndex(s["d"], s["nlist"], ("PQ", M) if M else "Flat")
    idx.centroids = torch.from_numpy(s["centroids"].copy()).cuda()
    if M:
        cb = np.random.default_rng(77).integers(-s["R"], s["R"] + 1, size=(M, 256, s["d"] // M)).astype(np.float32)
        idx.pq = torch.from_numpy(cb).cuda()
    idx.add(s["x"][:1500].copy())
    cls = {"packed": ci.CompressedIDInvertedListsPackedBits, "roc": ci.CompressedIDInvertedListsFenwickTree,
           "ef": ci.CompressedIDInvertedListsEliasFano, "wt": ci.CompressedIDInvertedListsWaveletTree}.get(container)
    if cls is not None:
        idx.replace_invlists(cls(idx.invlists))
    idx.nprobe, idx.parallel_mode = s["nprobe"], 3
    return idx


def compare_with_the_parent(idx, s, what):
    torch = _t()
    from vector_db_id_compression_amd.invlists import to_csr

    k, xq = s["k"], s["xq"]
    off, codes = idx._device_lists()
    vecs = idx._decode_codes(codes).cpu().numpy()
    probes = torch.cdist(torch.from_numpy(xq.copy()).cuda(), idx.centroids).topk(idx.nprobe, largest=False).indices
    want = ir.model(off, vecs, xq, probes.cpu().numpy(), k)
    free = ir.tie_free(off, vecs, xq, probes.cpu().numpy(), k)
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
    wl = want[1]
    wI = np.where(wl >= 0, ids[np.asarray(off, np.int64)[np.maximum(wl, 0) >> 32] + (np.maximum(wl, 0) & 0xFFFFFFFF)], -1)
    assert np.array_equal(sI.cpu().numpy(), wI), f"{what}: ids differ from the model's labels translated"
    return int(free.sum())


@pytest.mark.parametrize("pq", (False, True), ids=("flat", "pq"))
@pytest.mark.parametrize("container", CONTAINERS)
def test_against_the_parent_path(container, pq):
    s = ir.shape("distinct")
    idx = make_index("distinct", pq, container)
    nfree = compare_with_the_parent(idx, s, f"{container} pq={pq}")
    if not pq:
        assert nfree * 2 >= s["nq"]
    # codes_all moves: add, remove, add
    torch = _t()
    idx.add(s["x"][1500:1800].copy())
    if container != "wt":  # (a wavelet tree holds a permutation: no removal)
        assert idx.remove_ids(torch.arange(100, 400, 3, dtype=torch.int64).cuda() if container != "array" else np.arange(100, 400, 3)) == 100
    idx.add(s["x"][1800:].copy())
    compare_with_the_parent(idx, s, f"{container} pq={pq} after add / remove / add")
    t = ir.shape("ties")
    compare_with_the_parent(make_index("ties", pq, container), t, f"{container} pq={pq} ties")
