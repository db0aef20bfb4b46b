"""The coarse quantiser on the device (vidc_ivf_probe_dev, ivf_probe.probe_device) against a float64 reference written out here:
dist = ((xq[:, None] - c[None]) ** 2).sum(-1), order by np.lexsort((list, dist)), pad with -1 / inf.  Integer-grid inputs
(coordinates in [-R, R], d * (2R)^2 < 2^24) make the kernel's float32 expansion exact, so probes and distances are compared with ==.
Centroid rows are drawn from a few distinct rows and one more pair is made equal where it matters, so every integer fixture has a tie
inside a top-nprobe (where nprobe and nlist are at least 2) and one across position nprobe (where nprobe < nlist): ties go by list
number.  Every call goes through the C-ABI into guarded outputs with the d2h counter held."""
import numpy as np
import pytest

import contract_ref as cr

pytestmark = pytest.mark.gpu

INVALID = -1
TQ = {1: 32, 64: 32, 65: 16, 256: 16}  # the plan's query tile (csrc/ivf_probe_plan.h: tile_queries)


def _t():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


def ref(xq, c, nprobe):
    """-> (probes int64 [nq, nprobe], dist float64 [nq, nprobe], the whole float64 distance matrix)"""
    xq, c = np.asarray(xq, np.float64), np.asarray(c, np.float64)
    dist = np.stack([((q[None] - c) ** 2).sum(-1) for q in xq]) if len(xq) else np.zeros((0, len(c)))
    order = np.lexsort((np.broadcast_to(np.arange(len(c)), dist.shape), dist))[:, :nprobe]
    probes = np.full((len(xq), nprobe), -1, np.int64)
    out = np.full((len(xq), nprobe), np.inf)
    probes[:, :order.shape[1]] = order
    out[:, :order.shape[1]] = np.take_along_axis(dist, order, 1)
    return probes, out, dist


def grid(nq, nlist, d, nprobe, R=2, seed=0):
    """integer-grid queries and centroids with ties where they can be: rows drawn from nlist / 3 distinct ones, and the centroid at
    position nprobe of query 0 made a copy of the one in front of it"""
    assert d * (2 * R) ** 2 < 2 ** 24
    rng = np.random.default_rng(1000 * seed + nq + nlist + d + nprobe)
    base = rng.integers(-R, R + 1, size=(max(1, nlist // 3), d)).astype(np.float32)
    c = base[rng.integers(0, len(base), nlist)]
    xq = rng.integers(-R, R + 1, size=(nq, d)).astype(np.float32)
    if nprobe < nlist:
        o = ref(xq[:1], c, nprobe + 1)[0][0]
        c[o[nprobe]] = c[o[nprobe - 1]]
    P, D, dist = ref(xq, c, nprobe)
    if min(nprobe, nlist) >= 2:
        assert (D[:, 1:min(nprobe, nlist)] == D[:, :min(nprobe, nlist) - 1]).any(), "no tie inside a top-nprobe"
    if nprobe < nlist:
        assert (np.sort(dist, 1)[:, nprobe] == D[:, nprobe - 1]).any(), "no tie across position nprobe"
    return xq, c, (P, D)


def shifted(a, mis):
    """a on the device, its first byte `mis` bytes behind a 16-byte boundary"""
    torch = _t()
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
    v = buf[mis // 4: mis // 4 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == mis
    return v


def call(ctx, xq, c, nprobe, status=0, mis=0, cdist=True, over=None):
    """vidc_ivf_probe_dev into guarded outputs -> (probes, cdist or None); a refusal leaves both untouched"""
    torch, lib = _t(), _L()
    nq = len(xq)
    ct, qt = shifted(c, mis), shifted(xq, mis)
    wP, vP = cr.guarded((max(nq * nprobe, 1),), np.int64, device="cuda")
    wD, vD = cr.guarded((max(nq * nprobe, 1),), np.int32, device="cuda")
    a = dict(ctx=ctx.h, nlist=len(c), cent=lib.ptr(ct), d=c.shape[1], nq=nq, xq=lib.ptr(qt), nprobe=nprobe, probes=lib.ptr(vP),
             cdist=lib.ptr(vD) if cdist else None)
    a.update(over or {})
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d2h = ctx.d2h_bytes()
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_probe_dev(a["ctx"], a["nlist"], a["cent"], a["d"], a["nq"], a["xq"], a["nprobe"], a["probes"], a["cdist"])
    torch.cuda.synchronize()
    what = f"nq={nq} nlist={len(c)} d={c.shape[1]} nprobe={nprobe} mis={mis} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    assert ctx.d2h_bytes() == d2h, f"{what}: the d2h counter moved"
    assert np.array_equal(ct.cpu().numpy(), c) and np.array_equal(qt.cpu().numpy(), xq), f"{what}: the inputs changed"
    if status or nq == 0 or not cdist:
        cr.assert_untouched(wD, vD, what)
    if status or nq == 0:
        cr.assert_untouched(wP, vP, what)
        return None, None
    cr.assert_guards_intact(wP, vP, f"{what}: probes")
    cr.assert_guards_intact(wD, vD, f"{what}: cdist")
    return vP.cpu().numpy().reshape(nq, nprobe), (vD.view(torch.float32).cpu().numpy().reshape(nq, nprobe) if cdist else None)


def assert_exact(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: probes differ at {np.argwhere(got[0] != want[0])[:4].tolist()}"
    if got[1] is not None:
        assert got[1].dtype == np.float32 and np.array_equal(got[1].astype(np.float64), want[1]), f"{what}: distances differ"
    assert ((got[0] >= -1) & (got[0] < 2 ** 31)).all()


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


@pytest.fixture(scope="module")
def small():
    """a context created under VIDC_NUM_CU=1, pool poison on, on torch's stream (the idiom of tests/test_gpu_ivf_scan.py)"""
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


# every value of nq {1, 15, 17, 33, 100}, nlist {1, 63, 65, 129, 257, 1000}, d {1, 3, 4, 33, 130}, nprobe {1, 64, 65, 256} appears;
# nprobe > nlist (the -1 / +inf tail) in four of them
SEAMS = [(1, 1, 1, 1), (15, 63, 3, 64), (17, 65, 4, 65), (33, 129, 33, 256), (100, 257, 130, 1), (33, 1000, 4, 64), (17, 1000, 130, 256),
         (100, 1000, 3, 65), (1, 63, 33, 65)]


@pytest.mark.parametrize("nq,nlist,d,nprobe", SEAMS)
def test_tile_seams_exact(ctx, nq, nlist, d, nprobe):
    xq, c, want = grid(nq, nlist, d, nprobe)
    assert_exact(call(ctx, xq, c, nprobe), want, "seams")


@pytest.mark.parametrize("nprobe", (1, 64, 65, 256))
def test_ties_go_by_list_number(ctx, nprobe):
    """R = 1; one centroid row copied across tile boundaries and to the last list.  The default context cuts the 40 tiles into S = 32
    pieces of one or two: 127 | 128 and 639 | 640 are piece boundaries, 511 | 512 lies inside piece 3"""
    xq, c, _ = grid(5, 5000, 6, nprobe, R=1, seed=1)
    lead = [127, 128, 511, 512, 639, 640, 4999]
    xq[0] = 3.0  # (off the grid of the other rows)
    c[lead] = xq[0]  # the only centroids at distance 0 of query 0: they lead its row, in list order
    got = call(ctx, xq, c, nprobe)
    assert_exact(got, ref(xq, c, nprobe)[:2], "ties")
    lead = lead[:nprobe]
    assert got[0][0, :len(lead)].tolist() == lead and not got[1][0, :len(lead)].any()
    assert ctx.last_kernel_ms() > 0


@pytest.mark.parametrize("nprobe", (1, 64, 65, 256))
def test_the_cut(ctx, small, nprobe):
    """nq = 3, nlist = 5000: the default context cuts the centroid range and the merge runs; the one-CU context takes 5 TQ + 3 queries
    uncut, more than two trips of the grid-stride loop and a ragged last tile, from poisoned scratch.  Equal to the reference and
    bit-equal between the contexts"""
    nq = 5 * TQ[nprobe] + 3
    xq, c, want = grid(nq, 5000, 8, nprobe, seed=2)
    a = call(ctx, xq[:3], c, nprobe)
    assert_exact(a, (want[0][:3], want[1][:3]), "cut")
    b = call(small, xq, c, nprobe)
    assert_exact(b, want, "one CU")
    assert np.array_equal(a[0], b[0][:3]) and np.array_equal(a[1].view(np.uint32), b[1][:3].view(np.uint32))
    assert_exact(call(small, xq[:3], c, nprobe), (want[0][:3], want[1][:3]), "one CU, three queries")


@pytest.mark.parametrize("d", (4, 33, 130))
def test_misaligned_inputs_and_no_distances(ctx, d):
    """both arrays 4 bytes off a 16-byte boundary (the 4-byte load path), and d_cdist == NULL"""
    xq, c, want = grid(17, 257, d, 64, seed=3)
    assert_exact(call(ctx, xq, c, 64, mis=4), want, "misaligned")
    assert_exact(call(ctx, xq, c, 64, mis=4, cdist=False), want, "misaligned, no cdist")
    assert_exact(call(ctx, xq, c, 64, cdist=False), want, "no cdist")


def test_float_data_within_the_summation_bound(ctx, small):
    """Gaussian data: every returned distance within E(q, c) = (d + 4) 2^-24 (|q| + |c|)^2 of the float64 value; rows ascend in
    (distance, list); a returned list's float64 distance is at most the float64 nprobe-th smallest + E(q, c) + max_c E(q, c) (a true
    top list t it displaced has computed(l) <= computed(t)), which is within the 2 E of the statement; both contexts agree bit for bit"""
    d, nlist, nq, nprobe = 96, 777, 40, 32
    rng = np.random.default_rng(5)
    c, xq = rng.standard_normal((nlist, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    _, _, exact = ref(xq, c, nprobe)
    nrm = lambda a: np.sqrt((a.astype(np.float64) ** 2).sum(-1))
    E = (d + 4) * 2.0 ** -24 * (nrm(xq)[:, None] + nrm(c)[None]) ** 2
    P, D = call(ctx, xq, c, nprobe)
    assert ((P >= 0) & (P < nlist)).all()
    err = np.abs(D.astype(np.float64) - np.take_along_axis(exact, P, 1))
    print("largest error / E:", float((err / np.take_along_axis(E, P, 1)).max()))
    assert (err <= np.take_along_axis(E, P, 1)).all()
    key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | P.astype(np.uint64)
    assert (key[:, 1:] > key[:, :-1]).all()
    kth = np.sort(exact, 1)[:, nprobe - 1:nprobe]
    assert (np.take_along_axis(exact, P, 1) <= kth + np.take_along_axis(E, P, 1) + E.max(1, keepdims=True)).all()
    P1, D1 = call(small, xq, c, nprobe)
    assert np.array_equal(P, P1) and np.array_equal(D.view(np.uint32), D1.view(np.uint32))


@pytest.mark.parametrize("over", [dict(cent=None), dict(xq=None), dict(probes=None), dict(nprobe=0), dict(nprobe=257), dict(d=0), dict(d=2049),
                                  dict(nlist=0), dict(nlist=2 ** 31), dict(nq=2 ** 32), dict(ctx=None)], ids=str)
def test_refusals_on_a_live_context(ctx, over):
    xq, c, want = grid(5, 63, 4, 4, seed=4)
    call(ctx, xq, c, 4, status=INVALID, over=over)
    assert b"ivf probe" in _L().lib().vidc_last_error()
    call(ctx, xq[:0], c, 4)  # nq == 0: VIDC_OK, nothing written
    assert_exact(call(ctx, xq, c, 4), want, "after a refusal")


@pytest.mark.parametrize("container", ("array", "packed"))
def test_through_python_with_the_flag_on(container):
    """an integer-grid IVFIndex with coarse_device = True: search_device and range_search_device equal the same calls given the
    reference's probes, and add placed every vector in the reference's list"""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd import ivf_probe, ivf_range
    from vector_db_id_compression_amd.invlists import to_csr
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch = _t()
    d, nlist, n, nprobe = 8, 300, 2000, 5
    xq, c, (P, D) = grid(21, nlist, d, nprobe, seed=6)
    x = np.random.default_rng(8).integers(-2, 3, size=(n, d)).astype(np.float32)
    idx = IVFIndex(d, nlist)
    idx.centroids, idx.nprobe, idx.coarse_device = torch.from_numpy(c.copy()).cuda(), nprobe, True
    idx.add(x[:n // 2])
    if container == "packed":
        idx.replace_invlists(ci.CompressedIDInvertedListsPackedBits(idx.invlists))
    idx.add(x[n // 2:])
    il = idx.invlists
    off = np.asarray(idx._device_lists()[0], np.int64)
    ids = il.get_ids_all().cpu().numpy().view(np.int64) if hasattr(il, "get_ids_all") else to_csr(il)[1].view(np.int64)
    assign = np.empty(n, np.int64)
    assign[ids] = np.searchsorted(off, np.arange(n), side="right") - 1
    assert np.array_equal(assign, ref(x, c, 1)[0][:, 0])
    got_p, got_d = ivf_probe.probe_device(idx, xq)
    assert got_p.is_cuda and (got_p.dtype, got_d.dtype) == (torch.int64, torch.float32)
    assert_exact((got_p.cpu().numpy(), got_d.cpu().numpy()), (P, D), "probe_device")
    assert np.array_equal(ivf_probe.assign_device(idx, x).cpu().numpy(), assign)
    got = idx.search_device(xq, 10) + ivf_range.range_search_device(idx, xq, 9.0)
    probes = torch.from_numpy(P).cuda()
    idx._probe_rows = lambda q: probes  # the same calls, given the reference's probes
    want = idx.search_device(xq, 10) + ivf_range.range_search_device(idx, xq, 9.0)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[1].shape == (21, 10) and got[3].numel() > 21
