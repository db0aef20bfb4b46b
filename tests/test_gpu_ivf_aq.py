"""Additive-quantiser codes on the device (vidc_ivf_aq_lut_dev, vidc_ivf_scan_aq_dev, IVFIndex(d, nlist, ("RQ", M))) against the
float64 statement tests/ivf_aq_ref.py.  Grid data keep every intermediate an integer below 2^24, so float32 is exact and results are
compared by bytes; the two Gaussian checks carry rounding bounds derived in their docstrings."""
import numpy as np
import pytest

import contract_ref as cr
import ivf_aq_ref as aq
import ivf_scan_ref as ir
from test_gpu_ivf_probe import _L, _t, ctx, shifted, small  # noqa: F401  (the probe's fixtures and its misaligned upload)
from test_gpu_ivf_pqbits import ROWS, same

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def lut(ctx, cb, xq, status=0, over=None):
    """vidc_ivf_aq_lut_dev, operands 4 bytes off a 16-byte boundary, into a guarded output -> float32 [nq, M, 256]; a refusal
    leaves the output untouched"""
    torch, lib = _t(), _L()
    (M, _, d), nq = cb.shape, len(xq)
    ct, qt = shifted(cb, 4), shifted(xq, 4)
    w, v = cr.guarded((nq, M, 256), np.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    a = dict(d=d, M=M, cb=lib.ptr(ct), xq=lib.ptr(qt), lut=lib.ptr(v))
    a.update(over or {})
    st = lib.lib().vidc_ivf_aq_lut_dev(ctx.h, a["d"], a["M"], a["cb"], nq, a["xq"], a["lut"])
    torch.cuda.synchronize()
    assert st == status, (over, st, lib.lib().vidc_last_error())
    (cr.assert_untouched if status else cr.assert_guards_intact)(w, v, f"lut nq={nq} d={d} M={M} {over}")
    return v.view(torch.float32).cpu().numpy()


def scan(ctx, o, xq, probes, k, mis=0, status=0, over=None, codes=None):
    """vidc_ivf_scan_aq_dev over codes `mis` bytes off a 16-byte boundary between guard bands, into guarded outputs ->
    (D, labels, stats), or None for a refusal, which leaves the outputs untouched"""
    torch, lib = _t(), _L()
    xq, probes = np.ascontiguousarray(xq, np.float32), np.ascontiguousarray(probes, np.int64)
    codes = o["codes"] if codes is None else codes
    nbytes, pad = codes.size, 4096 + mis
    band = torch.full((pad + nbytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    band[pad:pad + nbytes].copy_(torch.from_numpy(codes.reshape(-1).copy()))
    assert band[pad:].data_ptr() % 16 == mis
    off = torch.from_numpy(np.asarray(o["offsets"], np.uint64).view(np.int64).copy()).cuda()
    cb, cent = torch.from_numpy(o["codebooks"].copy()).cuda(), torch.from_numpy(o["centroids"].copy()).cuda()
    qt, pt = torch.from_numpy(xq.copy()).cuda(), torch.from_numpy(probes.copy()).cuda()
    out = [cr.guarded((len(xq), n), t, device="cuda") for n, t in ((k or 1, np.int32), (k or 1, np.int64), (2, np.int32))]
    a = dict(M=o["M"], codes=lib.ptr(band[pad:]), cb=lib.ptr(cb), k=k)
    a.update(over or {})
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_scan_aq_dev(ctx.h, o["nlist"], lib.ptr(off), o["ntotal"], a["codes"], o["d"], a["M"], a["cb"],
                                        lib.ptr(cent) if o["res"] else None, len(xq), lib.ptr(qt), probes.shape[1], lib.ptr(pt), a["k"],
                                        *(lib.ptr(v) for _, v in out))
    torch.cuda.synchronize()
    what = f"d={o['d']} M={o['M']} res={o['res']} k={k} mis={mis} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    got = band.cpu().numpy()
    assert (got[:pad] == 0x5A).all() and (got[pad + nbytes:] == 0x5A).all() and np.array_equal(got[pad:pad + nbytes], codes.reshape(-1)), what
    for w, v in out:
        (cr.assert_untouched if status else cr.assert_guards_intact)(w, v, what)
    if status:
        return None
    return out[0][1].view(torch.float32).cpu().numpy(), out[1][1].cpu().numpy(), out[2][1].cpu().numpy().view(np.uint32)


def want(o, xq, probes, k, codes=None, dtype=np.float32):
    dist = aq.distances(o["codes"] if codes is None else codes, o["codebooks"], xq, o["rowc"])
    return aq.model(o["offsets"], dist, probes, k, dtype)


@pytest.mark.parametrize("nq,d,M", [(1, 1, 1), (17, 7, 3), (33, 130, 2), (16, 128, 8)])
def test_lut(ctx, small, nq, d, M):
    """integer grids: float32 is exact, == the float64 products on both contexts.  Gaussian: the batch and every query alone give
    equal bits; an entry is a chain of at most d roundings (d / 4 MFMA steps, four products each), each relative 2^-24 of a partial
    sum that is at most sum |x_i c_i|, so the error is at most d 2^-24 sum |x_i c_i|"""
    rng = np.random.default_rng(d + M)
    cb, xq = rng.integers(-3, 4, size=(M, 256, d)).astype(np.float32), rng.integers(-3, 4, size=(nq, d)).astype(np.float32)
    exact = np.einsum("qi,mji->qmj", xq.astype(np.float64), cb.astype(np.float64))
    for c in (ctx, small):
        assert np.array_equal(lut(c, cb, xq).astype(np.float64), exact)
    cb, xq = rng.standard_normal(cb.shape).astype(np.float32), rng.standard_normal(xq.shape).astype(np.float32)
    got = lut(ctx, cb, xq)
    for q in range(nq):
        assert np.array_equal(lut(ctx, cb, xq[q:q + 1])[0].view(np.uint32), got[q].view(np.uint32)), f"query {q} alone"
    x64, c64 = xq.astype(np.float64), cb.astype(np.float64)
    err = np.abs(got - np.einsum("qi,mji->qmj", x64, c64))
    assert (err <= d * U * np.einsum("qi,mji->qmj", np.abs(x64), np.abs(c64))).all(), err.max()


@pytest.mark.parametrize("res", (False, True), ids=("raw", "residual"))
@pytest.mark.parametrize("d,M", aq.FORMS)
def test_scan_against_the_model(ctx, small, d, M, res):
    """EDGE_SIZES put trips at 63, 64 and 65 rows; code_size % 4 is 1, 0, 3, 1 over the forms; the one-CU context takes several items
    a slot, the default one cuts the 16-probe rows; both give the model's D, labels and stats"""
    o = aq.obj(d, M, res)
    for rows, nq in ROWS:
        xq = ir.queries(d, nq)
        for k in (1, 64):
            for c in (ctx, small):
                same(scan(c, o, xq, rows, k), want(o, xq, rows, k), f"{d} {M} res={res} k={k} cu={c.num_cu()}")


@pytest.mark.parametrize("case", ("shifted", "negative"))
def test_the_norm_field_is_read(ctx, case):
    """every stored norm + 1: every finite D moves by 1.  Norms of every third row at -1000: v < 0 there, D is +0.0 (the bits of
    +0, not of -0 or of a negative value) and those rows come first, in label order"""
    o, xq = aq.obj(16, 8, True), ir.queries(16, 12)
    idx, norm = aq.unpack(o["codes"], 8)
    norm = norm + 1 if case == "shifted" else np.where(np.arange(norm.size) % 3 == 0, np.float32(-1000), norm)
    codes = aq.pack(idx, norm)
    got, base = scan(ctx, o, xq, ir.EDGE_ROWS, 64, codes=codes), want(o, xq, ir.EDGE_ROWS, 64)
    same(got, want(o, xq, ir.EDGE_ROWS, 64, codes=codes), case)
    if case == "shifted":
        assert np.array_equal(got[0][np.isfinite(got[0])], base[0][np.isfinite(base[0])] + 1)
    else:
        zero = got[0].view(np.uint32) == 0
        assert zero[7].sum() >= 20 and (np.diff(got[1][7][zero[7]]) > 0).all() and zero[7][:zero[7].sum()].all()


@pytest.mark.parametrize("mis", (1, 2, 3))
def test_buffer_edges(ctx, mis):
    """7-byte rows 1, 2 and 3 bytes off a 16-byte boundary, 4403 bytes in all: the first and last chunk of the cooperative load
    straddle the array's ends.  Results are unchanged and the bands around the codes and outputs are intact"""
    xq = ir.queries(10, 12)
    for res in (False, True):
        o = aq.obj(10, 3, res)
        assert o["codes"].size == 4403
        same(scan(ctx, o, xq, ir.EDGE_ROWS, 64, mis=mis), want(o, xq, ir.EDGE_ROWS, 64), f"mis={mis}")


def test_chunking(ctx):
    """M = 64: a chunk is 1024 queries, so 1040 queries are two table launches and two scans; still the model's bytes"""
    o = aq.obj(4, 64, True, sizes=(70, 0, 65, 64, 63, 1, 33, 70))
    xq, rows = ir.queries(4, 1040), ir.probe_rows(1040, 2)
    same(scan(ctx, o, xq, rows, 3), want(o, xq, rows, 3), "1040 queries")


@pytest.mark.parametrize("over", [dict(M=0), dict(M=65), dict(k=0), dict(codes=None), dict(cb=None)], ids=str)
def test_refusals_on_a_live_context(ctx, over):
    o, xq = aq.obj(16, 8, True), ir.queries(16, 12)
    scan(ctx, o, xq, ir.EDGE_ROWS, 10, status=-1, over=over)
    assert b"ivf aq scan:" in _L().lib().vidc_last_error()
    same(scan(ctx, o, xq, ir.EDGE_ROWS, 10), want(o, xq, ir.EDGE_ROWS, 10), "the next good call")


@pytest.mark.parametrize("over", [dict(M=0), dict(M=65), dict(d=0), dict(cb=None), dict(xq=None), dict(lut=None)], ids=str)
def test_lut_refusals_on_a_live_context(ctx, over):
    cb, xq = (np.random.default_rng(2).integers(-3, 4, size=s).astype(np.float32) for s in ((2, 256, 7), (5, 7)))
    lut(ctx, cb, xq, status=-1, over=over)
    assert b"ivf aq lut:" in _L().lib().vidc_last_error()
    assert np.array_equal(lut(ctx, cb, xq).astype(np.float64), np.einsum("qi,mji->qmj", xq.astype(np.float64), cb.astype(np.float64)))


@pytest.mark.parametrize("container", ("array", "packed"))
@pytest.mark.parametrize("res", (False, True), ids=("raw", "residual"))
def test_through_the_index(res, container):
    """IVFIndex(16, 8, ("RQ", 4)): train on grid data, add, search_device.  After train the centroids and codebooks are rounded to
    the grid, so that torch's _scan, the model and the kernel compute the same exact integers."""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch = _t()
    rng = np.random.default_rng(77)
    x, xq = (rng.integers(-30, 31, size=(n, 16)).astype(np.float32) for n in (3000, 40))
    idx = IVFIndex(16, 8, ("RQ", 4), by_residual=res)
    idx.train_device = idx.pq_device = container == "packed"  # (the device's k-means and argmin; the array cases go through torch)
    idx.train(x)
    assert idx.pq.shape == (4, 256, 16) and idx.code_size == 8
    idx.centroids, idx.pq = idx.centroids.round(), idx.pq.round()
    idx.add(x)
    if container == "packed":
        idx.replace_invlists(ci.CompressedIDInvertedListsPackedBits(idx.invlists))
    idx.nprobe, k = 4, 5
    off, codes = idx._device_lists()
    codes_np, cb, cent = codes.cpu().numpy(), idx.pq.cpu().numpy(), idx.centroids.cpu().numpy()
    rowc = cent[np.repeat(np.arange(8), np.diff(off))] if res else None
    vecs = (aq.decode(codes_np, cb) + (rowc if res else 0)).astype(np.float32)
    assert codes_np.shape == (3000, 8) and np.array_equal(aq.unpack(codes_np, 4)[1], (vecs.astype(np.float64) ** 2).sum(1)), "the stored norms"
    probes = idx._probe_rows(torch.from_numpy(xq).cuda()).cpu().numpy()
    free = ir.tie_free(off, vecs, xq, probes, k)
    assert free.mean() >= 0.9, f"only {free.mean():.2f} of the queries are tie-free"
    D, labels = idx.scan_device(xq, k)
    same((D.cpu().numpy(), labels.cpu().numpy()), aq.model(off, aq.distances(codes_np, cb, xq, rowc), probes, k)[:2], "scan_device against the model")
    pD, pL = idx._scan(xq, k)
    assert np.array_equal(D.cpu().numpy(), pD) and np.array_equal(labels.cpu().numpy()[free], pL[free]), "against the torch _scan"
    sD, sI = idx.search_device(xq, k)
    rD, rI = idx.search(xq, k)
    assert np.array_equal(sD.cpu().numpy(), rD) and np.array_equal(sI.cpu().numpy()[free], rI[free])
    il = idx.invlists
    ids = il.get_ids_all().cpu().numpy().view(np.int64) if hasattr(il, "get_ids_all") else np.concatenate([il.get_ids(l) for l in range(8)])
    pick = np.arange(0, 3000, 37)
    got = idx.reconstruct_batch(torch.from_numpy(ids[pick].copy()).cuda() if hasattr(il, "locate_batch") else ids[pick]).cpu().numpy()
    assert np.array_equal(got, vecs[pick]), "reconstruct_batch"


def gaussian_case(seed=4):
    """d = 24, M = 6, residual, the edge lists: Gaussian codebooks, centroids and queries, the norm the float32 of the float64 |y|^2"""
    o = dict(aq.obj(24, 6, True))
    rng = np.random.default_rng(seed)
    o["codebooks"], o["centroids"] = (rng.standard_normal(o[n].shape).astype(np.float32) for n in ("codebooks", "centroids"))
    o["rowc"] = o["centroids"][np.repeat(np.arange(o["nlist"]), np.diff(o["offsets"].astype(np.int64)))]
    y = aq.decode(o["codes"], o["codebooks"]) + o["rowc"]
    o["codes"] = aq.pack(aq.unpack(o["codes"], 6)[0], (y ** 2).sum(1))
    xq, rows, k = rng.standard_normal((32, 24)).astype(np.float32), ir.probe_rows(32, 4), 10
    bound = (24 + 6 + 6) * U * aq.distances(o["codes"], o["codebooks"], xq, o["rowc"], magnitude=True)
    D64 = want(o, xq, rows, k + 1, dtype=np.float64)[0]
    with np.errstate(invalid="ignore"):  # (inf - inf behind the last candidate)
        gaps = np.where(np.isfinite(D64[:, 1:]), np.diff(D64, axis=1), np.inf).min(1)
    return o, xq, rows, k, bound, gaps > 2 * bound.max(1)


def test_gaussian_end_to_end(ctx):
    """D within (d + M + 6) 2^-24 (qn + |n| + 2 (sum |xq_i cent_i| + sum_m sum |xq_i cb_i|)) of the float64 value computed from the
    stored float32 norm.  The derivation, to first order in u = 2^-24: a table entry and cq are chains of at most d roundings over
    partial sums bounded by their sums of absolute products (d u of them); t adds M entries (M u of their absolute sum); ip = cq + t,
    qn + n and the fmaf are one rounding each and qn is a chain of at most d (together at most (d + 3) u of the absolute total, with
    the factor 2 of the fmaf inside it).  Every term is covered by (d + M + 6) u times the absolute total.  Labels are compared on
    queries whose float64 top-(k + 1) gaps exceed twice the largest bound of the query; the seed gives at least 0.9 of them."""
    o, xq, rows, k, bound, free = gaussian_case()
    assert free.mean() >= 0.9, f"only {free.mean():.2f} of the queries are gap-free"
    D, L, _ = scan(ctx, o, xq, rows, k)
    ref = aq.distances(o["codes"], o["codebooks"], xq, o["rowc"])
    pos = o["offsets"].astype(np.int64)[np.maximum(L, 0) >> 32] + (np.maximum(L, 0) & 0xFFFFFFFF)
    q = np.arange(len(xq))[:, None]
    ok = np.where(L >= 0, np.abs(D.astype(np.float64) - ref[q, pos]) <= bound[q, pos], np.isinf(D))
    assert ok.all(), f"{(~ok).sum()} distances outside the bound"
    assert np.array_equal(L[free], want(o, xq, rows, k, dtype=np.float64)[1][free])
