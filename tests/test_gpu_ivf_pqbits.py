"""Packed PQ codes of 1 .. 12 bits on the device (vidc_ivf_scan_pqbits_dev, vidc_ivf_pq_encode_bits_dev, IVFIndex(d, nlist,
("PQ", M, nbits))) against the numpy statements: tests/ivf_pqbits_ref.py for the layout, ivf_scan_ref.model for the scan, a float64
argmin written out here for the encoder.  Data are integer grids, so every float32 result is exact and compared with ==."""
import numpy as np
import pytest

import contract_ref as cr
import ivf_pqbits_ref as pb
import ivf_scan_ref as ir
from test_gpu_ivf_probe import _L, _t, ctx, shifted, small  # noqa: F401  (the probe's fixtures and its misaligned upload)

pytestmark = pytest.mark.gpu


def scan(ctx, o, xq, probes, k, res, mis=0, status=0, over=None):
    """vidc_ivf_scan_pqbits_dev over codes `mis` bytes off a 16-byte boundary between guard bands, into guarded outputs ->
    (D, labels, stats), or None for a refusal, which leaves the outputs untouched"""
    torch, lib = _t(), _L()
    xq, probes = np.ascontiguousarray(xq, np.float32), np.ascontiguousarray(probes, np.int64)
    nbytes, pad = o["codes"].size, 4096 + mis
    band = torch.full((pad + nbytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    band[pad:pad + nbytes].copy_(torch.from_numpy(o["codes"].reshape(-1).copy()))
    assert band[pad:].data_ptr() % 16 == mis
    off = torch.from_numpy(np.asarray(o["offsets"], np.uint64).view(np.int64).copy()).cuda()
    cb, cent = torch.from_numpy(o["codebooks"].copy()).cuda(), torch.from_numpy(o["centroids"].copy()).cuda()
    qt, pt = torch.from_numpy(xq.copy()).cuda(), torch.from_numpy(probes.copy()).cuda()
    out = [cr.guarded((len(xq), n), t, device="cuda") for n, t in ((k or 1, np.int32), (k or 1, np.int64), (2, np.int32))]
    a = dict(d=o["d"], M=o["M"], nbits=o["nbits"], codes=lib.ptr(band[pad:]), cb=lib.ptr(cb), k=k)
    a.update(over or {})
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_scan_pqbits_dev(ctx.h, o["nlist"], lib.ptr(off), o["ntotal"], a["codes"], a["d"], a["M"], a["nbits"], a["cb"],
                                            lib.ptr(cent) if res else None, len(xq), lib.ptr(qt), probes.shape[1], lib.ptr(pt), a["k"],
                                            *(lib.ptr(v) for _, v in out))
    torch.cuda.synchronize()
    what = f"d={o['d']} M={o['M']} nbits={o['nbits']} res={res} k={k} mis={mis} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    got = band.cpu().numpy()
    assert (got[:pad] == 0x5A).all() and (got[pad + nbytes:] == 0x5A).all() and np.array_equal(got[pad:pad + nbytes], o["codes"].reshape(-1)), what
    for w, v in out:
        (cr.assert_untouched if status else cr.assert_guards_intact)(w, v, what)
    if status:
        return None
    return out[0][1].view(torch.float32).cpu().numpy(), out[1][1].cpu().numpy(), out[2][1].cpu().numpy().view(np.uint32)


def same(got, want, what):
    for g, w, name in zip(got, want, ("D", "labels", "stats")):
        bad = np.argwhere(np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8))
        assert g.shape == w.shape and bad.size == 0, f"{what}: {name} differs ({bad.shape[0]} bytes, first at {bad[:1].tolist()})"


ROWS = ((ir.EDGE_ROWS, 12), (ir.probe_rows(3, 16), 3))  # 12 rows of 4 probes; 3 rows of 16: cut into pieces on the default context


@pytest.mark.parametrize("res", (False, True), ids=("raw", "residual"))
@pytest.mark.parametrize("d,M,nbits", pb.FORMS)
def test_scan_against_the_model(ctx, small, d, M, nbits, res):
    """EDGE_SIZES put trips at 63, 64 and 65 codes and spans whose ends are not 4-byte aligned wherever code_size % 4 != 0; the
    one-CU context takes several items a slot, the default one cuts the 16-probe rows; both give the model's D, labels and stats"""
    o = pb.obj(d, M, nbits)
    for rows, nq in ROWS:
        xq = ir.queries(d, nq)
        for k in (1, 64):
            want = ir.model(o["offsets"], o["rvecs" if res else "vecs"], xq, rows, k)
            for c in (ctx, small):
                same(scan(c, o, xq, rows, k, res), want, f"{d} {M} {nbits} res={res} k={k} cu={c.num_cu()}")


@pytest.mark.parametrize("grid", (True, False), ids=("grid", "gaussian"))
def test_eight_bits_equal_the_8_bit_calls(ctx, grid):
    """the arithmetic is stated to be the PQ8 kernels': equal bits on the grid and on Gaussian data"""
    torch, lib = _t(), _L()
    o = dict(pb.obj(16, 4, 8))
    if not grid:
        rng = np.random.default_rng(8)
        o["codebooks"], o["centroids"] = (rng.standard_normal(o[n].shape).astype(np.float32) for n in ("codebooks", "centroids"))
    rows = ir.probe_rows(9, 16)
    xq = ir.queries(16, 9) if grid else np.random.default_rng(9).standard_normal((9, 16)).astype(np.float32)
    t = {n: torch.from_numpy(np.ascontiguousarray(v)).cuda() for n, v in (("off", np.asarray(o["offsets"]).view(np.int64)), ("codes", o["codes"]),
         ("cb", o["codebooks"]), ("cent", o["centroids"]), ("xq", xq), ("rows", rows))}
    for res in (False, True):
        D, L = torch.empty((9, 20), dtype=torch.float32, device="cuda"), torch.empty((9, 20), dtype=torch.int64, device="cuda")
        head = (ctx.h, o["nlist"], lib.ptr(t["off"]), o["ntotal"], lib.ptr(t["codes"]))
        tail = (9, lib.ptr(t["xq"]), 16, lib.ptr(t["rows"]), 20, lib.ptr(D), lib.ptr(L), None)
        if res:
            st = lib.lib().vidc_ivf_scan_residual_dev(*head, 16, 4, lib.ptr(t["cb"]), lib.ptr(t["cent"]), *tail)
        else:
            st = lib.lib().vidc_ivf_scan_dev(*head, lib.VIDC_IVF_PQ8, 16, 4, lib.ptr(t["cb"]), *tail)
        torch.cuda.synchronize()
        assert st == 0, lib.lib().vidc_last_error()
        same(scan(ctx, o, xq, rows, 20, res)[:2], (D.cpu().numpy(), L.cpu().numpy()), f"grid={grid} res={res}")


@pytest.mark.parametrize("mis", (1, 2, 3))
def test_buffer_edges(ctx, mis):
    """PQ8x10 codes 1, 2 and 3 bytes off a 16-byte boundary, 6290 bytes in all (no multiple of 4): the first and last chunk of the
    cooperative load straddle the array's ends.  Results are unchanged and the bands around the codes and outputs are intact.  A read
    outside the array would show here only through a wrong result: that the kernel reads nothing outside is argued in its source."""
    o, xq = pb.obj(16, 8, 10), ir.queries(16, 12)
    assert o["codes"].size % 4 == 2
    for res in (False, True):
        same(scan(ctx, o, xq, ir.EDGE_ROWS, 64, res, mis=mis), ir.model(o["offsets"], o["rvecs" if res else "vecs"], xq, ir.EDGE_ROWS, 64), f"mis={mis}")


NLIST = 7  # (the encoder)


def grid_batch(n, d, M, nbits, seed=0, R=2):
    assert d // M * (3 * R) ** 2 < 2 ** 24
    rng = np.random.default_rng(1000 * seed + n + d + M + nbits)
    x, c = (rng.integers(-R, R + 1, size=s).astype(np.float32) for s in ((n, d), (NLIST, d)))
    pq = rng.integers(-R, R + 1, size=(M, 1 << nbits, d // M)).astype(np.float32)
    assign = rng.integers(0, NLIST, n)
    if n > 1:
        assign[0], assign[n // 2] = -1, NLIST
    return x, pq, c, assign


def ref_fields(x, pq, c=None, assign=None):
    """the float64 argmin, first index on ties; rows with an assign outside [0, nlist) are zeros"""
    r = x if c is None else (x - c[np.clip(assign, 0, len(c) - 1)]).astype(np.float32)
    M, _, dsub = pq.shape
    f = np.stack([((r[:, m * dsub:(m + 1) * dsub].astype(np.float64)[:, None] - pq[m].astype(np.float64)[None]) ** 2).sum(-1).argmin(1)
                  for m in range(M)], 1)
    if c is not None:
        f[(assign < 0) | (assign >= len(c))] = 0
    return f


def encode(ctx, x, pq, nbits, c=None, assign=None, status=0, over=None):
    """vidc_ivf_pq_encode_bits_dev into a guarded buffer -> uint8 [n, code_size]; bytes behind n * code_size stay as they were"""
    torch, lib = _t(), _L()
    n, (M, _, dsub) = len(x), pq.shape
    cs = (M * nbits + 7) // 8
    xt, pt = shifted(x, 0), shifted(pq, 0)
    ct = shifted(c, 0) if c is not None else None
    at = torch.from_numpy(np.asarray(assign, np.int64)).cuda() if c is not None else None
    wC, vC = cr.guarded((-(-n * cs // 4),), np.int32, device="cuda")
    before = vC.clone()
    a = dict(x=lib.ptr(xt), d=M * dsub, M=M, nbits=nbits)
    a.update(over or {})
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_pq_encode_bits_dev(ctx.h, n, a["x"], a["d"], a["M"], a["nbits"], lib.ptr(pt), len(c) if c is not None else 0,
                                               lib.ptr(ct), lib.ptr(at), lib.ptr(vC))
    torch.cuda.synchronize()
    what = f"n={n} d={M * dsub} M={M} nbits={nbits} residual={c is not None} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    if status:
        cr.assert_untouched(wC, vC, what)
        return None
    cr.assert_guards_intact(wC, vC, what)
    got, was = vC.view(torch.uint8).cpu().numpy(), before.view(torch.uint8).cpu().numpy()
    assert np.array_equal(got[n * cs:], was[n * cs:]), f"{what}: bytes behind the codes changed"
    return got[:n * cs].reshape(n, cs)


@pytest.mark.parametrize("n,d,M,nbits", [(1, 10, 1, 10), (100, 16, 8, 10), (100, 32, 2, 10), (257, 12, 3, 10), (65, 10, 5, 5), (33, 64, 16, 4), (300, 34, 2, 12), (17, 7, 7, 1)])
def test_encoder_against_the_float64_argmin(ctx, small, n, d, M, nbits):
    """raw and residual; held (dsub <= 10) and streamed codebooks (dsub = 17 at 12 bits; dsub = 16 at 10 bits: the 16-byte loads,
    PQ8x10's form at d = 128), ksub < 16 (padded column blocks), ragged vector tiles; pack leaves pad bits zero; both contexts agree"""
    x, pq, c, assign = grid_batch(n, d, M, nbits)
    for args in ((), (c, assign)):
        want = pb.pack(ref_fields(x, pq, *args), nbits)
        got = encode(ctx, x, pq, nbits, *args)
        assert np.array_equal(got, want), f"codes differ at {np.argwhere(got != want)[:4].tolist()}"
        assert np.array_equal(encode(small, x, pq, nbits, *args), got)


def test_every_codeword_can_win_and_ties_go_down(ctx):
    """x is the 1024 codebook rows (dsub = 16: the streamed form).  Planted copies across a 128-codeword tile seam (127, 128), across
    the whole range (0, 1023) and inside a lane group (37, 38): the field of the copy is the index of the original"""
    _, pq, _, _ = grid_batch(1, 32, 2, 10, seed=1)
    pairs = [(127, 128), (0, 1023), (37, 38)]
    for a, b in pairs:
        pq[:, b] = pq[:, a]
    x = np.ascontiguousarray(np.concatenate(list(pq), 1))
    want = ref_fields(x, pq)
    assert all((want[b] == a).all() for a, b in pairs) and len(np.unique(want)) >= 1000
    assert np.array_equal(pb.unpack(encode(ctx, x, pq, 10), 2, 10), want)


def test_encoder_eight_bits_equal_the_8_bit_call(ctx):
    from vector_db_id_compression_amd import ivf_encode

    x, pq, c, assign = grid_batch(100, 16, 4, 8)
    for args in ((), (c, assign)):
        assert np.array_equal(encode(ctx, x, pq, 8, *args), ivf_encode.pq_encode_device(x, pq, *args).cpu().numpy())


@pytest.mark.parametrize("over", [dict(nbits=0), dict(nbits=13), dict(M=5), dict(codes=None), dict(cb=None), dict(d=128, M=64, nbits=10)], ids=str)
def test_scan_refusals_on_a_live_context(ctx, over):
    o, xq = pb.obj(16, 8, 10), ir.queries(16, 12)
    scan(ctx, o, xq, ir.EDGE_ROWS, 10, True, status=-1, over=over)
    assert b"ivf pqbits scan:" in _L().lib().vidc_last_error()
    same(scan(ctx, o, xq, ir.EDGE_ROWS, 10, True), ir.model(o["offsets"], o["rvecs"], xq, ir.EDGE_ROWS, 10), "the next good call")


@pytest.mark.parametrize("over", [dict(nbits=0), dict(nbits=13), dict(M=3), dict(x=None)], ids=str)
def test_encoder_refusals_on_a_live_context(ctx, over):
    x, pq, c, assign = grid_batch(33, 16, 8, 10)
    encode(ctx, x, pq, 10, c, assign, status=-1, over=over)
    assert np.array_equal(encode(ctx, x, pq, 10, c, assign), pb.pack(ref_fields(x, pq, c, assign), 10))


@pytest.mark.parametrize("container", ("array", "packed"))
@pytest.mark.parametrize("res", (False, True), ids=("raw", "residual"))
def test_through_the_index(res, container):
    """IVFIndex(16, 8, ("PQ", 8, 10)): train on grid data (1024 codewords a sub-quantiser), add, search_device.  After train the
    centroids and codebooks are rounded to the grid, so that torch's _scan, the model and the kernel compute the same exact integers."""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    torch = _t()
    rng = np.random.default_rng(77)
    x, xq = (rng.integers(-30, 31, size=(n, 16)).astype(np.float32) for n in (3000, 40))
    idx = IVFIndex(16, 8, ("PQ", 8, 10), by_residual=res)
    idx.train_device = container == "packed"  # (pq_train_device with ksub = 1024; the array cases train through torch)
    idx.train(x)
    assert idx.pq.shape == (8, 1024, 2) and idx.code_size == 10
    idx.centroids, idx.pq = idx.centroids.round(), idx.pq.round()
    idx.add(x)
    if container == "packed":
        idx.replace_invlists(ci.CompressedIDInvertedListsPackedBits(idx.invlists))
    idx.nprobe, k = 4, 5
    off, codes = idx._device_lists()
    codes_np, cb, cent = codes.cpu().numpy(), idx.pq.cpu().numpy(), idx.centroids.cpu().numpy()
    assert codes_np.shape == (3000, 10)
    vecs = pb.decode(codes_np, cb, 10)
    if res:
        vecs = vecs + cent[np.repeat(np.arange(8), np.diff(off))]
    probes = idx._probe_rows(torch.from_numpy(xq).cuda()).cpu().numpy()
    free = ir.tie_free(off, vecs, xq, probes, k)
    assert free.mean() >= 0.9, f"only {free.mean():.2f} of the queries are tie-free"
    want = ir.model(off, vecs, xq, probes, k)
    D, labels = idx.scan_device(xq, k)
    same((D.cpu().numpy(), labels.cpu().numpy()), want[:2], "scan_device against the model")
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
