"""The wide IVF scans on the device (vidc_ivf_scan_wide_dev, vidc_ivf_scan_aq_wide_dev, IVFIndex.scan_device with k > 256) against the
float64 statements tests/ivf_scan_ref.py and tests/ivf_aq_ref.py.  Data are integer grids: float32 distances are exact and D, labels
and stats are compared with ==.  Every call writes into guarded, poisoned outputs and reads codes between guard bands, 3 bytes (FLAT: 4) off a
16-byte boundary unless said otherwise.  A reference is computed once, at k = 2048: the result for a smaller k is its prefix."""
import functools

import numpy as np
import pytest

import contract_ref as cr
import ivf_aq_ref as aq
import ivf_scan_ref as ir
from test_gpu_ivf_probe import _L, _t, ctx, small  # noqa: F401  (the default context and the one-CU context)
from test_gpu_ivf_pqbits import same

pytestmark = pytest.mark.gpu

KINDS = ("flat", "pq8", "rq", "rq_res")
SIZES = (0, 1, 255, 256, 257, 64, 1500, 3000)  # the round edges, and lists of several flushes
# a duplicate, a -1, an invalid list; row 2 names 320 candidates (fewer than every k here: padding), row 3 none
ROWS = np.array([[7, 6, 3, 4], [6, 6, 7, -1], [1, 2, -1, 5], [0, -1, 8, 0], [3, 4, 2, 1], [7, 7, 7, 7]], dtype=np.int64)


def obj(kind, R=3):
    """d = 8: Flat, PQ4 or RQ3 (7-byte rows)"""
    return aq.obj(8, 3, kind == "rq_res", sizes=SIZES, R=R) if kind.startswith("rq") else ir.obj(8, 4 if kind == "pq8" else 0, sizes=SIZES, R=R)


@functools.lru_cache(maxsize=None)
def designed(kind, R=3):
    """-> the object, six queries, and the model's (D, labels, stats) for ROWS at k = 2048"""
    o = obj(kind, R)
    xq = ir.queries(8, len(ROWS), R=R)
    if kind.startswith("rq"):
        return o, xq, aq.model(o["offsets"], aq.distances(o["codes"], o["codebooks"], xq, o["rowc"]), ROWS, 2048)
    return o, xq, ir.model(o["offsets"], o["vecs"], xq, ROWS, 2048)


prefix = lambda want, k, idx=slice(None): (want[0][idx, :k], want[1][idx, :k], want[2][idx])  # noqa: E731


def scan(c, kind, o, xq, rows, k, wide=True, mis=3):
    """the wide (or the narrow) C call of the kind -> (D, labels, stats) numpy; the bands around the codes and the outputs are checked"""
    torch, lib = _t(), _L()
    xq, rows = np.ascontiguousarray(xq, np.float32), np.ascontiguousarray(rows, np.int64)
    mis = 4 * bool(mis) if kind == "flat" else mis  # (float32 loads stay 4-byte aligned)
    nbytes, pad = o["codes"].size, 4096 + mis
    band = torch.full((pad + nbytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    band[pad:pad + nbytes].copy_(torch.from_numpy(o["codes"].reshape(-1).copy()))
    assert band[pad:].data_ptr() % 16 == mis
    off = torch.from_numpy(np.asarray(o["offsets"], np.uint64).view(np.int64).copy()).cuda()
    cb = torch.from_numpy(o["codebooks"].copy()).cuda() if o["codebooks"] is not None else None
    qt, pt = torch.from_numpy(xq.copy()).cuda(), torch.from_numpy(rows.copy()).cuda()
    out = [cr.guarded((len(xq), n), t, device="cuda") for n, t in ((k, np.int32), (k, np.int64), (2, np.int32))]
    head = (c.h, o["nlist"], lib.ptr(off), o["ntotal"], lib.ptr(band[pad:]))
    tail = (len(xq), lib.ptr(qt), rows.shape[1], lib.ptr(pt), k, *(lib.ptr(v) for _, v in out))
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if kind.startswith("rq"):
        cent = torch.from_numpy(o["centroids"].copy()).cuda() if o["res"] else None
        fn = lib.lib().vidc_ivf_scan_aq_wide_dev if wide else lib.lib().vidc_ivf_scan_aq_dev
        st = fn(*head, o["d"], o["M"], lib.ptr(cb), lib.ptr(cent) if o["res"] else None, *tail)
    else:
        fn = lib.lib().vidc_ivf_scan_wide_dev if wide else lib.lib().vidc_ivf_scan_dev
        st = fn(*head, o["kind"], o["d"], o["M"], lib.ptr(cb) if o["M"] else None, *tail)
    torch.cuda.synchronize()
    what = f"{kind} k={k} wide={wide} mis={mis} cu={c.num_cu()}"
    assert st == 0, (what, st, lib.lib().vidc_last_error())
    got = band.cpu().numpy()
    assert (got[:pad] == 0x5A).all() and (got[pad + nbytes:] == 0x5A).all() and np.array_equal(got[pad:pad + nbytes], o["codes"].reshape(-1)), what
    for w, v in out:
        cr.assert_guards_intact(w, v, what)
    return out[0][1].view(torch.float32).cpu().numpy(), out[1][1].cpu().numpy(), out[2][1].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("k", (257, 512, 513, 1000, 2048))
@pytest.mark.parametrize("kind", KINDS)
def test_model_cases(ctx, kind, k):
    """six queries of four probes on the default context: the rows are cut (S = 4) and k_ivf_merge_wide runs"""
    o, xq, want = designed(kind)
    assert np.isinf(want[0][2, 320:]).all() and (want[1][2, 320:] == -1).all() and np.isfinite(want[0][2, :320]).all()
    same(scan(ctx, kind, o, xq, ROWS, k), prefix(want, k), f"{kind} k={k}")


def one_list(kind, order):
    """one list of 3000 entries whose distances from the origin are 1 .. 3000, stored ascending or descending"""
    r = np.arange(1, 3001, dtype=np.float32) if order == "ascending" else np.arange(3000, 0, -1, dtype=np.float32)
    off = np.array([0, 3000], np.uint64)
    if kind == "flat":  # d = 1: the distance is r^2 < 2^24
        vecs = r[:, None].copy()
        return dict(offsets=off, ntotal=3000, nlist=1, codes=vecs.view(np.uint8).reshape(3000, 4).copy(), vecs=vecs, codebooks=None, d=1, M=0,
                    kind=ir.FLAT), None
    cb = np.zeros((1, 256, 1), np.float32)  # every inner product is 0: the distance is the stored norm
    return dict(offsets=off, ntotal=3000, nlist=1, codes=aq.pack(np.zeros((3000, 1), np.int64), r), codebooks=cb, centroids=np.zeros((1, 1), np.float32),
                rowc=None, d=1, M=1, res=False), r


@pytest.mark.parametrize("order", ("descending", "ascending"))
@pytest.mark.parametrize("kind", ("flat", "rq"))
def test_worst_and_best_filter_cases(ctx, kind, order):
    """queries at the origin.  Descending: every candidate is below the threshold it meets, the buffer flushes as often as it can.
    Ascending: behind the first flush nothing survives.  nprobe = 1: no cut"""
    o, r = one_list(kind, order)
    xq, rows = np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int64)
    dist = np.sort(r if kind == "rq" else o["vecs"][:, 0] ** 2)
    for k in (257, 1000):
        D, L, st = scan(ctx, kind, o, xq, rows, k)
        pos = np.arange(k) if order == "ascending" else 2999 - np.arange(k)
        assert np.array_equal(D, np.tile(dist[:k], (2, 1))) and np.array_equal(L, np.tile(pos, (2, 1))) and (st == [1, 3000]).all(), (kind, order, k)


@pytest.mark.parametrize("kind", KINDS)
def test_ties(ctx, kind):
    """R = 1: fewer than 256 distinct distances over 5333 candidates, thousands of equal ones: labels decide"""
    o, xq, want = designed(kind, 1)
    assert max(np.unique(row[np.isfinite(row)]).size for row in want[0]) < 256
    for k in (257, 1000):
        same(scan(ctx, kind, o, xq, ROWS, k), prefix(want, k), f"{kind} ties k={k}")


def gaussian(kind):
    """the designed object with Gaussian vectors, codebooks, centroids and norms: no model, only wide == narrow"""
    o, rng = dict(obj(kind)), np.random.default_rng(6)
    if kind == "flat":
        o["codes"] = rng.standard_normal((o["ntotal"], 8)).astype(np.float32).view(np.uint8).reshape(o["ntotal"], 32)
    else:
        o["codebooks"] = rng.standard_normal(o["codebooks"].shape).astype(np.float32)
    if kind.startswith("rq"):
        o["centroids"] = rng.standard_normal(o["centroids"].shape).astype(np.float32)
        o["codes"] = aq.pack(aq.unpack(o["codes"], 3)[0], rng.standard_normal(o["ntotal"]) ** 2 + 20)
    return o, rng.standard_normal((len(ROWS), 8)).astype(np.float32)


@pytest.mark.parametrize("data", ("grid", "gaussian"))
@pytest.mark.parametrize("kind", KINDS)
def test_same_bytes_as_the_narrow_call(ctx, kind, data):
    """both kernels take their distances from the same per-trip code, so this is ==, on float data too.  mis = 0 and 3: the 16-byte
    and the narrow loads of FLAT and PQ8"""
    o, xq = gaussian(kind) if data == "gaussian" else designed(kind)[:2]
    for k, mis in ((1, 3), (20, 0), (256, 3)):
        same(scan(ctx, kind, o, xq, ROWS, k, mis=mis), scan(ctx, kind, o, xq, ROWS, k, wide=False, mis=mis), f"{kind} {data} k={k}")


@pytest.mark.parametrize("kind", KINDS)
def test_the_cut_on_a_one_cu_context(small, kind):
    """one compute unit holds at most eight workgroups: 6 queries are cut (S = 2), 27 are not and every workgroup takes several items;
    the runs come from poisoned scratch.  (The default context cuts the same rows into 4: test_model_cases)"""
    o, xq, want = designed(kind)
    for nq in (6, 27):
        idx = (np.arange(nq) * 5) % len(ROWS)
        for k in (257, 1000):
            same(scan(small, kind, o, xq[idx], ROWS[idx], k), prefix(want, k, idx), f"{kind} one CU nq={nq} k={k}")


@pytest.mark.parametrize("code,res", (("Flat", False), (("RQ", 4), True)), ids=("flat", "rq_res"))
def test_a_short_list_of_1000_through_the_index(code, res):
    """train, add, a packed container, search_device(xq, 1000) against search (the torch _scan and the ids of every probed list on
    the host).  D is equal everywhere.  torch.topk orders equal distances in its own way, so the (distance, id) pairs are compared
    as sets strictly below the query's 1000th distance, where every tie-break keeps the same set"""
    from vector_db_id_compression_amd import custom_invlists as ci
    from vector_db_id_compression_amd.ivf import IVFIndex

    rng = np.random.default_rng(78)
    x, xq = (rng.integers(-30, 31, size=(n, 16)).astype(np.float32) for n in (3000, 12))
    idx = IVFIndex(16, 8, code, by_residual=res)
    idx.train(x)
    idx.centroids = idx.centroids.round()
    if res:
        idx.pq = idx.pq.round()
    idx.add(x)
    idx.replace_invlists(ci.CompressedIDInvertedListsPackedBits(idx.invlists))
    idx.nprobe, k = 6, 1000
    D, I = (t.cpu().numpy() for t in idx.search_device(xq, k))
    rD, rI = idx.search(xq, k)
    assert D.shape == (12, k) and np.array_equal(D, rD) and np.isfinite(D).all(), "fewer than 1000 candidates, or D differs"
    for q in range(12):
        below = D[q] < D[q, -1]
        assert below.sum() > k // 2 and sorted(zip(D[q][below], I[q][below])) == sorted(zip(rD[q][below], rI[q][below])), q
