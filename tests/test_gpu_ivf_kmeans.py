"""One Lloyd iteration on the device (vidc_ivf_kmeans_step_dev, ivf_train) against the numpy model of tests/ivf_kmeans_ref.py.
Integer-grid inputs make every float32 score and every sum exact, so assign, counts and c_out are compared with ==.  Every call goes
through the C-ABI into guarded outputs with the d2h counter held."""
import numpy as np
import pytest

import contract_ref as cr
import ivf_kmeans_ref as km
from test_gpu_ivf_probe import _L, _t, ctx, shifted, small  # noqa: F401  (the probe's fixtures and its misaligned upload)

pytestmark = pytest.mark.gpu

INVALID = -1


def call(ctx, x, c, status=0, mis=0, over=None):
    """vidc_ivf_kmeans_step_dev into guarded outputs -> (c_out, assign, counts), or None; a refusal leaves all three untouched"""
    torch, lib = _t(), _L()
    n, ld = x.shape
    G, k, dsub = c.shape
    xt, ct = shifted(x, mis), shifted(c, mis)
    outs = [cr.guarded((max(sz, 1),), np.int32, device="cuda") for sz in (G * k * dsub, G * n, G * k)]
    a = dict(ctx=ctx.h, n=n, x=lib.ptr(xt), ld=ld, G=G, dsub=dsub, k=k, c_in=lib.ptr(ct), c_out=lib.ptr(outs[0][1]),
             assign=lib.ptr(outs[1][1]), counts=lib.ptr(outs[2][1]))
    a.update(over or {})
    if a["c_out"] == "alias":
        a["c_out"] = a["c_in"]
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d2h = ctx.d2h_bytes()
    torch.cuda.synchronize()
    st = lib.lib().vidc_ivf_kmeans_step_dev(a["ctx"], a["n"], a["x"], a["ld"], a["G"], a["dsub"], a["k"], a["c_in"], a["c_out"], a["assign"],
                                            a["counts"])
    torch.cuda.synchronize()
    what = f"n={n} ld={ld} G={G} dsub={dsub} k={k} mis={mis} {over}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    assert ctx.d2h_bytes() == d2h, f"{what}: the d2h counter moved"
    assert np.array_equal(xt.cpu().numpy(), x) and np.array_equal(ct.cpu().numpy(), c), f"{what}: the inputs changed"
    if status:
        for w, v in outs:
            cr.assert_untouched(w, v, what)
        return None
    for w, v in outs:
        cr.assert_guards_intact(w, v, what)
    c_out = outs[0][1].cpu().numpy().view(np.float32)[:G * k * dsub].reshape(G, k, dsub)
    if n == 0:
        cr.assert_untouched(*outs[1], what)
    return c_out, outs[1][1].cpu().numpy()[:G * n].reshape(G, n), outs[2][1].cpu().numpy().view(np.uint32)[:G * k].reshape(G, k)


def grid(n, G, dsub, ld, k, R=2, seed=0):
    """integer-grid points and centroids: every partial sum of a score and of a cluster sum is an integer below 2^24"""
    assert dsub * (3 * R) ** 2 < 2 ** 24 and n * R < 2 ** 24 and ld >= G * dsub
    rng = np.random.default_rng(1000 * seed + n + G + dsub + ld + k)
    return rng.integers(-R, R + 1, size=(n, ld)).astype(np.float32), rng.integers(-R, R + 1, size=(G, k, dsub)).astype(np.float32)


def assert_exact(got, x, c, what=""):
    want = km.step(x, c)
    for name, g, w in zip(("c_out", "counts", "assign"), (got[0], got[2], got[1]), want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"{what} {name} differs at {np.argwhere(g != w)[:4].tolist()}"
    return want


# (n, G, dsub, ld, k): k on both sides of an MFMA column block and of a 128-centroid tile, dsub on both sides of the padding to 4 and of
# the 32-component chunk, n on both sides of the 128-point block; G = 3 with ld > G * dsub: unused trailing columns, unaligned column
# bases.  Streamed centroids: (700, 1, 128, 128, 257), (129, 1, 33, 33, 600) (4-byte loads) and (700, 3, 128, 388, 257); held whole: the rest
SHAPES = [(1, 1, 1, 1, 1), (127, 1, 3, 3, 15), (129, 1, 8, 8, 17), (700, 1, 33, 33, 256), (700, 1, 128, 128, 257), (129, 3, 3, 11, 17),
          (700, 3, 8, 28, 256), (127, 3, 33, 100, 257), (129, 3, 128, 385, 15), (129, 1, 33, 33, 600), (700, 3, 128, 388, 257), (129, 1, 1, 2, 257)]


@pytest.mark.parametrize("n,G,dsub,ld,k", SHAPES)
def test_integer_grids_exact(ctx, n, G, dsub, ld, k):
    x, c = grid(n, G, dsub, ld, k)
    assert_exact(call(ctx, x, c), x, c)


@pytest.mark.parametrize("every", (False, True), ids=("sizes", "one-holds-all"))
def test_designed_clusters(ctx, small, every):
    """centroid j sits at 100 j on the first axis.  sizes: clusters of 0, 1, 256, 257 and 513 members, centroid 5 a copy of centroid 2
    (the smaller index wins, the twin stays empty and keeps c_in), centroid 6 far from every point.  one-holds-all: every point at
    centroid 1"""
    sizes = [0, 1027, 0] if every else [0, 1, 256, 257, 513, 0, 0]
    rng = np.random.default_rng(7)
    c = np.zeros((1, len(sizes), 4), np.float32)
    c[0, :, 0] = 100 * np.arange(len(sizes))
    c[0, :, 1:] = rng.integers(-2, 3, size=(len(sizes), 3))
    if not every:
        c[0, 5] = c[0, 2]
    x = np.concatenate([c[0, j] + rng.integers(-2, 3, size=(m, 4)) for j, m in enumerate(sizes)]).astype(np.float32)
    x = x[rng.permutation(len(x))]
    got = call(ctx, x, c)
    want = assert_exact(got, x, c)
    assert want[1][0].tolist() == sizes and np.array_equal(got[0][0][np.array(sizes) == 0], c[0][np.array(sizes) == 0])
    for a, b in zip(got, call(small, x, c)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n,G,dsub,ld,k", [(700, 2, 24, 52, 40), (700, 1, 128, 128, 2), (300, 1, 128, 128, 300), (700, 3, 5, 17, 256)])
def test_float_data(ctx, small, n, G, dsub, ld, k):
    """Gaussian data: the assignment within the header's bound of the float64 minimum; counts the bincount of the device's own
    assign; c_out within count 2^-24 sum |x_i| of the float64 mean of the device's own members and bit-equal to the chunk model on
    the device's assign; all three bit-equal on a one-CU context"""
    rng = np.random.default_rng(n + k)
    x, c = rng.standard_normal((n, ld)).astype(np.float32), rng.standard_normal((G, k, dsub)).astype(np.float32)
    c_out, a, counts = got = call(ctx, x, c)
    assert ((a >= 0) & (a < k)).all()
    dist = km.distances(x, c)
    nrm = lambda v: np.sqrt((v.astype(np.float64) ** 2).sum(-1))
    for g in range(G):
        xg = x[:, g * dsub:(g + 1) * dsub]
        bound = 2 * (dsub + 4) * 2.0 ** -24 * (nrm(xg) + nrm(c[g]).max()) ** 2
        excess = np.take_along_axis(dist[g], a[g][:, None].astype(np.int64), 1)[:, 0] - dist[g].min(1)
        print("largest excess / bound:", float((excess / bound).max()), "off the float64 argmin:", int((excess > 0).sum()))
        assert (excess <= bound).all()
        assert np.array_equal(counts[g], np.bincount(a[g], minlength=k))
        for j in np.flatnonzero(counts[g]):
            rows = xg[a[g] == j].astype(np.float64)
            assert (np.abs(c_out[g, j] - rows.mean(0)) <= len(rows) * 2.0 ** -24 * np.abs(rows).sum(0)).all()
    model = km.update(x, c, a)
    assert np.array_equal(c_out.view(np.uint32), model[0].view(np.uint32)) and np.array_equal(counts, model[1])
    for u, v in zip(got, call(small, x, c)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_kmeans_device_follows_the_model_step_by_step():
    """three iterations on integer-grid points, each step fed the device's previous output"""
    from vector_db_id_compression_amd import ivf_train

    x, _ = grid(300, 1, 16, 16, 10, R=8, seed=3)
    c = ivf_train._initial_rows(_t().from_numpy(x).cuda(), 10, 123)
    for _ in range(3):
        dev = ivf_train.kmeans_step_device(x, c)
        want = km.step(x, c.cpu().numpy()[None])
        assert np.array_equal(dev[1].cpu().numpy(), want[2][0]) and np.array_equal(dev[2].cpu().numpy(), want[1][0].astype(np.int32))
        assert np.array_equal(dev[0].cpu().numpy(), want[0][0])
        c = dev[0]
    assert np.array_equal(ivf_train.kmeans_device(x, 10, iters=3).cpu().numpy(), c.cpu().numpy())


def test_index_trains_on_the_device():
    from vector_db_id_compression_amd import ivf_train
    from vector_db_id_compression_amd.ivf import IVFIndex, _assign

    torch = _t()
    x = np.random.default_rng(11).standard_normal((600, 16)).astype(np.float32)
    idx = IVFIndex(16, 8, ("PQ", 4), by_residual=True)
    idx.train_device = True
    idx.train(x)
    xt = torch.from_numpy(x).cuda()
    cent = ivf_train.kmeans_device(xt, 8)
    assert torch.equal(idx.centroids, cent) and torch.equal(idx.pq, ivf_train.pq_train_device(xt - cent[_assign(xt, cent)], 4))
    assert idx.pq.shape == (4, 256, 4)
    idx.add(x)
    idx.nprobe = 8
    D, I = idx.search_device(x[:5], 3)
    assert I.shape == (5, 3) and (I[:, 0].cpu().numpy() >= 0).all() and bool(torch.isfinite(D[:, 0]).all())


@pytest.mark.parametrize("over", [dict(ctx=None), dict(x=None), dict(c_in=None), dict(c_out=None), dict(G=0), dict(k=0), dict(dsub=0),
                                  dict(dsub=2049), dict(ld=7), dict(G=1, k=2 ** 24 + 1), dict(n=2 ** 32), dict(c_out="alias")], ids=str)
def test_refusals_on_a_live_context(ctx, over):
    x, c = grid(5, 2, 4, 8, 3, seed=4)
    call(ctx, x, c, status=INVALID, over=over)
    assert b"ivf kmeans step" in _L().lib().vidc_last_error()
    c_out, _, counts = call(ctx, x[:0], c)  # n == 0: c_out = c_in, the counts zero
    assert np.array_equal(c_out, c) and not counts.any()
    assert_exact(call(ctx, x, c), x, c)
