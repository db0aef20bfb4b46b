"""The best-first graph search as one launch (vidc_{rows,compact,ef}_search_dev, graph_search.search_device) against the numpy model
(tests/graph_search_ref.py).  Data are integer grids, so D, I and stats are compared element for element, ties included.  Calls that go
through the C-ABI directly write into guarded, poisoned buffers; the d2h counter does not move; the objects' exported images are the
same before and after.  Shapes, hostile rows and the one-CU batch are the ones the CPU tests hold to their purpose."""
import ctypes as C

import numpy as np
import pytest

import contract_ref as cr
import graph_search_ref as gr
from test_graph_search_ref_cpu import ONE_CU_NQ

pytestmark = pytest.mark.gpu

KINDS = ("raw", "compact", "ef")
INVALID, UNSUPPORTED = -1, -6


def _t():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


def _gs():
    from vector_db_id_compression_amd import graph_search

    return graph_search


def build(kind, rows, ctx=None):
    """-> what vidc_*_search_dev takes for `rows`: (kind, holder); raw: an int32 CUDA tensor, else the codec object"""
    from vector_db_id_compression_amd import codecs

    torch = _t()
    rows = np.array(rows, dtype=np.int32, order="C")  # (a writable copy: the shapes are shared and read-only)
    if kind == "raw":
        return torch.from_numpy(rows).cuda()
    if kind == "compact":
        return codecs.CompactRows.encode_rows(rows, ctx=ctx)
    return codecs.EfLists.encode_rows(rows, ctx=ctx)


def call_abi(kind, obj, ctx, x, xq, k, L, entry=0, rounds=0, want_stats=True, N=None, K=None, status=0):
    """the C call into guarded buffers -> (D, I, stats) numpy; guards, inputs and the d2h counter are checked.  status != 0: the call
    must return it, name "search" and write nothing."""
    torch, lib = _t(), _L()
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    qt = torch.from_numpy(np.ascontiguousarray(xq, dtype=np.float32)).cuda()
    nq, d = qt.shape
    wD, vD = cr.guarded((nq, max(k, 1)), np.int32, device="cuda")  # (k = 0 is a refusal: the buffers only have to exist)
    wI, vI = cr.guarded((nq, max(k, 1)), np.int64, device="cuda")
    wS, vS = cr.guarded((nq, 2), np.int32, device="cuda")
    tail = (lib.ptr(xt), d, nq, lib.ptr(qt), k, L, entry, rounds, lib.ptr(vD), lib.ptr(vI), lib.ptr(vS) if want_stats else None)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d2h = ctx.d2h_bytes()
    torch.cuda.synchronize()
    if kind == "raw":
        st = lib.lib().vidc_rows_search_dev(ctx.h, obj.shape[0] if N is None else N, obj.shape[1] if K is None else K, lib.ptr(obj), *tail)
    else:
        fn = lib.lib().vidc_compact_search_dev if kind == "compact" else lib.lib().vidc_ef_search_dev
        st = fn(ctx.h, obj.h, *tail)
    torch.cuda.synchronize()
    what = f"{kind} nq={nq} k={k} L={L}"
    assert st == status, (what, st, lib.lib().vidc_last_error())
    assert ctx.d2h_bytes() == d2h, f"{what}: the search moved id payload to the host"
    if status:
        assert b"search" in lib.lib().vidc_last_error(), lib.lib().vidc_last_error()
        for w, v in ((wD, vD), (wI, vI), (wS, vS)):
            cr.assert_untouched(w, v, what)
        return None
    for w, v, name in ((wD, vD, "D"), (wI, vI, "I"), (wS, vS, "stats")):
        cr.assert_guards_intact(w, v, f"{what}: {name}")
    if not want_stats:
        cr.assert_untouched(wS, vS, what)
    assert np.array_equal(qt.cpu().numpy(), np.asarray(xq, dtype=np.float32)), f"{what}: the queries changed"
    return vD.view(torch.float32).cpu().numpy().copy(), vI.cpu().numpy().copy(), vS.cpu().numpy().view(np.uint32).copy()


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("D", "I", "stats")):
        w = np.asarray(w)
        bad = np.argwhere(np.asarray(g) != w)
        assert np.asarray(g).shape == w.shape and bad.size == 0, f"{what}: {name} differs at {bad[:4].tolist()} ({bad.shape[0]} elements)"


@pytest.fixture(scope="module")
def ctx():
    return _L().default_context()


@pytest.fixture(scope="module")
def objs(ctx):
    """the three containers of every shape, built once"""
    out = {}
    for name in gr.SHAPES:
        s = gr.shape(name)
        for kind in KINDS:
            out[name, kind] = build(kind, s["rows"])
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(gr.SHAPES))
def test_search_device_equals_the_model(name, kind):
    from vector_db_id_compression_amd import VidcError, altid

    gs, s = _gs(), gr.shape(name)
    graph = gs.RawGraph(s["rows"]) if kind == "raw" else (altid.CompactBitNSGGraph if kind == "compact" else altid.EliasFanoNSGGraph)(s["rows"])
    if kind == "ef" and s["K"] > 64:  # rows wider than 64 edges have no arena: refused, by name
        with pytest.raises(VidcError, match="EliasFanoNSGGraph.*64"):
            gs.search_device(graph, s["x"], s["xq"], s["k"], L=s["L"])
        return
    xt = _t().from_numpy(s["x"].copy()).cuda()
    D, I, st = gs.search_device(graph, xt, s["xq"], s["k"], L=s["L"], stats=True)
    assert D.is_cuda and I.is_cuda and st.is_cuda and D.dtype == _t().float32 and I.dtype == _t().int64
    assert_equal((D.cpu().numpy(), I.cpu().numpy(), st.cpu().numpy().view(np.uint32)), gr.expected(name), f"{name} {kind}")
    D2, I2 = gs.search_device(graph, s["x"], s["xq"], s["k"], L=s["L"])  # host vectors are uploaded; no stats: two results
    assert _t().equal(D2, D) and _t().equal(I2, I)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_rows_through_the_abi(objs, ctx, kind):
    """K = 80: two trips per row (raw, compact); an asserted refusal for Elias-Fano"""
    s = gr.shape("n700_k80")
    if kind == "ef":
        call_abi(kind, objs["n700_k80", kind], ctx, s["x"], s["xq"], s["k"], s["L"], status=UNSUPPORTED)
    else:
        assert_equal(call_abi(kind, objs["n700_k80", kind], ctx, s["x"], s["xq"], s["k"], s["L"]), gr.expected("n700_k80"), kind)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_sizes(objs, ctx, kind):
    s = gr.shape("n500")
    want = gr.expected("n500")
    for nq in (1, 63, 64, 65, 300):
        idx = np.arange(nq) % s["nq"]
        got = call_abi(kind, objs["n500", kind], ctx, s["x"], s["xq"][idx], s["k"], s["L"])
        assert_equal(got, [w[idx] for w in want], f"{kind} nq={nq}")


@pytest.mark.parametrize("kind", KINDS)
def test_parameters(objs, ctx, kind):
    for name, k, L, rounds in (("n500", 32, 32, 0), ("n500", 10, 32, 1), ("n500", 10, 32, 3), ("n2000", 10, 64, 3), ("n300", 1, 1, 0),
                               ("n300", 8, 256, 0), ("n300", 256, 256, 0)):
        s = gr.shape(name)
        got = call_abi(kind, objs[name, kind], ctx, s["x"], s["xq"], k, L, rounds=rounds)
        assert_equal(got, gr.expected(name, k=k, L=L, max_rounds=rounds), f"{kind} {name} k={k} L={L} rounds={rounds}")
    s = gr.shape("n300")  # no stats array, another entry node
    want = gr.model(s["rows"], s["x"], s["xq"][:9], 8, 8, entry=299)
    got = call_abi(kind, objs["n300", kind], ctx, s["x"], s["xq"][:9], 8, 8, entry=299, want_stats=False)
    assert_equal(got[:2], want[:2], f"{kind} entry=299")


@pytest.mark.parametrize("kind", KINDS)
def test_scalar_distance_path(ctx, kind):
    """d = 7 is no multiple of 4: a component per lane and load, 8 lanes per neighbour; d = 3 through a misaligned query array"""
    s = gr.shape("n300")
    obj = build(kind, s["rows"])
    for d in (7, 3):
        x, xq = np.ascontiguousarray(s["x"][:, :d]), np.ascontiguousarray(s["xq"][:, :d])
        assert_equal(call_abi(kind, obj, ctx, x, xq, 8, 8), gr.model(s["rows"], x, xq, 8, 8), f"{kind} d={d}")
    torch = _t()
    x4 = torch.zeros(s["N"] * 8 + 1, device="cuda")[1:].view(s["N"], 8)  # d = 8 from a 4-byte aligned array: the scalar path too
    x4.copy_(torch.from_numpy(s["x"].copy()))
    assert x4.data_ptr() % 16 == 4
    assert_equal(call_abi(kind, obj, ctx, x4, s["xq"], 8, 8), gr.expected("n300"), f"{kind} misaligned x")


def ef_image(obj):
    lib = _L()
    lw, hw = C.c_uint64(), C.c_uint64()
    lib.check(lib.lib().vidc_ef_stream_words(obj.h, C.byref(lw), C.byref(hw)))
    low, high = np.zeros(max(lw.value, 1), np.uint64), np.zeros(max(hw.value, 1), np.uint64)
    lib.check(lib.lib().vidc_ef_export_all(obj.ctx.h, obj.h, lib.ptr(low), low.size, lib.ptr(high), high.size))
    info = obj.info()
    return [low, high, info["sizes"], info["low_bits"], info["universe"]]


def test_objects_are_unchanged_and_the_arena_is_read_in_place(ctx):
    from vector_db_id_compression_amd import persist

    s = gr.shape("n500")
    want = gr.expected("n500")
    c = build("compact", s["rows"])
    im0 = persist.compact_image(c)
    assert_equal(call_abi("compact", c, ctx, s["x"], s["xq"], s["k"], s["L"]), want, "compact")
    assert np.array_equal(persist.compact_image(c), im0)
    e = build("ef", s["rows"])  # fresh: its per-list streams do not exist yet
    assert_equal(call_abi("ef", e, ctx, s["x"], s["xq"], s["k"], s["L"]), want, "ef before export")
    im1 = ef_image(e)  # (the export builds the streams)
    assert_equal(call_abi("ef", e, ctx, s["x"], s["xq"], s["k"], s["L"]), want, "ef after export")
    im2 = ef_image(e)
    assert all(np.array_equal(a, b) for a, b in zip(im1, im2))
    out, cnt = e.decode_rows(None, s["K"])
    ref = np.sort(np.where(s["rows"] < 0, np.iinfo(np.int32).max, s["rows"]), axis=1)
    assert np.array_equal(np.where(out.cpu().numpy() < 0, np.iinfo(np.int32).max, out.cpu().numpy()), ref)


@pytest.mark.parametrize("kind", KINDS)
def test_hostile_rows(ctx, kind):
    from vector_db_id_compression_amd import VidcError, persist

    for empty_entry in (False, True):
        h = gr.hostile(entry_row_empty=empty_entry, big_ids=(kind == "raw"))  # (only raw rows can carry an id >= N)
        obj = build(kind, h["rows"])
        want = gr.model(h["rows"], h["x"], h["xq"], h["k"], h["L"])
        assert_equal(call_abi(kind, obj, ctx, h["x"], h["xq"], h["k"], h["L"]), want, f"{kind} hostile empty_entry={empty_entry}")
    if kind == "compact":  # the same id through a hand-made image: the import refuses it, so no search ever decodes it
        h = gr.hostile(big_ids=False)
        c = build("compact", h["rows"])
        img = persist.compact_image(c).copy()
        bits, N = c.bits, h["N"]
        assert N + 1 < (1 << bits)
        word = int.from_bytes(img[2, :8].tobytes(), "little")
        word = (word & ~((1 << bits) - 1)) | (N + 1)  # field 0 of row 2, in front of its sentinel
        img[2, :8] = np.frombuffer(word.to_bytes(8, "little"), np.uint8)
        with pytest.raises(VidcError, match="row 2"):
            persist.compact_from_image(N, h["K"], img)


@pytest.mark.parametrize("kind", ("compact", "ef"))
def test_updated_and_loaded_objects(ctx, kind, tmp_path):
    from vector_db_id_compression_amd import VidcError, codecs, persist

    s = gr.shape("n500")
    N, K, n_new = s["N"], s["K"], s["N"] + 37
    rng = np.random.default_rng(17)
    nodes = np.concatenate([rng.choice(N, 40, replace=False), np.arange(N, N + 20)]).astype(np.int64)
    batch = np.full((nodes.size, K), -1, np.int32)
    for i, n in enumerate(rng.integers(0, K + 1, size=nodes.size)):
        batch[i, :n] = rng.choice(n_new, size=int(n), replace=False)
    nodes[0], batch[0, :4] = 0, [N, N + 1, N + 19, 7]  # the entry's row leads into the new nodes
    rows = np.full((n_new, K), -1, np.int32)
    rows[:N] = s["rows"]
    rows[nodes] = batch
    x = np.concatenate([s["x"], rng.integers(-s["R"], s["R"] + 1, size=(n_new - N, s["d"])).astype(np.float32)])
    want = gr.model(rows, x, s["xq"], s["k"], s["L"])
    old = build(kind, s["rows"])
    new = codecs.update_rows(old, nodes, batch, n_new=n_new)
    assert_equal(call_abi(kind, new, ctx, x, s["xq"], s["k"], s["L"]), want, f"{kind} updated")
    assert_equal(call_abi(kind, old, ctx, s["x"], s["xq"], s["k"], s["L"]), gr.expected("n500"), f"{kind}: the old object")
    path = persist.save(new, str(tmp_path / f"g_{kind}"))
    loaded = persist.load(path)
    if kind == "compact":
        assert_equal(call_abi(kind, loaded, ctx, x, s["xq"], s["k"], s["L"]), want, "compact loaded")
    else:  # a loaded Elias-Fano image is a list object (per-list streams, no arena): refused, not searched
        call_abi(kind, loaded, ctx, x, s["xq"], s["k"], s["L"], status=UNSUPPORTED)
        assert b"lists" in _L().lib().vidc_last_error()
        with pytest.raises(VidcError, match="EfLists.*lists"):
            _gs().search_device(loaded, x, s["xq"], s["k"], L=s["L"])


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


@pytest.mark.parametrize("kind", KINDS)
def test_one_cu_context_every_slot_is_reused(small, kind):
    """32 slots, 101 queries: every visited set serves three or four queries, from scratch that was handed out full of 0xFF.  A slot
    that is not cleared in front of a query loses candidates."""
    s = gr.shape("n500")
    obj = build(kind, s["rows"], ctx=small)
    idx = (np.arange(ONE_CU_NQ) * 7) % s["nq"]
    want = [w[idx] for w in gr.expected("n500")]
    for _ in range(2):  # (the second call gets the first one's block back from the cache)
        assert_equal(call_abi(kind, obj, small, s["x"], s["xq"][idx], s["k"], s["L"]), want, f"{kind} one CU")


def test_float_data(ctx):
    N, d, K, k, L, nq = 2000, 16, 24, 10, 64, 40
    rng = np.random.default_rng(23)
    rows = gr.random_rows(rng, N, K)
    rows[0, : K // 2] = rng.choice(np.arange(1, N), size=K // 2, replace=False)
    x, xq = rng.normal(size=(N, d)).astype(np.float32), rng.normal(size=(nq, d)).astype(np.float32)
    res = {kind: call_abi(kind, build(kind, rows), ctx, x, xq, k, L) for kind in KINDS}
    D, I, st = res["raw"]
    for kind in ("compact", "ef"):  # a (query, node) distance has the same bits whichever container led to it
        assert_equal(res[kind], res["raw"], f"float {kind} vs raw")
    assert (I >= 0).all() and (I < N).all() and (st[:, 0] >= 3).all()
    for q in range(nq):
        assert len(set(I[q].tolist())) == k
        assert (np.diff(D[q]) >= 0).all()
    exact = ((x[I].astype(np.float64) - xq[:, None, :].astype(np.float64)) ** 2).sum(2)
    # float32 sum of d squares of float32 differences: (d + 2) roundings of 2^-24 relative each, all terms non-negative
    assert (np.abs(D.astype(np.float64) - exact) <= (d + 2) * 2.0 ** -23 * exact).all()


def test_refusals_on_a_live_context(objs, ctx):
    from vector_db_id_compression_amd import codecs

    s = gr.shape("n500")
    N = s["N"]
    for kind in KINDS:
        o = objs["n500", kind]
        for kw in (dict(k=0, L=32), dict(k=33, L=32), dict(k=10, L=257), dict(k=10, L=32, entry=N), dict(k=10, L=32, entry=2 ** 32 - 1)):
            call_abi(kind, o, ctx, s["x"], s["xq"], status=INVALID, **kw)
    call_abi("raw", objs["n500", "raw"], ctx, s["x"], s["xq"], 10, 32, K=0, status=INVALID)
    call_abi("raw", objs["n500", "raw"], ctx, s["x"], s["xq"], 10, 32, N=2 ** 31, status=INVALID)
    lists = codecs.EfLists.encode(np.array([0, 3, 5], np.uint64), np.array([1, 4, 9, 2, 7], np.uint64).view(np.int64))
    call_abi("ef", lists, ctx, s["x"], s["xq"], 10, 32, status=UNSUPPORTED)
    call_abi("ef", objs["n700_k80", "ef"], ctx, s["x"], s["xq"], 10, 32, status=UNSUPPORTED)
    lib = _L()
    tail = (None, s["d"], 0, None, 10, 32, 0, 0, None, None, None)  # nq == 0: nothing is launched, no array is needed
    assert lib.lib().vidc_compact_search_dev(ctx.h, objs["n500", "compact"].h, *tail) == 0
    assert lib.lib().vidc_ef_search_dev(ctx.h, objs["n500", "ef"].h, *tail) == 0
    # the context is still usable
    assert_equal(call_abi("ef", objs["n500", "ef"], ctx, s["x"], s["xq"], s["k"], s["L"]), gr.expected("n500"), "after the refusals")
