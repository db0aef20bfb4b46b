"""vidc_{compact,ef,roc}_update_rows_dev: rows of a graph object replaced and nodes added on the device.

The statement under test: the updated object IS the object the existing row encoder builds from the updated matrix R' of the numpy
model (tests/rows_update_ref.py) -- every exported byte / word, every size, every per-row field -- and decodes to R' through every
decode form.  Compact and Elias-Fano are also compared with the closed-form model of tests/rows_ref.py, ROC streams of a sample of rows
with the pinned oracle.  Every comparison is between integers and exact.

Shapes: node counts 1, around the 64-row tile, several tiles; K = 1, 7, 32, 33, 64 (compact also 100); batches of 0, 1, 63, 64, 65 and
1000 rows with repeated nodes inside a tile and across tiles, negative nodes, nodes beyond the object, every node named; growth by 0,
1 (a new node without a row) and more, across the compact width steps 255 -> 256 and 1023 -> 1024, and across a step of the
Elias-Fano record bound that the test looks for with the model and asserts to have crossed."""
import ctypes as C

import numpy as np
import pytest

import rows_ref as rr
import rows_update_ref as ru
import test_gpu_graph_rows as gr

pytestmark = pytest.mark.gpu

N_OLDS = [1, 63, 64, 65, 200, 1000]
MS = [0, 1, 63, 64, 65, 1000]
KS = [1, 7, 32, 33, 64]
GROW = [0, 1, 0, 37, 1, 0, 130]
CONTENT = ["uniform", "blocks", "degrees", "l_steps"]  # blocks: full rows (no sentinel) and empty rows; degrees: every sentinel position
ROC_SAMPLE = 48


def _torch():
    import torch

    return torch


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _cases():
    out = []
    for i, n_old in enumerate(N_OLDS):
        for j, m in enumerate(MS):
            k = i * len(MS) + j
            out.append((n_old, KS[(i + j) % len(KS)], m, ru.BATCHES[k % len(ru.BATCHES)], GROW[k % len(GROW)], CONTENT[k % len(CONTENT)]))
    return out


CASES = _cases()


def make_case(n_old, K, m, batch_name, grow, content, seed=0):
    """-> (old rows, nodes, batch rows, n_new): ids of the batch rows lie below n_new, old ids below n_old"""
    n_new = n_old + grow
    rows = rr.family("uniform" if content != "degrees" else "degrees", n_old, K, seed=seed + 1)
    batch = rr.family(content, n_new, K, seed=seed + 2, nrows=m) if m else np.zeros((0, K), np.int32)
    nodes = ru.batch_nodes(batch_name, m, n_new, seed=seed + 3)
    return rows, nodes, batch, n_new


def compact_image(c):
    from vector_db_id_compression_amd import persist

    return persist.compact_image(c)


def run_update(obj, nodes, batch, n_new, **kw):
    """update_rows with device-resident inputs and an invalid counter -> (new object, invalid count); the payload counter must not move"""
    torch = _torch()
    d_nodes = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int64)).cuda()
    d_rows = torch.from_numpy(np.ascontiguousarray(batch, dtype=np.int32)).cuda()
    invalid = torch.zeros(1, dtype=torch.int64, device="cuda")
    before = obj.ctx.d2h_bytes()
    new = _codecs().update_rows(obj, d_nodes, d_rows, n_new=n_new, invalid=invalid, **kw)
    assert obj.ctx.d2h_bytes() == before, "row payload crossed PCIe"
    return new, int(invalid.item())


# --------------------------------------------------------------------------------------------------------------- per codec
def same_compact(got, fresh, R, what):
    N, K = R.shape
    assert (got.N, got.K) == (N, K)
    assert (got.bits, got.stride, got.size_in_bytes) == (fresh.bits, fresh.stride, fresh.size_in_bytes), f"{what}: bits / stride / size"
    assert (got.bits, got.stride) == (rr.compact_bits(N), rr.compact_stride(N, K)), what
    a, b = compact_image(got), compact_image(fresh)
    assert np.array_equal(a, b), f"{what}: export_all against encode_rows(R') {gr._diff(a, b)}"
    assert np.array_equal(a, rr.compact_rows(R)), f"{what}: export_all against the model {gr._diff(a, rr.compact_rows(R))}"
    want, deg = rr.expected_compact(R)
    gr.check_decodes(got, K, want, deg, what)


def same_ef(got, fresh, R, what):
    N, K = R.shape
    gi, fi = got.info(), fresh.info()
    m = rr.ef_rows(R)
    for key in ("sizes", "low_bits", "universe"):
        assert np.array_equal(gi[key], fi[key]), f"{what}: {key} {gr._diff(gi[key], fi[key])}"
    assert np.array_equal(gi["sizes"], m.n) and np.array_equal(gi["low_bits"], m.l) and np.array_equal(gi["universe"], m.u.astype(np.uint64)), what
    assert got.compressed_bytes == fresh.compressed_bytes == m.size_in_bytes, f"{what}: compressed_bytes"
    want, deg = rr.expected_ef(R)
    gr.check_decodes(got, K, want, deg, what)  # (the arena decoders, before the CSR streams exist)
    wide, cnt = got.decode_rows(None, K + 3)   # K above the object's K
    wide = wide.cpu().numpy()
    assert np.array_equal(wide[:, :K], want) and (wide[:, K:] == -1).all() and np.array_equal(cnt, deg), f"{what}: decode_rows at K + 3"
    a, b = gr.ef_all_words(got), gr.ef_all_words(fresh)
    assert (a[0].size, a[1].size) == (b[0].size, b[1].size), f"{what}: stream_words"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), f"{what}: export_all"
    for i in gr.sample_rows(N, False, seed=N)[:: max(1, N // 40)]:
        low, high, lb, hb = got.export(int(i))
        wl, wh = m.words(i)
        assert (lb, hb) == (int(m.low_nbits[i]), int(m.high_nbits[i])) and np.array_equal(low, wl) and np.array_equal(high, wh), f"{what}: row {i}"


def same_roc(got, fresh, R, what, oracle=None, key=None):
    N, K = R.shape
    deg = rr.row_degrees(R)
    gi, fi = got.info(), fresh.info()
    for name in ("sizes", "precision", "heads", "nwords", "mt_draws"):
        assert np.array_equal(gi[name], fi[name]), f"{what}: {name} {gr._diff(gi[name], fi[name])}"
    assert np.array_equal(gi["sizes"], deg), what
    assert (got.total_words, got.compressed_bytes, got.ntotal, got.nlist) == (fresh.total_words, fresh.compressed_bytes, fresh.ntotal, N), what
    wa, wb = got.all_words(), fresh.all_words()
    assert np.array_equal(wa, wb), f"{what}: export_all_words {gr._diff(wa, wb)}"
    every_f = fresh.decode_rows(None, K)[0].cpu().numpy()
    every, cnt = got.decode_rows(None, K)
    assert np.array_equal(every.cpu().numpy(), every_f) and np.array_equal(cnt, deg), f"{what}: decode_rows(None)"
    nodes = gr.request_nodes(N, seed=N)
    idx = nodes.astype(np.int64)
    sub, c2 = got.decode_rows(nodes, K)
    assert np.array_equal(sub.cpu().numpy(), every_f[idx]) and np.array_equal(c2, deg[idx]), f"{what}: decode_rows(host nodes)"
    dsub, c3 = got.decode_rows(_torch().from_numpy(np.concatenate([idx, [-1]])).cuda(), K)
    dsub = dsub.cpu().numpy()
    assert np.array_equal(dsub[:-1], every_f[idx]) and (dsub[-1] == -1).all() and np.array_equal(c3.cpu().numpy()[:-1], deg[idx]), f"{what}: CUDA nodes"
    if oracle is not None:
        rng = np.random.default_rng(N + K)
        only = np.unique(np.concatenate([[0, N - 1], rng.integers(0, N, ROC_SAMPLE)]))
        exp = gr.roc_expectation(oracle, R, key, only)
        woff = np.concatenate([[0], np.cumsum(gi["nwords"].astype(np.int64))])
        for i in only[deg[only] > 0]:
            assert (gi["precision"][i], gi["heads"][i], gi["nwords"][i], gi["mt_draws"][i]) == (exp["prec"][i], exp["heads"][i], exp["nwords"][i], exp["draws"][i]), f"{what}: row {i}"
            assert np.array_equal(wa[woff[i]:woff[i + 1]], exp["words"][int(i)]), f"{what}: row {i}: stack words against the oracle"
        assert np.array_equal(every_f[only], exp["dec"][only]), f"{what}: decode against the oracle"


def check_codec(codec, rows, nodes, batch, n_new, what, oracle=None, key=None):
    """old = encode_rows(rows); new = codecs.update_rows(old, batch); new against encode_rows(R'); old untouched -> (old, new, R')"""
    cd = _codecs()
    cls = {"compact": cd.CompactRows, "ef": cd.EfLists, "roc": cd.RocLists}[codec]
    R, want_invalid, _ = ru.update_rows(rows, nodes, batch, n_new)
    old = cls.encode_rows(gr.dev_rows(rows))
    image = {"compact": compact_image, "ef": gr.ef_all_words, "roc": lambda o: o.all_words()}[codec]
    before = image(old)
    new, invalid = run_update(old, nodes, batch, n_new)
    assert invalid == want_invalid, f"{what}: *d_invalid {invalid}, model {want_invalid}"
    fresh = cls.encode_rows(gr.dev_rows(R))
    tag = f"{what} {codec}"
    if codec == "compact":
        same_compact(new, fresh, R, tag)
    elif codec == "ef":
        same_ef(new, fresh, R, tag)
    else:
        same_roc(new, fresh, R, tag, oracle, key)
    after = image(old)
    for a, b in zip(before if isinstance(before, tuple) else (before,), after if isinstance(after, tuple) else (after,)):
        assert np.array_equal(a, b), f"{tag}: the old object changed"
    return old, new, R


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("n_old,K,m,batch_name,grow,content", CASES)
def test_update_is_the_fresh_encode(n_old, K, m, batch_name, grow, content, oracle):
    rows, nodes, batch, n_new = make_case(n_old, K, m, batch_name, grow, content, seed=n_old + m)
    what = f"N {n_old} -> {n_new} K {K} m {m} {batch_name} {content}"
    for codec in ("compact", "ef", "roc"):
        check_codec(codec, rows, nodes, batch, n_new, what, oracle, (what, "roc"))


def test_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(N_OLDS) and {c[2] for c in CASES} == set(MS) and {c[1] for c in CASES} == set(KS)
    assert {c[3] for c in CASES} == set(ru.BATCHES) and {c[4] for c in CASES} >= {0, 1, 37} and {c[5] for c in CASES} == set(CONTENT)
    # a batch that names every node, with room to spare; a growth by one without a row for the new node
    assert any(c[3].startswith("every_node") and c[2] >= c[0] + c[4] for c in CASES)
    full = rr.family("blocks", 200, 32, seed=2, nrows=65)
    assert (rr.row_degrees(full) == 32).any() and (rr.row_degrees(full) == 0).any()  # full rows (no sentinel), rows emptied


@pytest.mark.parametrize("K", [32, 5, 100])
@pytest.mark.parametrize("n_old,n_new", [(255, 256), (1023, 1024), (300, 301), (255, 1024), (256, 256)])
def test_compact_width_steps_and_sentinels(n_old, n_new, K):
    """8 -> 9 and 10 -> 11 bits (every field re-packed), a growth that keeps the width (every sentinel still changes), two steps at
    once, and no growth; through the tile stride (K = 32), an odd stride (K = 5) and the wide walk (K = 100)"""
    stepped = rr.compact_bits(n_old) != rr.compact_bits(n_new)
    assert stepped == ((n_old, n_new) in ((255, 256), (1023, 1024), (255, 1024)))
    rows = rr.family("degrees", n_old, K, seed=K)
    m = 70
    batch = rr.family("degrees", n_new, K, seed=K + 1, nrows=m)
    batch[0, 0] = n_new - 1  # the largest id the new width must hold
    batch[0, 1:] = -1
    nodes = ru.batch_nodes("mixed", m, n_new, seed=K)
    nodes[0] = n_new - 1     # (a new node with a row, unless a later mention takes it)
    check_codec("compact", rows, nodes, batch, n_new, f"compact N {n_old} -> {n_new} K {K}")


def _lw(K, U):
    return (rr.record_bound(K, U)[0] + 63) // 64


@pytest.mark.parametrize("K", [7, 33, 64])
def test_ef_restride_across_a_step_of_the_record_bound(K):
    """The low words of an arena record step with the largest id: found here with the model, crossed once by growing N, once by a batch
    id far above N, and once backwards (the row with the large id is replaced: the record shrinks again)."""
    U = next(u for u in range(66, 1 << 16) if _lw(K, u) > _lw(K, u - 1))  # the first id that needs one more low word
    n_old, n_new = U, U + 1                                               # ids < n_old fit LW - 1, n_new - 1 == U does not
    assert _lw(K, n_new - 1) == _lw(K, n_old - 1) + 1, "the step was not crossed"
    rows = rr.family("max_low", n_old, K, seed=K)
    batch = rr.family("max_low", n_new, K, seed=K + 1, nrows=65)
    nodes = ru.batch_nodes("repeats_in_tile", 65, n_new, seed=K)
    nodes[-1] = n_new - 1
    old, new, R = check_codec("ef", rows, nodes, batch, n_new, f"ef growth across the bound K {K}")
    # a large id, no growth: the geometry follows the id (as encode_rows' second pass does)
    big = next(u for u in (4 * n_old << sh for sh in range(24)) if _lw(K, u) > _lw(K, n_old - 1) + 1) + 1
    b2 = rr.family("uniform", n_old, K, seed=3, nrows=3)
    b2[1, 0] = big
    nodes2 = np.array([5 % n_old, 7 % n_old, -1], np.int64)
    assert _lw(K, big) > _lw(K, n_old - 1)
    old2, new2, R2 = check_codec("ef", rows, nodes2, b2, n_old, f"ef batch id {big} K {K}")
    assert int(new2.info()["universe"].max()) == big
    # ... and back: the row that holds it is replaced by a small one
    b3 = rr.family("uniform", n_old, K, seed=4, nrows=1)
    new3, inv = run_update(new2, np.array([7 % n_old]), b3, n_old)
    R3, _, _ = ru.update_rows(R2, np.array([7 % n_old]), b3, n_old)
    assert R3.max() < n_old and inv == 0
    same_ef(new3, _codecs().EfLists.encode_rows(gr.dev_rows(R3)), R3, f"ef back below the bound K {K}")


@pytest.mark.parametrize("codec", ["compact", "ef", "roc"])
def test_update_of_an_updated_object_save_load_and_lifetimes(codec, oracle, tmp_path):
    from vector_db_id_compression_amd import persist

    n_old, K = 200, 33
    rows, nodes, batch, n_new = make_case(n_old, K, 65, "mixed", 20, "degrees", seed=7)
    old, new, R = check_codec(codec, rows, nodes, batch, n_new, "first update", oracle, ("compose", 1))
    rows2, nodes2, batch2, n_new2 = make_case(n_new, K, 64, "every_node_twice", 1, "blocks", seed=8)
    new2, inv = run_update(new, nodes2, batch2, n_new2)
    R2, want_inv, _ = ru.update_rows(R, nodes2, batch2, n_new2)
    assert inv == want_inv
    cd = _codecs()
    cls = {"compact": cd.CompactRows, "ef": cd.EfLists, "roc": cd.RocLists}[codec]
    same = {"compact": same_compact, "ef": same_ef, "roc": same_roc}[codec]
    same(new2, cls.encode_rows(gr.dev_rows(R2)), R2, f"{codec}: update of an updated object")
    # save / load / decode
    back = persist.load(persist.save(new2, str(tmp_path / f"{codec}.npz")))
    want = {"compact": rr.expected_compact(R2)[0], "ef": rr.expected_ef(R2)[0], "roc": new2.decode_rows(None, K)[0].cpu().numpy()}[codec]
    got, cnt = back.decode_rows(None, K)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cnt, rr.row_degrees(R2)), f"{codec}: decode after save / load"
    # either may be destroyed first: the middle object goes, its parent and its child still answer
    want_old = old.decode_rows(None, K)[0].cpu().numpy().copy()
    del new, back
    _lib().default_context().trim()
    assert np.array_equal(old.decode_rows(None, K)[0].cpu().numpy(), want_old), f"{codec}: the old object after its child was destroyed"
    del old
    assert np.array_equal(new2.decode_rows(None, K)[0].cpu().numpy(), want), f"{codec}: the new object after its parents were destroyed"
    # m == 0, no growth: an equal object
    eq, inv = run_update(new2, np.zeros(0, np.int64), np.zeros((0, K), np.int32), None)
    same(eq, cls.encode_rows(gr.dev_rows(R2)), R2, f"{codec}: empty update")


@pytest.mark.parametrize("mode", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE", "VIDC_FORCE_LANE"])
def test_modes(mode, oracle, monkeypatch):
    """the kernel families of the ROC rows path (the streams do not depend on them); the other two codecs have one path"""
    monkeypatch.setenv(mode, "1")
    for n_old, K, m, name, grow, content in ((200, 64, 65, "mixed", 1, "degrees"), (65, 7, 1000, "every_node_twice", 0, "uniform")):
        rows, nodes, batch, n_new = make_case(n_old, K, m, name, grow, content, seed=11)
        for codec in ("compact", "ef", "roc"):
            check_codec(codec, rows, nodes, batch, n_new, f"{mode} N {n_old} K {K}", oracle, (mode, n_old, K))


def test_poisoned_pool(oracle):
    """every cached device block is 0xFF when it is handed out: unused record words, empty rows and fields behind a sentinel must be
    written, not inherited.  Twice: the second pass takes the blocks the first one released."""
    ctx = _lib().default_context()
    ctx.set_pool_poison(True)
    try:
        for _ in range(2):
            for n_old, K, m, name, grow, content in ((129, 64, 65, "mixed", 70, "blocks"), (200, 7, 64, "negatives", 1, "degrees")):
                rows, nodes, batch, n_new = make_case(n_old, K, m, name, grow, content, seed=5)
                for codec in ("compact", "ef", "roc"):
                    check_codec(codec, rows, nodes, batch, n_new, f"poisoned N {n_old} K {K}", oracle, ("poison", n_old, K))
    finally:
        ctx.set_pool_poison(False)


def test_refusals_leave_out_null_and_the_context_usable():
    cd = _codecs()
    L, VidcError = _lib().lib(), _lib().VidcError
    torch = _torch()
    N, K = 100, 8
    rows = rr.family("uniform", N, K, seed=1)
    good_nodes, good_batch = np.array([3, 4], np.int64), rr.family("uniform", N, K, seed=2, nrows=2)
    off = np.arange(0, 33, 8, dtype=np.uint64)
    ids = torch.arange(32, dtype=torch.int64, device="cuda")
    wide_rows = rr.family("uniform", 300, 128, seed=3)
    objs = {"compact": cd.CompactRows.encode_rows(gr.dev_rows(rows)), "ef": cd.EfLists.encode_rows(gr.dev_rows(rows)),
            "roc": cd.RocLists.encode_rows(gr.dev_rows(rows))}
    fns = {"compact": lambda o, m, nd, rw, n, out: L.vidc_compact_update_rows_dev(o.ctx.h, o.h, m, nd, rw, n, out, None),
           "ef": lambda o, m, nd, rw, n, out: L.vidc_ef_update_rows_dev(o.ctx.h, o.h, m, nd, rw, n, out, None),
           "roc": lambda o, m, nd, rw, n, out: L.vidc_roc_update_rows_dev(o.ctx.h, o.h, m, nd, rw, n, -1, out, None)}
    d_nodes = torch.from_numpy(good_nodes).cuda()
    d_batch = torch.from_numpy(good_batch).cuda()
    bad_id = {"compact": N, "ef": -5, "roc": -5}  # compact: outside [0, N_new); the others: a negative id before the terminator
    refused = {"ef": [cd.EfLists.encode(off, ids), cd.EfLists.encode_rows(gr.dev_rows(wide_rows))],
               "roc": [cd.RocLists.encode(off, ids), cd.RocLists.encode_rows(gr.dev_rows(wide_rows))], "compact": []}

    def good_call_follows(codec):
        new, inv = run_update(objs[codec], good_nodes, good_batch, N)
        R, _, _ = ru.update_rows(rows, good_nodes, good_batch, N)
        want = {"compact": lambda: rr.expected_compact(R)[0], "ef": lambda: rr.expected_ef(R)[0],
                "roc": lambda: cd.RocLists.encode_rows(gr.dev_rows(R)).decode_rows(None, K)[0].cpu().numpy()}[codec]()
        assert inv == 0 and np.array_equal(new.decode_rows(None, K)[0].cpu().numpy(), want), f"{codec}: a good call after a refusal"

    for codec, obj in objs.items():
        call = fns[codec]
        for o in refused[codec]:  # an IVF object, a wide (K = 128) object
            out = C.c_void_p(1)
            assert call(o, 2, d_nodes.data_ptr(), d_batch.data_ptr(), 300, C.byref(out)) == -6, codec
            assert out.value is None
            good_call_follows(codec)
        out = C.c_void_p(1)
        assert call(obj, 2, d_nodes.data_ptr(), d_batch.data_ptr(), N - 1, C.byref(out)) == -1 and out.value is None, f"{codec}: N_new < N_old"
        assert call(obj, 2, d_nodes.data_ptr(), d_batch.data_ptr(), (1 << 32) - 1, C.byref(out)) == -1 and out.value is None, f"{codec}: N_new too large"
        assert call(obj, 2, None, d_batch.data_ptr(), N, C.byref(out)) == -1 and call(obj, 2, d_nodes.data_ptr(), None, N, C.byref(out)) == -1, codec
        good_call_follows(codec)
        bad = good_batch.copy()
        bad[1, 1] = bad_id[codec]
        bad[1, 2] = 1
        with pytest.raises(VidcError, match="status -4"):
            cd.update_rows(obj, good_nodes, bad, n_new=N)
        out = C.c_void_p(1)
        d_bad = torch.from_numpy(bad).cuda()
        assert call(obj, 2, d_nodes.data_ptr(), d_bad.data_ptr(), N, C.byref(out)) == -4 and out.value is None, f"{codec}: out-of-domain id"
        good_call_follows(codec)
        # the same id behind the terminator is not looked at
        ok = good_batch.copy()
        ok[1, 1] = -1
        ok[1, 2] = bad_id[codec]
        new = cd.update_rows(obj, good_nodes, ok, n_new=N)
        assert int(new.decode_rows(np.array([4], np.uint64), K)[1][0]) == 1, codec


def test_altid_graph_classes_update_rows(oracle):
    from vector_db_id_compression_amd import altid

    N, K = 130, 33
    rows, nodes, batch, n_new = make_case(N, K, 65, "mixed", 7, "degrees", seed=3)
    R, _, _ = ru.update_rows(rows, nodes, batch, n_new)
    deg = rr.row_degrees(R)
    for cname, cls in (("compact", altid.CompactBitNSGGraph), ("elias-fano", altid.EliasFanoNSGGraph), ("roc", altid.ROCNSGGraph)):
        g = cls(rows.copy())
        u = g.update_rows(nodes, batch, n_new=n_new)
        f = cls(R.copy())
        assert type(u) is cls and (u.N, u.K) == (n_new, K) and g.N == N
        for attr in ("bits", "stride", "compressed_ids_size_in_bytes", "overhead_in_bytes"):
            if hasattr(f, attr):
                assert getattr(u, attr) == getattr(f, attr), (cname, attr)
        for attr in ("num_outgoing_edges", "id_symbol_precision"):
            if hasattr(f, attr):
                assert np.array_equal(getattr(u, attr), getattr(f, attr)), (cname, attr)
        out, cnt = u.get_neighbors_batch(np.arange(n_new))
        fo, fc = f.get_neighbors_batch(np.arange(n_new))
        assert np.array_equal(out, fo) and np.array_equal(cnt, deg) and np.array_equal(fc, deg), cname
        assert u.get_neighbors(n_new - 1).tolist() == fo[n_new - 1, : deg[n_new - 1]].tolist()
        same = g.update_rows(np.zeros(0, np.int64), np.zeros((0, K), np.int32))
        assert same.N == N and np.array_equal(same.get_neighbors_batch(np.arange(N))[0], g.get_neighbors_batch(np.arange(N))[0]), cname
