"""Output contracts of the decode entry points (include/vidc.h): after a call every element of the promised region is defined
-- rows: the ids, then -1 up to column K -- and not one byte outside that region has changed.

Every call goes through the C-ABI with the address of a poisoned view that has a guard band of 4 KiB on either side
(tests/contract_ref.py); the codecs.py wrappers allocate their own outputs and are used for encoding only.  After each call the guards
must be untouched and the WHOLE view must equal the reference that contract_ref computes from nothing but the ids that went into the
encoder (numpy + the CPU oracle).  Host result arrays (counts, out_offsets, ids_out) are numpy arrays with guards of their own.

The tests look for stray and missing writes inside memory they own; nothing here tries to make a kernel fault.
"""
import numpy as np
import pytest

import contract_ref as cr

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _L():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def ptr(x):
    return _L().ptr(x)


def check(status):
    _L().check(status)


def dev_i64(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


FAMILIES = {"default": None, "lane": "VIDC_FORCE_LANE", "nolane": "VIDC_NO_LANE", "general": "VIDC_FORCE_GENERAL"}


def set_family(monkeypatch, family):
    """the kernel-family switches are read per call"""
    for var in ("VIDC_FORCE_LANE", "VIDC_NO_LANE", "VIDC_FORCE_GENERAL"):
        monkeypatch.delenv(var, raising=False)
    if FAMILIES[family]:
        monkeypatch.setenv(FAMILIES[family], "1")


# ======================================================================================================================== rows
ROW_KS = [1, 3, 16, 31, 32, 33, 48, 63, 64, 65, 128]  # <= 64: arena / tile / tiny-lane objects; 65, 128: list-kernel objects
N_ROWS = 5003  # not a multiple of 64
BIG_ID_K = 48  # the Elias-Fano and ROC objects of this K also hold ids up to 2^30


def make_rows(K, big):
    """empty rows, full rows and everything between; ids below N (distinct inside a row); rows whose maximum is 0 or a power of two
    (the reference ROC codec's lossy case stays in the comparison)"""
    rng = np.random.default_rng(1000 + K)
    N = N_ROWS
    rows = np.full((N, K), -1, np.int32)
    deg = rng.integers(0, K + 1, N)
    deg[::89] = K
    deg[::97] = 0
    for i in range(N):
        d = int(deg[i])
        if d == 0:
            continue
        if i % 103 == 7:
            ids = np.zeros(1, np.int64)  # maximum 0
        elif i % 101 == 5:
            ids = np.concatenate([[4096], rng.choice(4096, d - 1, replace=False)])  # maximum 2^12
        elif big and i % 5 == 0:
            u = np.unique(rng.integers(0, 1 << 30, 2 * d + 8))
            ids = rng.permutation(u)[:d]
        else:
            ids = rng.choice(N, d, replace=False)
        rows[i, : ids.size] = ids
    return rows


def resolve_width(spec, K):
    if spec == "K":
        return K
    if spec == "K+1":
        return K + 1
    if spec == "up4":
        return (K // 4 + 1) * 4  # the next multiple of 4 above K
    return int(spec)


def width_class(w, K):
    return "=K" if w == K else ("<=64" if w <= 64 else ">64")


# (decode width, request form, bytes off a 16-byte boundary, kernel family).  Forms: "all" = nodes NULL, m = N; ("null", m) = nodes
# NULL; ("host", m) = host node list with repeats; ("dev", m) = device node list with negatives and nodes >= N.
# The family switches steer the ROC kernels only: an Elias-Fano object takes the same decoder under all four, so for it these
# entries are further (width, form, alignment) cases, not four kernel families.
ROW_COMBOS = [
    # width = the object's K
    ("K", "all", 0, "default"),
    ("K", ("host", 2048), 4, "default"),
    ("K", ("dev", 3000), 8, "lane"),
    ("K", ("null", 65), 12, "nolane"),
    # wider than the object, at most 64
    (64, "all", 0, "lane"),
    ("K+1", ("null", 63), 4, "default"),
    ("up4", ("host", 65), 8, "nolane"),
    (64, ("dev", 1000), 12, "general"),
    ("up4", ("null", 64), 0, "default"),
    # wider than 64
    (100, "all", 0, "default"),
    (65, ("host", 2047), 4, "lane"),
    (128, ("dev", 3000), 8, "default"),
    (200, ("host", 5000), 12, "nolane"),
    (128, ("null", 1), 0, "general"),
    (100, ("host", 1), 4, "default"),
    (65, ("dev", 1000), 12, "default"),
    (200, "all", 8, "general"),
]
COMPACT_COMBOS = [  # compact rows have no width argument
    ("all", 0), ("all", 4), ("all", 8), ("all", 12),
    (("null", 1), 4), (("null", 63), 8), (("null", 64), 12), (("null", 65), 0),
    (("host", 1), 8), (("host", 65), 12), (("host", 2047), 0), (("host", 2048), 4), (("host", 5000), 8),
    (("dev", 3000), 12), (("dev", 1000), 0), (("dev", 3000), 4), (("dev", 65), 8),
]


def combos_for(K):
    """ROW_COMBOS at an object of width K: widths below K dropped, duplicates after resolution dropped"""
    seen, out = set(), []
    for spec, form, align, family in ROW_COMBOS:
        w = resolve_width(spec, K)
        if w < K or (w, form, align, family) in seen:
            continue
        seen.add((w, form, align, family))
        out.append((w, form, align, family))
    return out


def _check_row_coverage():
    """the fixed list covers every width, form, alignment and family, and every (width class x alignment) pair at every tile object"""
    forms = {f for _, f, _, _ in ROW_COMBOS}
    assert forms >= {"all", ("null", 1), ("null", 63), ("null", 64), ("null", 65), ("host", 1), ("host", 65), ("host", 2047),
                     ("host", 2048), ("host", 5000)} and any(isinstance(f, tuple) and f[0] == "dev" for f in forms)
    assert {s for s, _, _, _ in ROW_COMBOS} >= {"K", "K+1", "up4", 64, 65, 100, 128, 200}
    assert {a for _, _, a, _ in ROW_COMBOS} == {0, 4, 8, 12} and {f for _, _, _, f in ROW_COMBOS} == set(FAMILIES)
    for K in ROW_KS:
        have = {(width_class(w, K), a) for w, _, a, _ in combos_for(K)}
        classes = ["=K", ">64"] + (["<=64"] if K < 64 else [])
        if K <= 64:
            assert have >= {(c, a) for c in classes for a in (0, 4, 8, 12)}, (K, have)
        assert {w for w, _, _, _ in combos_for(K)} >= {w for w in (K, K + 1, 100, 128, 200) if w >= K}
    cforms = {f for f, _ in COMPACT_COMBOS}
    assert cforms >= {f for f in forms if f == "all" or f[0] != "dev"} and any(f[0] == "dev" for f in cforms if f != "all")
    assert {a for _, a in COMPACT_COMBOS} == {0, 4, 8, 12}


_check_row_coverage()


def make_request(form, rng):
    """-> (m, nodes for the call or None, is_device).  Host lists hold repeats; device lists hold negatives and nodes >= N too."""
    N = N_ROWS
    if form == "all":
        return N, None, False
    what, m = form
    if what == "null":
        return m, None, False
    nodes = rng.integers(0, N, m).astype(np.int64)
    if m > 1:
        nodes[m // 2] = nodes[0]  # a repeat
        nodes[-1] = N - 1
    if what == "host":
        return m, nodes, False
    kind = rng.integers(0, 100, m)
    nodes[kind < 4] = -1
    nodes[(kind >= 4) & (kind < 6)] = -rng.integers(2, 1 << 62, int(((kind >= 4) & (kind < 6)).sum()))
    sel = (kind >= 6) & (kind < 10)
    nodes[sel] = N + rng.integers(0, 3, int(sel.sum())) * (1 << 33)
    nodes[0] = -1  # (the request's first node is not its first valid one)
    nodes[1] = N
    return m, nodes, True


def run_rows(kind, obj, ref, K_out, form, align, rng, what):
    """one decode call into guarded, poisoned buffers; everything it owns is compared in full"""
    torch = _torch()
    lib = _L().lib()
    m, nodes, is_dev = make_request(form, rng)
    exp, exp_cnt = ref.expected(np.arange(m) if nodes is None else nodes, K_out)
    whole, view = cr.guarded((m, K_out), np.int32, "cuda", None, align // 4)
    assert view.data_ptr() % 16 == align
    kargs = () if kind == "compact" else (K_out,)
    if is_dev:
        d_nodes = dev_i64(nodes)
        cw, cv = cr.guarded(m, np.uint32, "cuda")
        iw, iv = cr.guarded(1, np.uint64, "cuda")
        iv.zero_()
        fn = {"compact": lib.vidc_compact_rows_decode_dev, "ef": lib.vidc_ef_decode_rows_dev, "roc": lib.vidc_roc_decode_rows_dev}[kind]
        check(fn(obj.ctx.h, obj.h, m, ptr(d_nodes), *kargs, ptr(view), ptr(cv), ptr(iv)))
        torch.cuda.synchronize()
        assert np.array_equal(d_nodes.cpu().numpy(), nodes), f"{what}: the request was modified"
        cr.assert_guards_intact(iw, iv, what + " d_invalid")
        cr.assert_view_equals(iv, np.array([int((nodes >= N_ROWS).sum())], np.uint64), what + " d_invalid")
    else:
        nd = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.uint64)
        cw, cv = cr.guarded(m, np.uint32, "cpu")
        fn = {"compact": lib.vidc_compact_rows_decode, "ef": lib.vidc_ef_decode_rows, "roc": lib.vidc_roc_decode_rows}[kind]
        check(fn(obj.ctx.h, obj.h, m, ptr(nd), *kargs, ptr(view), ptr(cv)))
        torch.cuda.synchronize()
    cr.assert_guards_intact(whole, view, what + " rows")
    cr.assert_view_equals(view, exp, what + " rows")
    cr.assert_guards_intact(cw, cv, what + " counts")
    cr.assert_view_equals(cv, exp_cnt, what + " counts")


def _raise_all(failures):
    if failures:
        raise AssertionError(f"{len(failures)} call(s) broke the output contract:\n  " + "\n  ".join(failures))


@pytest.mark.parametrize("K", ROW_KS)
@pytest.mark.parametrize("kind", ["ef", "roc"])
def test_rows_fill_their_region_and_nothing_else(kind, K, monkeypatch, oracle):
    cd = _codecs()
    rows = make_rows(K, big=(K == BIG_ID_K))
    ref = cr.RowRef(kind, rows, oracle)
    obj = (cd.EfLists if kind == "ef" else cd.RocLists).encode_rows(rows)
    rng = np.random.default_rng(K)
    failures = []
    for w, form, align, family in combos_for(K):
        what = f"{kind} K={K} width={w} ({width_class(w, K)}) form={form} align={align} family={family}"
        set_family(monkeypatch, family)
        try:
            run_rows(kind, obj, ref, w, form, align, rng, what)
        except (AssertionError, _L().VidcError) as e:
            failures.append(f"{what}: {str(e).splitlines()[0]}")
    _raise_all(failures)


@pytest.mark.parametrize("K", ROW_KS)
def test_compact_rows_fill_their_region_and_nothing_else(K):
    rows = make_rows(K, big=False)
    ref = cr.RowRef("compact", rows)
    obj = _codecs().CompactRows.encode_rows(rows)
    rng = np.random.default_rng(K)
    failures = []
    for form, align in COMPACT_COMBOS:
        what = f"compact K={K} form={form} align={align}"
        try:
            run_rows("compact", obj, ref, K, form, align, rng, what)
        except (AssertionError, _L().VidcError) as e:
            failures.append(f"{what}: {str(e).splitlines()[0]}")
    _raise_all(failures)


# ======================================================================================================================= lists
SIZES = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 4096, 4097, 5000, 0]  # 512 = CHUNK_IDS; total 16 973, odd
assert sum(SIZES) % 2 == 1
SHAPES = {
    "base": SIZES,  # first and last list empty
    "last1": SIZES + [1, 1],  # the last list has one id
    "first1": [1, 1] + SIZES,  # the first list is not empty, the last is
}
CODECS = ["roc", "ef", "wt", "packed13", "packed33"]


def shape_sizes(shape):
    if shape == "many":  # ~10 000 short lists in front of the lists above: ROC lane / row classes, Elias-Fano single-pass classes
        short = np.random.default_rng(5).integers(0, 40, 10000).tolist()
        sizes = short + SIZES
        return sizes if sum(sizes) % 2 == 1 else sizes + [1]
    return SHAPES[shape]


def _distinct(rng, universe, n):
    u = np.unique(rng.integers(0, universe, 2 * n + 16, dtype=np.uint64))
    while u.size < n:
        u = np.unique(np.concatenate([u, rng.integers(0, universe, 2 * n + 16, dtype=np.uint64)]))
    return rng.permutation(u)[:n]


def make_lists(codec, shape):
    sizes = np.asarray(shape_sizes(shape), np.uint64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    nlist, total = sizes.size, int(off[-1])
    rng = np.random.default_rng(CODECS.index(codec) * 10 + len(sizes))
    ids = np.zeros(total, np.uint64)
    wide = int(np.flatnonzero(sizes == 513)[0])
    if codec == "wt":  # a permutation of 0..ntotal-1, ascending inside every list
        ids = rng.permutation(total).astype(np.uint64)
        for l in range(nlist):
            ids[int(off[l]): int(off[l + 1])].sort()
        return off, ids
    for l in range(nlist):
        n = int(sizes[l])
        a = int(off[l])
        if codec == "roc":  # below 2^20 (one list: 27-bit ids), any order
            ids[a: a + n] = _distinct(rng, 1 << (27 if l == wide else 20), n)
        elif codec == "ef":  # ascending (one list is not: the encoder's retry path)
            v = np.sort(_distinct(rng, 1 << 30, n))
            ids[a: a + n] = rng.permutation(v) if l == wide else v
        else:  # packed: input order, repeats allowed
            ids[a: a + n] = rng.integers(0, 1 << int(codec[6:]), n, dtype=np.uint64)
    return off, ids


_LISTS = {}


def list_object(codec, shape, oracle):
    key = (codec, shape)
    if key not in _LISTS:
        cd = _codecs()
        off, ids = make_lists(codec, shape)
        kind = "packed" if codec.startswith("packed") else codec
        ref = cr.ListRef(kind, off, ids, oracle)
        if codec == "roc":
            obj = cd.RocLists.encode(off, ids)
        elif codec == "ef":
            obj = cd.EfLists.encode(off, ids)
        elif codec == "wt":
            obj = cd.WaveletTreeLists.build(off, ids)
        else:
            obj = cd.PackedLists.encode(off, ids, bits=int(codec[6:]))
        _LISTS[key] = (kind, obj, ref, off)
    return _LISTS[key]


def selection(off):
    """a repeat, empties, the first list, the last list and the longest list"""
    sizes = np.diff(off.astype(np.int64))
    nlist = sizes.size
    longest = int(np.argmax(sizes))
    empties = np.flatnonzero(sizes == 0)
    mid = int(np.flatnonzero(sizes == 513)[0])
    return np.array([longest, 0, nlist - 1, int(empties[0]), mid, longest, int(empties[-1]), mid + 1, mid - 1], np.uint64)


def run_decode_all(kind, obj, ref, misalign, what):
    lib = _L().lib()
    exp, _ = ref.expected(None)
    whole, view = cr.guarded(exp.size, np.uint64, "cuda", None, misalign)
    assert view.data_ptr() % 16 == 8 * misalign
    check(getattr(lib, f"vidc_{kind}_decode_all")(obj.ctx.h, obj.h, ptr(view)))
    _torch().cuda.synchronize()
    cr.assert_guards_intact(whole, view, what)
    cr.assert_view_equals(view, exp, what)


def run_decode_lists(kind, obj, ref, list_nos, misalign, what):
    lib = _L().lib()
    ln = np.ascontiguousarray(list_nos, dtype=np.uint64)
    exp, exp_off = ref.expected(ln)
    whole, view = cr.guarded(exp.size if ln.size else 4, np.uint64, "cuda", None, misalign)
    ow, ov = cr.guarded(ln.size + 1, np.uint64, "cpu")
    check(getattr(lib, f"vidc_{kind}_decode_lists")(obj.ctx.h, obj.h, ln.size, ptr(ln) if ln.size else None, ptr(view), ptr(ov)))
    _torch().cuda.synchronize()
    cr.assert_guards_intact(ow, ov, what + " out_offsets")
    cr.assert_view_equals(ov, exp_off, what + " out_offsets")
    if ln.size == 0:
        cr.assert_untouched(whole, view, what)  # m = 0: neither guards nor payload change
    else:
        cr.assert_guards_intact(whole, view, what)
        cr.assert_view_equals(view, exp, what)


def run_list_calls(codec, shape, oracle, tag=""):
    kind, obj, ref, off = list_object(codec, shape, oracle)
    nlist = off.size - 1
    for misalign in (0, 1):  # 16-byte aligned, and 8-byte but not 16-byte aligned
        what = f"{codec} {shape}{tag} align={8 * misalign}"
        run_decode_all(kind, obj, ref, misalign, what + " decode_all")
        run_decode_lists(kind, obj, ref, selection(off), misalign, what + " decode_lists(selection)")
        run_decode_lists(kind, obj, ref, np.arange(nlist), misalign, what + " decode_lists(every list)")
    run_decode_lists(kind, obj, ref, np.zeros(0, np.uint64), 0, f"{codec} {shape}{tag} decode_lists(m=0)")


@pytest.mark.parametrize("shape", ["base", "last1", "first1", "many"])
@pytest.mark.parametrize("codec", CODECS)
def test_lists_fill_their_region_and_nothing_else(codec, shape, monkeypatch, oracle):
    set_family(monkeypatch, "default")
    run_list_calls(codec, shape, oracle)


@pytest.mark.parametrize("shape", ["base", "many"])
@pytest.mark.parametrize("family", ["nolane", "lane", "general"])
def test_roc_lists_under_every_kernel_family(family, shape, monkeypatch, oracle):
    set_family(monkeypatch, family)
    run_list_calls("roc", shape, oracle, tag=f" family={family}")


@pytest.mark.parametrize("shape", ["base", "many"])
def test_roc_lists_with_poisoned_scratch(shape, monkeypatch, oracle):
    """the context's scratch blocks come filled with 0xFF (reads as -1 / all ones): a decoder that took its padding or its ids from
    scratch instead of writing them shows up against the reference"""
    set_family(monkeypatch, "default")
    kind, obj, ref, off = list_object("roc", shape, oracle)
    obj.ctx.set_pool_poison(True)
    try:
        run_list_calls("roc", shape, oracle, tag=" pool poison")
    finally:
        obj.ctx.set_pool_poison(False)


def test_roc_rows_with_poisoned_scratch(monkeypatch, oracle):
    """the ROC row decoders with 0xFF in every scratch block: the -1 padding must be written, not found"""
    cd = _codecs()
    K = 33
    rows = make_rows(K, big=False)
    ref = cr.RowRef("roc", rows, oracle)
    obj = cd.RocLists.encode_rows(rows)
    rng = np.random.default_rng(K)
    obj.ctx.set_pool_poison(True)
    try:
        for w, form, align, family in combos_for(K):
            set_family(monkeypatch, family)
            run_rows("roc", obj, ref, w, form, align, rng, f"roc (pool poison) K={K} width={w} form={form} align={align} family={family}")
    finally:
        obj.ctx.set_pool_poison(False)


# ============================================================================================================== picked results
def make_items(off, n, rng):
    """n (list, offset) pairs over the non-empty lists, the first and last id of the longest list among them"""
    sizes = np.diff(off.astype(np.int64))
    ne = np.flatnonzero(sizes)
    l = rng.choice(ne, n)
    o = rng.integers(0, sizes[l])
    longest = int(np.argmax(sizes))
    l[0], o[0] = longest, 0
    l[-1], o[-1] = longest, sizes[longest] - 1
    return l.astype(np.uint64), o.astype(np.uint64)


@pytest.mark.parametrize("shape", ["base", "many"])
@pytest.mark.parametrize("codec", CODECS)
def test_decode_gather_writes_n_items_and_nothing_else(codec, shape, monkeypatch, oracle):
    set_family(monkeypatch, "default")
    kind, obj, ref, off = list_object(codec, shape, oracle)
    fn = getattr(_L().lib(), f"vidc_{kind}_decode_gather")
    rng = np.random.default_rng(17)
    for n in (1, 7, 1000):
        l, o = make_items(off, max(n, 2), rng)
        l, o = np.ascontiguousarray(l[-n:]), np.ascontiguousarray(o[-n:])
        touched, slot = np.unique(l, return_inverse=True)
        touched, slot = np.ascontiguousarray(touched, np.uint64), np.ascontiguousarray(slot.reshape(-1), np.uint64)
        want = np.array([ref.item(a, b) for a, b in zip(l, o)], np.uint64)
        whole, view = cr.guarded(n, np.int64, "cpu", None, n % 2)
        check(fn(obj.ctx.h, obj.h, touched.size, ptr(touched), n, ptr(slot), ptr(o), ptr(view)))
        cr.assert_guards_intact(whole, view, f"{codec} {shape} decode_gather n={n}")
        cr.assert_view_equals(view, want, f"{codec} {shape} decode_gather n={n}")
    # n_items = 0: nothing is touched, with and without touched lists
    whole, view = cr.guarded(4, np.int64, "cpu")
    touched = np.array([1, 2], np.uint64)
    check(fn(obj.ctx.h, obj.h, 2, ptr(touched), 0, None, None, ptr(view)))
    check(fn(obj.ctx.h, obj.h, 0, None, 0, None, None, ptr(view)))
    cr.assert_untouched(whole, view, f"{codec} {shape} decode_gather n_items=0")


@pytest.mark.parametrize("codec", ["packed13", "packed33", "ef", "wt"])
def test_random_access_writes_m_ids_and_nothing_else(codec, oracle):
    """vidc_packed_get, vidc_ef_get, vidc_wt_select"""
    kind, obj, ref, off = list_object(codec, "base", oracle)
    fn = getattr(_L().lib(), "vidc_wt_select" if kind == "wt" else f"vidc_{kind}_get")
    rng = np.random.default_rng(23)
    for m in (1, 2, 513):
        l, o = make_items(off, max(m, 2), rng)
        l, o = np.ascontiguousarray(l[-m:]), np.ascontiguousarray(o[-m:])
        want = np.array([ref.item(a, b) for a, b in zip(l, o)], np.uint64)
        whole, view = cr.guarded(m, np.int64, "cpu", None, m % 2)
        check(fn(obj.ctx.h, obj.h, m, ptr(l), ptr(o), ptr(view)))
        cr.assert_guards_intact(whole, view, f"{codec} get m={m}")
        cr.assert_view_equals(view, want, f"{codec} get m={m}")
    whole, view = cr.guarded(4, np.int64, "cpu")
    check(fn(obj.ctx.h, obj.h, 0, None, None, ptr(view)))
    cr.assert_untouched(whole, view, f"{codec} get m=0")


def make_labels(off, n, rng):
    """valid labels (repeats included) mixed with -1, other negatives, list >= nlist, offset >= size, labels into empty lists"""
    sizes = np.diff(off.astype(np.int64))
    nlist = sizes.size
    l, o = make_items(off, max(n, 2), rng)
    l, o = l[:n].astype(np.int64), o[:n].astype(np.int64)
    lab = (l << 32) | o
    kind = rng.integers(0, 100, n)
    lab[kind < 8] = -1
    lab[(kind >= 8) & (kind < 10)] = -rng.integers(2, 1 << 62, int(((kind >= 8) & (kind < 10)).sum()))
    sel = (kind >= 10) & (kind < 13)
    lab[sel] = ((nlist + rng.integers(0, 1000, int(sel.sum()))) << 32) | rng.integers(0, 4, int(sel.sum()))
    sel = (kind >= 13) & (kind < 16)
    lab[sel] = (l[sel] << 32) | (sizes[l[sel]] + rng.integers(0, 3, int(sel.sum())))
    sel = (kind >= 16) & (kind < 18)
    lab[sel] = rng.choice(np.flatnonzero(sizes == 0), int(sel.sum())).astype(np.int64) << 32
    if n > 4:
        lab[n // 2] = lab[n // 4]
    return lab


def expect_labels(lab, off, ref):
    sizes = np.diff(off.astype(np.int64))
    out = np.full(lab.size, -1, np.int64)
    bad = 0
    for i, v in enumerate(lab.tolist()):
        if v < 0:
            continue
        l, o = v >> 32, v & 0xFFFFFFFF
        if l >= sizes.size or o >= sizes[l]:
            bad += 1
        else:
            out[i] = ref.item(l, o)
    return out, bad


@pytest.mark.parametrize("shape", ["base", "many"])
@pytest.mark.parametrize("codec", CODECS)
def test_translate_labels_writes_n_ids_and_nothing_else(codec, shape, monkeypatch, oracle):
    torch = _torch()
    set_family(monkeypatch, "default")
    kind, obj, ref, off = list_object(codec, shape, oracle)
    fn = getattr(_L().lib(), f"vidc_{kind}_translate_labels_dev")
    rng = np.random.default_rng(29)
    for n in (1, 63, 4097):
        lab = make_labels(off, n, rng)
        want, bad = expect_labels(lab, off, ref)
        for in_place in (False, True):
            what = f"{codec} {shape} translate_labels n={n} in_place={in_place}"
            whole, view = cr.guarded(n, np.int64, "cuda", None, n % 2)
            iw, iv = cr.guarded(1, np.uint64, "cuda")
            iv.zero_()
            if in_place:
                view.copy_(dev_i64(lab))
                d_lab = view
            else:
                d_lab = dev_i64(lab)
            check(fn(obj.ctx.h, obj.h, n, ptr(d_lab), ptr(view), ptr(iv)))
            torch.cuda.synchronize()
            cr.assert_guards_intact(whole, view, what)
            cr.assert_view_equals(view, want, what)
            cr.assert_guards_intact(iw, iv, what + " d_invalid")
            cr.assert_view_equals(iv, np.array([bad], np.uint64), what + " d_invalid")
            if not in_place:
                assert np.array_equal(d_lab.cpu().numpy(), lab), what + ": the labels were modified"
    # n = 0: nothing is touched
    whole, view = cr.guarded(4, np.int64, "cuda")
    iw, iv = cr.guarded(1, np.uint64, "cuda")
    check(fn(obj.ctx.h, obj.h, 0, None, ptr(view), ptr(iv)))
    check(fn(obj.ctx.h, obj.h, 0, ptr(view), ptr(view), ptr(iv)))
    torch.cuda.synchronize()
    cr.assert_untouched(whole, view, f"{codec} {shape} translate_labels n=0")
    cr.assert_untouched(iw, iv, f"{codec} {shape} translate_labels n=0 d_invalid")


def test_rows_of_an_empty_request_touch_nothing():
    """m = 0 on the six row entry points: VIDC_OK, nothing written"""
    cd = _codecs()
    lib = _L().lib()
    rng = np.random.default_rng(0)
    rows = np.full((200, 16), -1, np.int32)
    for i in range(200):
        d = int(rng.integers(0, 17))
        rows[i, :d] = rng.choice(200, d, replace=False)
    whole, view = cr.guarded((4, 16), np.int32, "cuda")
    cw, cv = cr.guarded(4, np.uint32, "cuda")
    hw, hv = cr.guarded(4, np.uint32, "cpu")
    iw, iv = cr.guarded(1, np.uint64, "cuda")
    for kind, cls in (("ef", cd.EfLists), ("roc", cd.RocLists), ("compact", cd.CompactRows)):
        obj = cls.encode_rows(rows)
        k = () if kind == "compact" else (16,)
        host = {"compact": lib.vidc_compact_rows_decode, "ef": lib.vidc_ef_decode_rows, "roc": lib.vidc_roc_decode_rows}[kind]
        dev = {"compact": lib.vidc_compact_rows_decode_dev, "ef": lib.vidc_ef_decode_rows_dev, "roc": lib.vidc_roc_decode_rows_dev}[kind]
        check(host(obj.ctx.h, obj.h, 0, None, *k, ptr(view), ptr(hv)))
        check(dev(obj.ctx.h, obj.h, 0, None, *k, ptr(view), ptr(cv), ptr(iv)))
    _torch().cuda.synchronize()
    for w, v, what in ((whole, view, "rows"), (cw, cv, "d_counts"), (hw, hv, "counts"), (iw, iv, "d_invalid")):
        cr.assert_untouched(w, v, "m=0 " + what)
