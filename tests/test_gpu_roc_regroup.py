"""vidc_roc_regroup / codecs.roc_regroup on the GPU (include/vidc.h, ROC section): a new object made of whole lists of other objects, without encoding.

Sources: A and B, family F of tests/test_gpu_shards.py cut in two (lists 0 .. 11 and 12 .. 36; B holds the 3000-id list), W (sizes 3000 /
0 / 1 / 1500 / 2 / 6000, distinct ids below 2^31: a one-id list lives in its head alone; at 31 bits the 3000-id stream is 1958 words and
the 1500-id one 1025 -- ROC saves log2(n!) bits -- so each crosses one seam of the copy's 1024-word chunks, and the sixth list is there
because only its stream, 6000 ids, is longer than 2048 words and crosses several) and D (a duplicate-heavy list, where the reference
codec is lossy).  Everything the new object exports -- words, the five per-list arrays, offsets, permutation -- and everything it decodes is compared with the numpy gather of what the sources
export and decode.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_shards import csr, dev
from test_shards_cpu import F_SIZES

pytestmark = pytest.mark.gpu

W_SIZES = [3000, 0, 1, 1500, 2, 6000]
KEYS = ("sizes", "precision", "heads", "nwords", "mt_draws")


def _torch():
    import torch

    return torch


def _roc():
    from vector_db_id_compression_amd.codecs import RocLists

    return RocLists


def regroup(*args, **kw):
    from vector_db_id_compression_amd.codecs import roc_regroup

    return roc_regroup(*args, **kw)


def export(r):
    """everything a source exports and decodes, once: info, per-list word slices, per-list decoded ids, per-list nonclean flags"""
    info = r.info()
    woff = np.concatenate([[0], np.cumsum(info["nwords"], dtype=np.int64)])
    off = np.concatenate([[0], np.cumsum(info["sizes"], dtype=np.int64)])
    words, dec = r.all_words(), r.decode_all().cpu().numpy()
    return dict(info=info, woff=woff, off=off, words=[words[woff[l]: woff[l + 1]] for l in range(r.nlist)],
                dec=[dec[off[l]: off[l + 1]] for l in range(r.nlist)])


@pytest.fixture(scope="module")
def sources():
    _torch().cuda.set_device(0)
    R = _roc()
    off, ids = csr(F_SIZES)
    cut = int(off[12])
    a = R.encode(off[:13].copy(), dev(ids[:cut]), want_perm=True)
    b = R.encode((off[12:] - off[12]).astype(np.uint64), dev(ids[cut:]))
    woff = np.concatenate([[0], np.cumsum(W_SIZES)]).astype(np.uint64)
    wids = np.random.default_rng(41).choice(2 ** 31 - 1, int(woff[-1]), replace=False).astype(np.uint64)
    w = R.encode(woff, dev(wids))
    dup = np.concatenate([np.repeat(np.array([5, 5000], np.uint64), 100), np.array([3, 1, 4, 1, 5], np.uint64)])
    d = R.encode(np.array([0, 200, 205], np.uint64), dev(dup))
    objs = dict(A=a, B=b, W=w, D=d)
    yield objs, {k: export(v) for k, v in objs.items()}


def gathered(exports, names, src_no, list_no):
    """the numpy gather of the sources' exports: what the regrouped object must export and decode"""
    rows = [(exports[names[s]], int(l)) for s, l in zip(src_no, list_no)]
    info = {k: np.array([e["info"][k][l] for e, l in rows], dtype=exports[names[0]]["info"][k].dtype) for k in KEYS}
    words = np.concatenate([e["words"][l] for e, l in rows] + [np.zeros(0, np.uint32)])
    dec = [e["dec"][l] for e, l in rows]
    return info, words, dec


def check_regroup(sources, names, src_no, list_no, want_perm=True):
    objs, exports = sources
    src_no, list_no = np.asarray(src_no, np.uint32), np.asarray(list_no, np.uint64)
    ctx = next(objs[n] for n in names if n).ctx
    before = ctx.d2h_bytes()
    g = regroup([objs[n] if n else None for n in names], src_no, list_no, want_perm=want_perm)
    assert ctx.d2h_bytes() - before <= 8, "only the word total is read back"
    ref = next(n for n in names if n)
    info, words, dec = gathered(exports, [n or ref for n in names], src_no, list_no)
    m = src_no.size
    assert g.nlist == m and g.ntotal == int(info["sizes"].sum()) and g.total_words == int(info["nwords"].sum()) == words.size
    assert g.compressed_bytes == 8 * int((info["sizes"] > 0).sum()) + 4 * words.size
    got = g.info()
    for k in KEYS:
        assert np.array_equal(got[k], info[k]), k
    assert np.array_equal(g.all_words(), words), "stack words"
    off = np.concatenate([[0], np.cumsum(info["sizes"], dtype=np.uint64)]).astype(np.uint64)
    assert np.array_equal(g.offsets, off)
    if want_perm:
        assert np.array_equal(g.perm(), np.concatenate([np.arange(n) for n in info["sizes"]] + [np.zeros(0, np.int64)]))
    else:
        from vector_db_id_compression_amd._lib import VidcError

        with pytest.raises(VidcError):
            g.perm()
    want_all = np.concatenate(dec + [np.zeros(0, np.int64)])
    assert np.array_equal(g.decode_all().cpu().numpy(), want_all), "decode_all"
    nonclean_all = g.last_decode_nonclean
    # the sources' own count over the same lists (one decode_lists per source; a repeated list counts per mention)
    want_nonclean = 0
    for s, n in enumerate(names):
        mine = list_no[src_no == s]
        if n and mine.size:
            objs[n].decode_lists(mine)
            want_nonclean += objs[n].last_decode_nonclean
    assert nonclean_all == want_nonclean, "last_decode_nonclean"
    if m:
        req = np.random.default_rng(m).integers(0, m, min(m, 40))
        ids, ro = g.decode_lists(req)
        assert np.array_equal(ids.cpu().numpy(), np.concatenate([dec[j] for j in req] + [np.zeros(0, np.int64)])), "decode_lists"
        assert np.array_equal(ro, np.concatenate([[0], np.cumsum(info["sizes"][req], dtype=np.uint64)]).astype(np.uint64))
    return g, info


def big_table(exports):
    """600 rows over A, B and W in a seeded order -- more than one block of the metadata kernel, every list at least once, repeats"""
    rng = np.random.default_rng(43)
    names = ["A", "B", "W"]
    every = [(s, l) for s, n in enumerate(names) for l in range(len(exports[n]["words"]))]
    extra = [every[i] for i in rng.integers(0, len(every), 600 - len(every))]
    rows = [every[i] for i in rng.permutation(len(every))] + extra
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return names, np.array([r[0] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint64)


def test_the_sources_are_what_the_cases_count_on(sources):
    _, ex = sources
    w = ex["W"]["info"]
    assert int(w["nwords"].max()) > 2048, "a stream of W crosses two seams of the copy's 1024-word chunks"
    assert ((w["sizes"] > 0) & (w["nwords"] == 0)).any(), "a non-empty list that lives in its head alone"
    assert (w["sizes"] == 0).any() and (ex["A"]["info"]["sizes"] == 0).any() and (ex["B"]["info"]["sizes"] == 0).any()
    assert ex["D"]["info"]["sizes"].tolist() == [200, 5]


@pytest.mark.parametrize("hook", [None, "VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
def test_an_arbitrary_order_with_repeats_over_three_sources(sources, monkeypatch, hook):
    """both copy paths run: a list takes 16-byte accesses iff its word offsets in source and destination agree mod 4 (the word arrays
    are blocks of the contexts' caches, 16-byte aligned); the hooks send the hint-less object to the other decoder families"""
    for h in ("VIDC_FORCE_GENERAL", "VIDC_NO_LANE"):
        monkeypatch.delenv(h, raising=False)
    _, ex = sources
    names, src_no, list_no = big_table(ex)
    # the references were decoded without a hook; the regrouped object decodes under it
    if hook:
        monkeypatch.setenv(hook, "1")
    g, info = check_regroup(sources, names, src_no, list_no)
    assert src_no.size == 600 > 256 and g.nlist == 600
    dst_woff = np.concatenate([[0], np.cumsum(info["nwords"], dtype=np.int64)])[:-1]
    src_woff = np.array([ex[names[s]]["woff"][int(l)] for s, l in zip(src_no, list_no)])
    has_words = info["nwords"] > 0
    agree = ((src_woff - dst_woff) % 4 == 0) & has_words
    assert agree.any() and (~agree & has_words).any(), "both the 16-byte path and the word path must run"
    assert (agree & (dst_woff % 4 != 0) & (info["nwords"] > 4)).any(), "a 16-byte run behind a head of one to three words"
    assert (info["nwords"] > 2048).sum() >= 2, "the longest stream of W, more than once"
    assert ((info["nwords"] > 1024) & (info["nwords"] <= 2048)).any(), "a stream that crosses exactly one seam"


def test_a_null_source_that_no_row_names(sources):
    g, _ = check_regroup(sources, ["A", None, "W"], [2, 0, 2, 0, 2, 2], [3, 11, 0, 5, 1, 2], want_perm=False)
    assert g.nlist == 6


def test_selections_of_empty_lists_only(sources):
    _, ex = sources
    empties = [(s, l) for s, n in enumerate(["A", "B", "W"]) for l in np.flatnonzero(ex[n]["info"]["sizes"] == 0)]
    assert len(empties) >= 4
    g, _ = check_regroup(sources, ["A", "B", "W"], [e[0] for e in empties] * 2, [e[1] for e in empties] * 2)
    assert g.ntotal == 0 and g.total_words == 0 and g.compressed_bytes == 0
    ids, off = g.decode_lists([0, 1])
    assert ids.numel() == 0 and off.tolist() == [0, 0, 0]


@pytest.mark.parametrize("row", [("W", 0), ("W", 2), ("W", 1), ("W", 5), ("B", 2)])
def test_one_list(sources, row):
    g, info = check_regroup(sources, [row[0]], [0], [row[1]])
    assert g.nlist == 1


def test_no_list_is_an_object_without_lists(sources):
    """m == 0 is what vidc_roc_import makes of nlist == 0: VIDC_OK and an empty object"""
    objs, _ = sources
    g = regroup([objs["A"]], [], [], want_perm=True)
    assert g.nlist == 0 and g.ntotal == 0 and g.total_words == 0 and g.compressed_bytes == 0
    assert g.decode_all().numel() == 0
    imp = _roc().from_streams(np.zeros(1, np.uint64), [], [], [], [])
    assert imp.nlist == 0 and imp.ntotal == 0


def test_a_duplicate_heavy_list_keeps_its_stream(sources):
    """the reference codec is lossy for duplicates: what the list decodes to encodes to another stream, and the regroup must not
    replace the one with the other"""
    objs, ex = sources
    g, info = check_regroup(sources, ["D", "W"], [0, 1, 0], [0, 3, 1])
    d = ex["D"]
    fresh = _roc().encode(np.array([0, 200], np.uint64), dev(d["dec"][0].view(np.uint64)))
    fi = fresh.info()
    same = all(fi[k][0] == d["info"][k][0] for k in KEYS) and np.array_equal(fresh.all_words(), d["words"][0])
    assert not same, "the duplicate-heavy list re-encodes to its own stream: the case shows nothing"
    assert np.array_equal(g.words(0), d["words"][0]) and int(g.info()["heads"][0]) == int(d["info"]["heads"][0])


def test_a_regrouped_object_is_a_source_like_any_other(sources):
    objs, ex = sources
    g1 = regroup([objs["B"], objs["W"]], [1, 0, 0, 1], [0, 2, 20, 3])
    g2 = regroup([g1, objs["A"]], [0, 1, 0, 0], [3, 4, 0, 1], want_perm=True)
    want = [ex["W"]["dec"][3], ex["A"]["dec"][4], ex["W"]["dec"][0], ex["B"]["dec"][2]]
    assert np.array_equal(g2.decode_all().cpu().numpy(), np.concatenate(want))
    assert np.array_equal(g2.all_words(), np.concatenate([ex["W"]["words"][3], ex["A"]["words"][4], ex["W"]["words"][0], ex["B"]["words"][2]]))


def test_refused_calls_leave_no_object(sources):
    from vector_db_id_compression_amd import _lib

    objs, _ = sources
    L = _lib.lib()
    arr = (ctypes.c_void_p * 2)(objs["A"].h, objs["W"].h)

    def call(nsrc, sn, ln):
        sn, ln = np.asarray(sn, np.uint32), np.asarray(ln, np.uint64)
        out = ctypes.c_void_p(1)
        st = L.vidc_roc_regroup(objs["A"].ctx.h, nsrc, arr, sn.size, _lib.ptr(sn), _lib.ptr(ln), 0, ctypes.byref(out))
        assert out.value is None
        return st

    assert call(2, [0, 1], [12, 0]) == -1 and b"names list 12 of source 0, which holds 12" in L.vidc_last_error()
    assert call(2, [0, 2], [0, 0]) == -1 and b"names source 2 of 2" in L.vidc_last_error()
    assert call(9, [0], [0]) == -1
    rows = _torch().full((4, 8), -1, dtype=_torch().int32, device="cuda")
    rows[:, 0] = _torch().arange(4, dtype=_torch().int32)
    graph = _roc().encode_rows(rows)
    arr[1] = graph.h
    assert call(2, [0], [0]) == -6 and b"graph" in L.vidc_last_error()
