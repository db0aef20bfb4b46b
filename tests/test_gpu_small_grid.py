"""Grid-stride loops past their first trip: every operation on a context whose grids are sized for ONE compute unit.

Almost every kernel walks its work in a grid-stride loop whose grid is capped at ctx->num_cu * K workgroups.  On the 256 CUs of an
MI355X the shapes of the other GPU tests never send a wavefront through such a loop twice.  A context created under VIDC_NUM_CU=1
(include/vidc.h: vidc_ctx_num_cu) sizes the same grids for one CU, so a few ten thousand ids give three trips and more.  Its pool
poison is on: output that a skipped trip never wrote reads back as 0xFF, not as a lucky zero.

Every case is compared twice: exactly against the reference the other tests use for the operation (the CPU oracle for ROC heads,
words, precisions and decode order; lists_ref, rows_ref, append_ref, remove_ref, locate_ref, rows_update_ref, rebalance_ref,
roc_seg_ref), and word for word against the same call on the default context -- at these sizes still single-trip --, which pins that
the host plans' use of num_cu (promote_r2, ef_chunk_form, the wavelet plans) never changes a bit.

CAPACITY is what ONE trip of a capped loop covers at one CU, re-derived from the launch sites; OFFERS says, per shape, how many items
it gives each family.  tests/test_small_grid_shapes_cpu.py asserts without a GPU that every shape offers each family it names more than
two trips and a ragged last one: that condition, not a measurement, is what keeps these tests from passing with single-trip loops.

No case fell back to the default-context comparison alone: the numpy / oracle models of every shape run in a few seconds.  Out of
scope: loops whose cap is a constant, not num_cu.
"""
import numpy as np
import pytest

import append_ref as ar
import contract_ref as cr
import lists_ref as lr
import locate_ref
import remove_ref
import image_ref
import roc_seg_ref as sr
import rows_ref as rr
import rows_update_ref as ru
import wt_ref

pytestmark = pytest.mark.gpu

#: family -> (items one trip covers at num_cu == 1, items of the smallest unit that can be left partly filled: a wavefront of a
#: thread-per-item kernel, a workgroup of a wavefront-per-item kernel), with the launch sites the figure comes from
CAPACITY = {
    # requests.h req_grid: 32 workgroups x 256 threads, an item each -- translate_labels of every codec, k_loc_labels, k_app_keys /
    # bounds / place, k_rm_*, k_rows_upd_slots, k_req_nodes_sanitize / fixup, k_rocseg_labels / add_base / compose_perm /
    # inner_offsets / max; ef.hip k_iota_perm has the same geometry
    "req": (32 * 256, 64),
    # roc_seg.hip chunk_grid (k_rocseg_count / scatter / fix), append.h app_chunk_grid (k_app_copy, k_app_labels_perm, k_rm_mark,
    # k_rm_compact, k_loc_mark; the ROC splice's k_roc_regroup_copy / perm), shards.hip copy_grid: 16 workgroups x 4 wavefronts, a chunk
    # of <= 1024 elements of one list each
    "chunk1024": (16 * 4, 4),
    # append.h app_sort_phase (k_app_hist, k_app_scatter): 32 workgroups of one wavefront, a tile of 1024 pairs each
    "sort_tile": (32, 1),
    # chunks.h k_fill_items (64 workgroups, a list each), k_ef_decode / k_ef_hrank_from_high / k_rows_to_ids / k_compact_rows encode and
    # update (64 workgroups of one wavefront, a list or row each)
    "wave_per_list": (64, 1),
    # chunks.h k_fill_items_flat, rows_csr.h k_rows_count, ef.hip k_ef_arena_geom: 16 workgroups x 256 threads, a list or row each
    "flat_lists": (16 * 256, 64),
    # packed.hip k_packed_encode / decode / decode_lists, ef.hip host-offset chunk forms and cgrid: 256 workgroups of one wavefront, a
    # chunk of <= 512 ids (CHUNK_IDS) of one list each; k_ef_decode_rec: 256 workgroups, a batch each
    "chunk512": (256, 1),
    # ef_plan.h ef_chunk_form with device offsets (EF_FORM_DEV): 32 workgroups of one wavefront, a chunk each
    "chunk512_dev": (32, 1),
    # rows_tile.h tile_grid: min(16, 150 KiB / LDS bytes of a tile) resident tiles of 64 rows (Elias-Fano arena rows, compact rows).  16
    # at K = 16: a compact tile takes (64 * (stride / 4 | 1) + 1) * 4 = 1796 bytes (the CPU shape test derives it), an Elias-Fano tile
    # (64 * (record words | 1) + 1) * 8 + 4864 bytes, under 9600 for records of up to 8 words
    "rows_tile": (16 * 64, 64),
    # packed.hip k_compact_check_rows (import): 64 workgroups x 4 rows; k_compact_rows_decode (rows whose stride is no multiple of four
    # bytes): 256 workgroups x 4 rows; k_compact_rows_decode_wide (K > 64): 256 workgroups, a row each
    "compact_check": (64 * 4, 4),
    "compact_rows4": (256 * 4, 4),
    "compact_wide": (256, 1),
    # roc.hip finish_complete: k_roc_compact_groups (64 workgroups x 64 lists), k_roc_compact_waves (8 workgroups x 16 lists),
    # k_roc_compact (16 workgroups, a list each), k_roc_rows_compact (max(64, occupancy / 64 * 64) tiles of 64 rows: 64, a CU holds
    # at most 32 wavefronts); enc_prepass k_roc_prepass (32 workgroups, a list each; only under VIDC_FULL_PREPASS=1)
    "roc_groups": (64 * 64, 64),
    "roc_waves": (8 * 16, 16),
    "roc_lists": (16, 1),
    "roc_rows": (64 * 64, 64),
    "roc_prepass": (32, 1),
    # wt_plan.h: k_wt_check_syms (32 workgroups x 256 ids), k_wt_scatter_syms (32 x 4096 ids; below 2^18 ids or under VIDC_WT_SCATTER),
    # k_wt_imp_check_blocks (wt_type 1: 8 workgroups x 256 blocks of 63 positions), k_rrr_classes / k_rrr_offsets (wt_type 1 build) and
    # k_rrr_expand (wt_type 1 decode_all): 32 workgroups x 256 blocks of 63 positions
    "wt_rrr_blocks": (32 * 256 * 63, 63),
    "wt_check": (32 * 256, 64),
    "wt_scatter": (32 * 4096, 4096),
    "wt_imp_blocks": (8 * 256 * 63, 63),
}

HOOKS = ("VIDC_FORCE_GENERAL", "VIDC_NO_LANE", "VIDC_FULL_PREPASS")
KEYS = ("sizes", "precision", "heads", "nwords", "mt_draws")
BITS = 28      # packed width of the list shapes: every id, batch ids included, lies below 2^28
SEG_T, SEG_B = 16, 16


# ---------------------------------------------------------------------------------------------------------------- shapes (numpy only)
def spread(k):
    """k -> 6 k + 3: distinct stays distinct, ascending stays ascending, nothing is a power of two (the ids ROC round-trips)"""
    return (6 * np.asarray(k, dtype=np.uint64) + 3).astype(np.uint64)


def csr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


def ascending_lists(rng, sizes, kbits):
    """per list n distinct ascending ids 6 k + 3, k < 2^kbits"""
    out = []
    for n in sizes:
        n = int(n)
        u = np.unique(rng.integers(0, 1 << kbits, 2 * n + 16, dtype=np.uint64))
        assert u.size >= n
        out.append(spread(np.sort(rng.permutation(u)[:n])))
    return out


def chunks_of(sizes, unit):
    sizes = np.asarray(sizes, dtype=np.int64)
    return int(((sizes + unit - 1) // unit).sum())


_SHAPES = {}


def shape(name):
    """-> dict(off, ids, lists, sizes, offers): built once, never changed"""
    if name not in _SHAPES:
        _SHAPES[name] = _BUILDERS[name]()
    return _SHAPES[name]


def _lists_shape(lists, offers):
    sizes = np.array([len(l) for l in lists], dtype=np.int64)
    ids = np.concatenate(lists + [np.zeros(0, np.uint64)]).astype(np.uint64)
    return dict(off=csr(sizes), ids=ids, lists=lists, sizes=sizes, offers=offers)


def _short():
    """17 001 lists of 0 .. 9 ids: the per-list loops (k_app_bounds, k_rm_new_off, k_fill_items_flat), the ROC compaction of tiny lists"""
    rng = np.random.default_rng(1701)
    sizes = rng.integers(0, 10, 17001)
    sizes[::97] = 0
    sizes[-1] = 9
    for i in range(1, 9):  # (a last trip of the wavefront-per-chunk kernels that ends inside a workgroup)
        if int((sizes > 0).sum()) % 4:
            break
        sizes[i] = 0
    s = _lists_shape(ascending_lists(rng, sizes, 22), {})
    nonempty = int((sizes > 0).sum())
    s["offers"] = {"req": sizes.size + 1, "flat_lists": sizes.size, "roc_groups": sizes.size, "wave_per_list": sizes.size,
                   "chunk512": nonempty, "chunk1024": nonempty, "chunk512_dev": nonempty}
    return s


def _mid():
    """300 lists of 17 .. 256 ids below 2^30: 64 .. 200 stream words per list on average, the wavefront-per-four-lists compaction"""
    rng = np.random.default_rng(300)
    sizes = rng.integers(17, 257, 300)
    sizes[:4] = [17, 256, 64, 65]
    return _lists_shape(ascending_lists(rng, sizes, 27), {"roc_waves": 300})


def _long():
    """40 lists of 300 .. 2000 ids: the list-per-workgroup compaction; four lists at least half as long as the longest, so at one CU
    promote_r2 (cap = 4) takes its n_long <= cap branch"""
    rng = np.random.default_rng(40)
    sizes = np.concatenate([[2000, 1500, 1100, 1001], rng.integers(300, 1000, 36)])
    sizes = sizes[rng.permutation(sizes.size)]
    return _lists_shape(ascending_lists(rng, sizes, 27), {"roc_lists": 40})


def _mixed():
    """the three ROC classes in one call, interleaved (9000 of the short lists): every kernel family of the encoder and the decoder"""
    rng = np.random.default_rng(9340)
    lists = shape("short")["lists"][:9000] + shape("mid")["lists"] + shape("long")["lists"]
    lists = [lists[i] for i in rng.permutation(len(lists))]
    return _lists_shape(lists, {"roc_groups": len(lists), "roc_prepass": len(lists), "req": sum(len(l) for l in lists)})


def _many_long():
    """7 lists of 33 000 .. 40 000 ids, all at least half as long as the longest: n_long > cap = 4 at one CU, promote_r2 takes its
    other branch (the six longest to the position-bitmap chains, one stays on the general kernel)"""
    rng = np.random.default_rng(7)
    sizes = rng.integers(33000, 40001, 7)
    return _lists_shape(ascending_lists(rng, sizes, 24), {})


def _chunky():
    """600 lists of 0 .. 5000 ids, about 130 000 ids: the chunk kernels of every family, with empty lists between working ones"""
    rng = np.random.default_rng(600)
    sizes = rng.integers(1, 400, 600)
    sizes[::29] = 0
    sizes[[3, 50, 111, 200, 333, 401, 480, 555, 599]] = [512, 513, 1023, 1024, 1025, 2049, 4097, 5000, 700]
    s = _lists_shape(ascending_lists(rng, sizes, 24), {})
    c512, c1024 = chunks_of(sizes, 512), chunks_of(sizes, 1024)
    s["offers"] = {"chunk512": c512, "chunk512_dev": c512, "chunk1024": c1024, "wave_per_list": sizes.size, "req": int(sizes.sum())}
    return s


def _full():
    """280 lists of 520 .. 600 ids: two chunks each that hold more than 256 ids on average (the full-chunk Elias-Fano form)"""
    rng = np.random.default_rng(280)
    sizes = rng.integers(520, 601, 281)
    s = _lists_shape(ascending_lists(rng, sizes, 24), {})
    s["offers"] = {"chunk512": chunks_of(sizes, 512)}
    return s


def _perm_lists(ntotal=300_001, nlist=600):
    """a permutation of 0 .. ntotal - 1, ascending inside each list (what a wavelet tree holds); lists 0, 7, 14, ... are empty.  300 001
    ids in 600 lists; 1 100 003 ids in 100 lists for the block passes of the RRR coding"""
    rng = np.random.default_rng(ntotal // 100)
    lst = rng.choice(np.array([l for l in range(nlist) if l % 7]), ntotal)
    ids = np.argsort(lst, kind="stable").astype(np.uint64)
    sizes = np.bincount(lst, minlength=nlist).astype(np.int64)
    off = csr(sizes)
    lists = [ids[int(off[l]):int(off[l + 1])] for l in range(nlist)]
    offers = {"wt_check": ntotal, "wt_scatter": ntotal, "wt_imp_blocks": ntotal, "req": ntotal}
    if ntotal > 1 << 20:
        offers = {"wt_rrr_blocks": ntotal, "wt_check": ntotal, "wt_imp_blocks": ntotal}
    return dict(off=off, ids=ids, lists=lists, sizes=sizes, sym=lst, offers=offers)


def _seg():
    """segmented ROC at T = 16, B = 16: 17 lists of 8193 ids (k = 10: 1024 segments, nine chunks, the last of one id), three of
    2000 ids (k = 7), 30 lists that are not split (k = 0: the early `continue` of both multisplit passes) and 5 empty ones, interleaved;
    every second list shuffled"""
    rng = np.random.default_rng(16)
    sizes = [8193] * 17 + [2000] * 3 + list(rng.integers(1, 17, 30)) + [0] * 5
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    lists = []
    for i, n in enumerate(sizes):
        li = np.sort(rng.choice(1 << SEG_B, int(n), replace=False)).astype(np.uint64)
        lists.append(rng.permutation(li) if i % 2 else li)
    s = _lists_shape(lists, {})
    k = np.array([sr.seg_k(int(n), SEG_T, SEG_B) for n in s["sizes"]])
    s["offers"] = {"chunk1024": chunks_of(s["sizes"], 1024), "req": int((1 << k).sum()) + 1}
    return s


ROWS_N, ROWS_K, ROWS_M, ROWS_GROW = 9001, 16, 20001, 130
#: K = 16: the tile kernels of compact rows and of the Elias-Fano arena, ROC's row kernels; K = 80 (> 64): Elias-Fano and ROC rows become
#: CSR lists (rows_csr.h), compact rows take the row-per-wavefront kernels; K = 7: compact rows of 13 bytes, no multiple of four
ROWS_SHAPES = {"rows": 16, "rows_wide": 80, "rows_k7": 7}


def _rows(K=ROWS_K):
    """a graph of 9001 nodes; a request of 20 001 nodes (every node, repeats, negative nodes, nodes beyond the graph); an update batch of
    20 001 rows that also adds 130 nodes"""
    rows = rr.family("uniform", ROWS_N, K, seed=11)
    rng = np.random.default_rng(9001)
    nodes = np.concatenate([rng.permutation(ROWS_N), rng.integers(0, ROWS_N, ROWS_M - ROWS_N)]).astype(np.int64)
    r = rng.random(ROWS_M)
    nodes[r < 0.05] = -1 - rng.integers(0, 5, int((r < 0.05).sum()))
    nodes[(r >= 0.05) & (r < 0.1)] = ROWS_N + rng.integers(0, 3, int(((r >= 0.05) & (r < 0.1)).sum()))
    n_new = ROWS_N + ROWS_GROW
    upd_nodes = ru.batch_nodes("mixed", ROWS_M, n_new, seed=5)
    upd_nodes[:n_new] = np.where(rng.random(n_new) < 0.5, rng.permutation(n_new), upd_nodes[:n_new])  # (half the graph is named)
    upd_rows = rr.family("uniform", ROWS_N, K, seed=12, nrows=ROWS_M)  # (ids below the OLD node count: valid in both graphs)
    offers = {"req": ROWS_M, "compact_check": ROWS_N}
    if K == 16:    # (flat_lists: k_ef_arena_geom, when the arena rows become CSR streams for decode_lists)
        offers.update({"rows_tile": ROWS_M, "roc_rows": ROWS_N, "flat_lists": ROWS_N})
    elif K > 64:   # (flat_lists: k_rows_count; wave_per_list: k_rows_to_ids, k_compact_rows_encode / update, k_ef_decode)
        offers.update({"flat_lists": ROWS_N, "wave_per_list": ROWS_N, "compact_wide": ROWS_M})
    else:
        offers.update({"compact_rows4": ROWS_M, "wave_per_list": ROWS_N})
    return dict(rows=rows, nodes=nodes, upd_nodes=upd_nodes, upd_rows=upd_rows, n_new=n_new, offers=offers)


_BUILDERS = {"short": _short, "mid": _mid, "long": _long, "mixed": _mixed, "many_long": _many_long, "chunky": _chunky, "full": _full,
             "perm": _perm_lists, "perm_big": lambda: _perm_lists(1_100_003, 100), "seg": _seg, "rows": _rows, "rows_wide": lambda: _rows(80), "rows_k7": lambda: _rows(7)}

#: pairs of a batch (append, remove, locate): three trips of the sort tiles (32 x 1024 pairs) and of the request kernels
N_PAIRS = 70_001
#: pairs of a batch on the 17 001 short lists: the per-list loops are what that shape is there for
N_PAIRS_SHORT = 20_001
BATCH_OFFERS = {"sort_tile": (N_PAIRS + 1023) // 1024, "req": N_PAIRS}
BATCH_SHORT_OFFERS = {"req": N_PAIRS_SHORT}


def lists_of(pos, off):
    return (np.searchsorted(np.asarray(off).astype(np.int64), pos, side="right") - 1).astype(np.int64)


def pair_batch(off, ids, n, seed, absent=1):
    """(list, id) pairs for a remove or a locate: half of them hit; the rest name an id no list holds (id + absent: 6 k + 4 in the list
    shapes; the permutation shape passes ntotal), a present id under another list, a negative or too large list number, or repeat an
    earlier pair"""
    rng = np.random.default_rng(seed)
    nlist = off.size - 1
    pos = rng.choice(ids.size, n, replace=n > ids.size // 2)
    want, ln = ids[pos].copy(), lists_of(pos, off)
    what = rng.integers(0, 10, n)
    want[what == 5] += np.uint64(absent)
    wrong = what == 6
    ln[wrong] = (ln[wrong] + 1 + rng.integers(0, nlist - 1, int(wrong.sum()))) % nlist
    ln[what == 7] = -1 - rng.integers(0, 5, int((what == 7).sum()))
    ln[what == 8] = nlist + rng.integers(0, 3, int((what == 8).sum()))
    rep = np.flatnonzero(what == 9)
    src = rng.integers(0, n, rep.size)
    want[rep], ln[rep] = want[src], ln[src]
    return ln, want


def append_batch(kind, sh, n, seed, only=None):
    """n (list, id) pairs whose ids no list holds yet; some pairs skipped (negative list) or invalid (list >= nlist).  only: the lists
    the valid pairs go to.  Wavelet tree: ids ntotal .. in batch order, so that the merged lists stay a permutation."""
    rng = np.random.default_rng(seed)
    nlist, ntotal = sh["sizes"].size, int(sh["sizes"].sum())
    pool = np.arange(nlist) if only is None else np.asarray(only)
    ln = pool[rng.integers(0, pool.size, n)].astype(np.int64)
    ln[rng.integers(0, n, 40)] = -1
    ln[rng.integers(0, n, 40)] = nlist + rng.integers(0, 3, 40)
    if kind.startswith("wt"):
        valid = (ln >= 0) & (ln < nlist)
        return ln, (ntotal + np.cumsum(valid) - 1).astype(np.uint64)
    return ln, spread((1 << 24) + rng.permutation(n))  # (above every id of the list shapes, below 2^28)


# --------------------------------------------------------------------------------------------------------------------------- GPU side
def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _codecs():
    from vector_db_id_compression_amd import codecs

    return codecs


def sync():
    _torch().cuda.synchronize()


def dev(a):
    t = _torch()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return t.from_numpy(a.view(np.int64)).cuda() if a.size else t.zeros(0, dtype=t.int64, device="cuda")


def dev_i64(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def zeros1():
    return _torch().zeros(1, dtype=_torch().int64, device="cuda")


@pytest.fixture(scope="module")
def small():
    """three contexts created under VIDC_NUM_CU=1, pool poison on: [0] runs on torch's stream like the default context does (the
    home of the sharded objects), [1] and [2] hold the two shards"""
    L, torch = _lib(), _torch()
    torch.cuda.set_device(0)
    mp = pytest.MonkeyPatch()
    mp.setenv("VIDC_NUM_CU", "1")
    ctxs = [L.Context(0) for _ in range(3)]
    mp.undo()
    for c in ctxs:
        assert c.num_cu() == 1
        c.set_pool_poison(True)
    ctxs[0].set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctxs
    sync()
    for c in ctxs:
        c.synchronize()
        c.close()


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for h in HOOKS + ("VIDC_NUM_CU", "VIDC_WT_SCATTER"):
        monkeypatch.delenv(h, raising=False)


def test_the_hook_only_lowers_the_count(small, monkeypatch):
    L = _lib()
    own = L.default_context().num_cu()
    assert own > 1 and all(c.num_cu() == 1 for c in small)
    for value, want in (("100000", own), (str(own), own), ("0", own), ("-3", own), ("four", own), ("2x", own), ("", own), ("2", 2),
                        (str(own - 1), own - 1)):
        monkeypatch.setenv("VIDC_NUM_CU", value)
        c = L.Context(0)
        monkeypatch.delenv("VIDC_NUM_CU")
        assert c.num_cu() == want, f"VIDC_NUM_CU={value!r}"
        c.close()
    assert L.lib().vidc_ctx_num_cu(None) == 0


# ----------------------------------------------------------------------------------------------------------------- the list containers
def encode(kind, off, ids, ctx, want_perm=True, dev_offsets=False):
    cd = _codecs()
    d = dev(ids)
    o = dev(off) if dev_offsets else off
    sync()
    if kind == "packed":
        return cd.PackedLists.encode(o, d, bits=BITS, ctx=ctx)
    if kind == "ef":
        return cd.EfLists.encode(o, d, want_perm=want_perm, ctx=ctx)
    if kind == "roc":
        return cd.RocLists.encode(o, d, want_perm=want_perm, ctx=ctx)
    return cd.WaveletTreeLists.build(o, d, wt_type=1 if kind == "wt1" else 0, ctx=ctx)


def image(kind, obj, want_perm=True):
    from vector_db_id_compression_amd import persist

    import test_gpu_dev_offsets as do

    sync()
    if kind == "packed":
        return dict(offsets=obj.offsets, **do.packed_image(obj))
    if kind == "ef":
        d = dict(offsets=obj.offsets, **do.ef_image(obj, want_perm))
        if obj.ntotal == 0:  # (an object without ids reports one padding word per stream that no encoder writes)
            d["low"], d["high"] = d["low"][:0], d["high"][:0]
        return d
    if kind == "roc":
        return dict(offsets=obj.offsets, ntotal=obj.ntotal, **do.roc_image(obj, want_perm))
    return dict(size=obj.size_in_bytes, levels=obj.levels, **persist.wt_image(obj))


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differs"


_DEFAULT = {}


def default_image(kind, name):
    """the image of the shape's object on the default context, computed once"""
    if (kind, name) not in _DEFAULT:
        sh = shape(name)
        obj = encode(kind, sh["off"], sh["ids"], None)
        assert obj.ctx.num_cu() > 1
        _DEFAULT[(kind, name)] = image(kind, obj)
    return _DEFAULT[(kind, name)]


_ROC = {}


def roc_expectation(oracle, name):
    """per list of the shape what the CPU oracle makes of it: precision, head, word count, draws; all words, the decode order and the
    permutation back to back.  Computed once."""
    if name not in _ROC:
        sh = shape(name)
        n = sh["sizes"].size
        exp = dict(precision=np.zeros(n, np.uint32), heads=np.zeros(n, np.uint64), nwords=np.zeros(n, np.uint32),
                   mt_draws=np.zeros(n, np.uint32))
        words, dec, perm = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint64)], [np.zeros(0, np.uint32)]
        for l, li in enumerate(sh["lists"]):
            if not li.size:
                continue
            P = oracle.list_precision(li)
            e = oracle.roc_encode(li, P)
            exp["precision"][l], exp["heads"][l], exp["nwords"][l], exp["mt_draws"][l] = P, e["head"], e["words"].size, e["mt_draws"]
            words.append(e["words"]); dec.append(e["order"]); perm.append(e["perm"])
        exp.update(words=np.concatenate(words), dec=np.concatenate(dec).astype(np.uint64), perm=np.concatenate(perm))
        _ROC[name] = exp
    return _ROC[name]


def check_roc_streams(obj, sh, exp, what):
    info = obj.info()
    ne = sh["sizes"] > 0
    assert np.array_equal(info["sizes"], sh["sizes"]) and np.array_equal(info["nwords"], exp["nwords"]), f"{what}: sizes / word counts"
    for k in ("precision", "heads", "mt_draws"):
        assert np.array_equal(info[k][ne], exp[k][ne]), f"{what}: {k} differs from the oracle"
    assert np.array_equal(obj.all_words(), exp["words"]), f"{what}: stack words differ from the oracle"
    assert obj.compressed_bytes == 8 * int(ne.sum()) + 4 * exp["words"].size
    assert np.array_equal(obj.perm(), exp["perm"]), f"{what}: the permutation differs from the oracle"


def expected_flat(kind, sh, oracle, name):
    """what decode_all must return: packed input order, Elias-Fano / wavelet tree ascending (the shapes are ascending), ROC the
    oracle's sampling order"""
    return roc_expectation(oracle, name)["dec"] if kind == "roc" else sh["ids"]


def check_requests(kind, obj, sh, flat, what):
    """decode_all, decode_lists (every list, in reverse, and repeats), translate_labels (every position, negative and invalid labels,
    in place), decode_gather"""
    torch = _torch()
    off, sizes = sh["off"].astype(np.int64), sh["sizes"]
    nlist = sizes.size
    rng = np.random.default_rng(nlist)
    sync()
    dec = obj.decode_all().cpu().numpy().view(np.uint64)
    assert np.array_equal(dec, flat), f"{what}: decode_all"
    req = np.concatenate([np.arange(nlist)[::-1], rng.integers(0, nlist, 9), [0, 0]]).astype(np.uint64)
    got, ro = obj.decode_lists(req)
    want = [flat[off[l]:off[l + 1]] for l in req.astype(np.int64)]
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.concatenate(want)), f"{what}: decode_lists"
    assert np.array_equal(ro, csr([w.size for w in want])), f"{what}: decode_lists offsets"
    lab = lr.all_labels(sizes, rng)
    want_ids, want_invalid = lr.expect_labels(lab, sizes, flat)
    d_lab, invalid = dev_i64(lab), zeros1()
    sync()
    out = obj.translate_labels(d_lab, invalid=invalid)
    sync()
    assert np.array_equal(out.cpu().numpy(), want_ids) and int(invalid.item()) == want_invalid, f"{what}: translate_labels"
    assert np.array_equal(d_lab.cpu().numpy(), lab), f"{what}: the labels are left alone"
    assert obj.translate_labels(d_lab, out=d_lab, invalid=invalid) is d_lab
    sync()
    assert np.array_equal(d_lab.cpu().numpy(), want_ids) and int(invalid.item()) == 2 * want_invalid, f"{what}: in place"
    uniq = np.flatnonzero(sizes)[:: max(1, nlist // 300)]
    slot = rng.integers(0, uniq.size, 500)
    item = (rng.random(500) * sizes[uniq[slot]]).astype(np.int64)
    assert np.array_equal(obj.decode_gather(uniq, slot, item).view(np.uint64), flat[off[uniq[slot]] + item]), f"{what}: decode_gather"


def check_model_words(kind, obj, sh, what):
    """Elias-Fano and packed bits: the closed-form model's words, list by list (a sample that holds every size class)"""
    sizes = sh["sizes"]
    rng = np.random.default_rng(sizes.size)
    pick = np.unique(np.concatenate([[0, sizes.size - 1], np.argsort(sizes)[-12:], np.flatnonzero(sizes == 0)[:2],
                                     rng.integers(0, sizes.size, 120)]))
    if kind == "ef":
        assert obj.compressed_bytes == lr.ef_sizes(sh["lists"])["compressed_bytes"], f"{what}: compressed_bytes"
        assert np.array_equal(obj.info()["sizes"], sizes)
        for l in pick[sizes[pick] > 0]:
            m = lr.ef_list(sh["lists"][l])
            low, high, lb, hb = obj.export(int(l))
            assert (lb, hb) == (m.low_nbits, m.high_nbits) and np.array_equal(low, m.low) and np.array_equal(high, m.high), f"{what}: list {l}"
    elif kind == "packed":
        assert obj.bits == BITS
        for l in pick:
            assert np.array_equal(obj.export_bytes(int(l)), lr.packed_list(sh["lists"][l], BITS)), f"{what}: list {l}"


_WT_LEVELS = {}


def check_wt_model(kind, obj, sh, name, what):
    """the numpy model of the tree (tests/wt_ref.py, tests/image_ref.py): levels, the documented size, every bit of the plain image, the
    class words and offset-stream lengths of the RRR image (the offsets themselves are the library's own combinatorial rank)"""
    from vector_db_id_compression_amd import persist

    nlist = sh["sizes"].size
    if name not in _WT_LEVELS:
        _WT_LEVELS[name] = wt_ref.levels(sh["sym"], nlist)
    lv = _WT_LEVELS[name]
    im = persist.wt_image(obj)
    assert obj.levels == len(lv) == wt_ref.n_levels(nlist)
    if kind == "wt":
        assert obj.size_in_bytes == wt_ref.plain_size(lv, nlist), f"{what}: size_in_bytes"
        assert np.array_equal(im["bits"], image_ref.wt_plain_image(lv, nlist)), f"{what}: the level bits differ from the model"
    else:
        assert obj.size_in_bytes == wt_ref.rrr_size(lv, nlist), f"{what}: size_in_bytes"
        cls, off_bits = image_ref.wt_rrr_classes(lv, nlist)
        assert np.array_equal(im["cls"], cls) and np.array_equal(im["off_bits"], off_bits), f"{what}: the RRR classes differ from the model"
    assert image_ref.node_counts_ok(lv, sh["off"], nlist)


LIST_CASES = [("packed", "short"), ("packed", "chunky"), ("packed", "full"), ("ef", "short"), ("ef", "chunky"), ("ef", "full"),
              ("roc", "short"), ("roc", "mid"), ("roc", "long"), ("roc", "chunky"), ("wt", "perm"), ("wt1", "perm")]


@pytest.mark.parametrize("kind,name", LIST_CASES)
def test_encode_and_every_request(small, oracle, kind, name):
    """host offsets and device offsets on the one-CU context: the default context's object word for word, the model's words, every
    request against the reference"""
    sh = shape(name)
    what = f"{kind} {name}"
    obj = encode(kind, sh["off"], sh["ids"], small[0])
    got = image(kind, obj)
    same(got, default_image(kind, name), f"{what}: one CU against the default context")
    from_dev = encode(kind, sh["off"], sh["ids"], small[0], dev_offsets=True)
    same(image(kind, from_dev), got, f"{what}: device offsets against host offsets")
    if kind == "roc":
        check_roc_streams(obj, sh, roc_expectation(oracle, name), what)
        assert obj.last_decode_nonclean == 0
    check_model_words(kind, obj, sh, what)
    flat = expected_flat(kind, sh, oracle, name)
    check_requests(kind, obj, sh, flat, what)
    check_requests(kind, from_dev, sh, flat, what + " (device offsets)")
    if kind.startswith("wt"):
        check_wt_model(kind, obj, sh, name, what)
        ne = np.flatnonzero(sh["sizes"])
        rng = np.random.default_rng(3)
        ln = rng.choice(ne, 3000)
        of = (rng.random(ln.size) * sh["sizes"][ln]).astype(np.uint64)
        assert np.array_equal(obj.select(ln, of).view(np.uint64), sh["ids"][sh["off"].astype(np.int64)[ln] + of.astype(np.int64)])


def test_wavelet_tree_direct_scatter_at_every_size(small, monkeypatch):
    """VIDC_WT_SCATTER: the direct scatter (32 workgroups x 4096 ids a trip at one CU) instead of the partitioned one -- the same tree"""
    sh = shape("perm")
    monkeypatch.setenv("VIDC_WT_SCATTER", "1")
    for kind in ("wt", "wt1"):
        same(image(kind, encode(kind, sh["off"], sh["ids"], small[0])), default_image(kind, "perm"), f"{kind}: direct scatter")


def test_wavelet_tree_rrr_block_passes(small):
    """1 100 003 ids: the block passes of the RRR coding (k_rrr_classes, k_rrr_offsets at build, k_rrr_expand at decode_all; 516 096 ids
    a trip at one CU) take three trips.  Build from host and device offsets, the default context's image, the model's classes and
    size, and the cheap exact invariants of a case this large: decode_all is the input, select answers it"""
    sh = shape("perm_big")
    what = "wt1 perm_big"
    obj = encode("wt1", sh["off"], sh["ids"], small[0])
    got = image("wt1", obj)
    same(got, default_image("wt1", "perm_big"), f"{what}: one CU against the default context")
    from_dev = encode("wt1", sh["off"], sh["ids"], small[0], dev_offsets=True)
    same(image("wt1", from_dev), got, f"{what}: device offsets against host offsets")
    check_wt_model("wt1", obj, sh, "perm_big", what)
    sync()
    for o in (obj, from_dev):
        dec = o.decode_all().cpu().numpy().view(np.uint64)
        assert np.array_equal(dec, sh["ids"]), f"{what}: decode_all is not the input permutation"
    off = sh["off"].astype(np.int64)
    assert all(np.all(np.diff(dec[off[l]:off[l + 1]].astype(np.int64)) > 0) for l in range(off.size - 1)), "ascending inside every list"
    rng = np.random.default_rng(5)
    ln = rng.choice(np.flatnonzero(sh["sizes"]), 3000)
    of = (rng.random(ln.size) * sh["sizes"][ln]).astype(np.uint64)
    assert np.array_equal(obj.select(ln, of).view(np.uint64), sh["ids"][off[ln] + of.astype(np.int64)])
    lab = (ln.astype(np.int64) << 32) | of.astype(np.int64)
    out = obj.translate_labels(dev_i64(lab))
    sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), sh["ids"][off[ln] + of.astype(np.int64)])


@pytest.mark.parametrize("hook", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
@pytest.mark.parametrize("name", ["short", "mid", "long", "chunky", "many_long"])
def test_roc_shapes_with_the_other_kernel_families(small, oracle, monkeypatch, name, hook):
    """every ROC shape again with every list on the general kernels and with the lane kernels off: the compaction kernel of a call is
    chosen by its average stream length, so each of the three meets each family"""
    sh, exp = shape(name), roc_expectation(oracle, name)
    want = default_image("roc", name)
    monkeypatch.setenv(hook, "1")
    obj = encode("roc", sh["off"], sh["ids"], small[0])
    same(image("roc", obj), want, f"{name}, {hook}: one CU against the default context without the hook")
    check_roc_streams(obj, sh, exp, f"{name}, {hook}")
    sync()
    assert np.array_equal(obj.decode_all().cpu().numpy().view(np.uint64), exp["dec"]), f"{name}, {hook}: decode_all"
    assert obj.last_decode_nonclean == 0


@pytest.mark.parametrize("hook", [None, *HOOKS])
def test_roc_every_class_in_one_call(small, oracle, monkeypatch, hook):
    """9000 short lists, 300 of 17 .. 256 ids and 40 of 300 .. 2000 ids in one call, also with the lane kernels off, with every list on
    the general kernels, and with the full prepass (32 workgroups, a list each)"""
    sh, exp = shape("mixed"), roc_expectation(oracle, "mixed")
    want = default_image("roc", "mixed")
    if hook:
        monkeypatch.setenv(hook, "1")
    obj = encode("roc", sh["off"], sh["ids"], small[0])
    same(image("roc", obj), want, f"mixed, {hook}: one CU against the default context")
    check_roc_streams(obj, sh, exp, f"mixed, {hook}")
    check_requests("roc", obj, sh, exp["dec"], f"mixed, {hook}")
    assert obj.last_decode_nonclean == 0


def test_roc_more_long_lists_than_chains_fit(small, oracle):
    """seven lists of 33 000 .. 40 000 ids: at one CU only six of them go to the position-bitmap chains (promote_r2, n_long > cap), on
    the default context all seven do (tests/test_small_grid_shapes_cpu.py runs the planner's own promote_r2 on these sizes; no call
    reports the chain class of a launch: vidc_ctx_chain_info speaks of the universe-bitmap kernels only) -- the same streams"""
    sh, exp = shape("many_long"), roc_expectation(oracle, "many_long")
    obj = encode("roc", sh["off"], sh["ids"], small[0])
    same(image("roc", obj), default_image("roc", "many_long"), "many_long: one CU against the default context")
    check_roc_streams(obj, sh, exp, "many_long")
    sync()
    assert np.array_equal(obj.decode_all().cpu().numpy().view(np.uint64), exp["dec"])


# ----------------------------------------------------------------------------------------------------------- segmented ROC lists
_SEG = {}


def seg_reference(oracle):
    if not _SEG:
        sh = shape("seg")
        model = sr.split(sh["off"], sh["ids"], SEG_T, SEG_B)
        encs = sr.encode_segments(model, oracle)
        _SEG.update(T=SEG_T, B=SEG_B, off=sh["off"], ids=sh["ids"], model=model, encs=encs, dec=sr.decode_order(model, encs),
                    perm=sr.compose_perm(model, sr.inner_perm(model, encs)))
    return _SEG


@pytest.mark.parametrize("hook", [None, "VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
def test_segmented_roc(small, oracle, monkeypatch, hook):
    import test_gpu_roc_segmented as seg

    ref = seg_reference(oracle)
    k = ref["model"]["k"]
    assert sorted(set(k.tolist())) == [0, 7, 10] and len(sr.chunk_table(ref["off"], SEG_T, SEG_B)[0]) == shape("seg")["offers"]["chunk1024"]
    cls = _codecs().RocSegLists
    d_ids = dev(ref["ids"])
    sync()
    if "default" not in _SEG:
        _SEG["default"] = seg.export(cls.encode(ref["off"], d_ids, seg_ids=SEG_T, universe_bits=SEG_B, want_perm=True))
    if hook:
        monkeypatch.setenv(hook, "1")
    obj = cls.encode(ref["off"], d_ids, seg_ids=SEG_T, universe_bits=SEG_B, want_perm=True, ctx=small[0])
    for a, b in zip(seg.export(obj), _SEG["default"]):
        assert np.array_equal(a, b), "one CU against the default context"
    dec = seg.check_object(obj, ref)
    off = ref["off"].astype(np.int64)
    for l in range(off.size - 1):
        assert np.array_equal(np.sort(dec[off[l]:off[l + 1]]), np.sort(ref["ids"][off[l]:off[l + 1]])), f"list {l}: lossless"
    if hook is None:  # device offsets, universe_bits found on the device (k_rocseg_max), no permutation
        found = cls.encode(dev(ref["off"]), d_ids, seg_ids=SEG_T, ctx=small[0])
        assert found.universe_bits == SEG_B
        for a, b in zip(seg.export(found), _SEG["default"]):
            assert np.array_equal(a, b), "device offsets against the default context"
        seg.check_object(found, ref, perm=False)


# ------------------------------------------------------------------------------------------------------- append, remove, locate
def ref_kind(kind):
    return "wt" if kind == "wt1" else kind


def do_append(kind, obj, ln, add, invalid):
    d_ln, d_add = dev_i64(ln), dev(add)
    sync()
    if kind in ("ef", "roc"):
        out = obj.append(d_ln, d_add, want_perm=True, labels=True, invalid=invalid)
    else:
        out = obj.append(d_ln, d_add, labels=True, invalid=invalid)
    sync()
    return out


#: (kind, shape): the wavelet tree holds a permutation and has its own shape
BATCH_CASES = [(k, n) for k in ("packed", "ef", "roc") for n in ("chunky", "short")] + [("wt", "perm"), ("wt1", "perm")]


@pytest.mark.parametrize("kind,name", BATCH_CASES)
def test_append(small, oracle, kind, name):
    sh = shape(name)
    n = N_PAIRS_SHORT if name == "short" else N_PAIRS
    ln, add = append_batch(kind, sh, n, seed=len(kind) + n)
    what = f"{kind} {name} append"
    news, labs = [], []
    for ctx in (small[0], None):
        old = encode(kind, sh["off"], sh["ids"], ctx)
        before = image(kind, old)
        inv = zeros1()
        new, lab = do_append(kind, old, ln, add, inv)
        same(image(kind, old), before, f"{what}: the old object changed")
        news.append(new); labs.append((lab.cpu().numpy(), int(inv.item())))
    new = news[0]
    old_dec = expected_flat(kind, sh, oracle, name)
    m = ar.merge(sh["off"], old_dec, ln, add)
    got = image(kind, new)
    same(got, image(kind, news[1]), f"{what}: one CU against the default context")
    same(got, image(kind, encode(kind, m.offsets, m.ids, None)), f"{what}: against the encoder's object of the merged lists")
    assert labs[0][1] == labs[1][1] == m.invalid
    want_lab = ar.labels(ref_kind(kind), m, oracle)
    assert np.array_equal(labs[0][0], want_lab) and np.array_equal(labs[1][0], want_lab), f"{what}: labels differ from the reference"
    back = new.translate_labels(dev_i64(labs[0][0]))
    sync()
    assert np.array_equal(back.cpu().numpy(), np.where(m.valid, add.view(np.int64), -1)), f"{what}: the labels do not lead back to the batch"


def do_remove(kind, obj, ln, rm):
    from vector_db_id_compression_amd import removal

    d_ln, d_rm = None if ln is None else dev_i64(ln), dev(rm)
    mis, inv = zeros1(), zeros1()
    sync()
    new, mask = removal.remove(obj, d_ln, d_rm, want_perm=True, missing=mis, invalid=inv)
    sync()
    return new, mask.cpu().numpy(), int(mis.item()), int(inv.item())


@pytest.mark.parametrize("mode", ["pairs", "any"])
@pytest.mark.parametrize("name", ["chunky", "short"])
@pytest.mark.parametrize("kind", ["packed", "ef", "roc"])
def test_remove(small, oracle, kind, name, mode):
    sh = shape(name)
    n = N_PAIRS_SHORT if name == "short" else N_PAIRS
    ln, rm = pair_batch(sh["off"], sh["ids"], n, seed=n + len(kind))
    ln = ln if mode == "pairs" else None
    what = f"{kind} {name} remove ({mode})"
    res = []
    for ctx in (small[0], None):
        old = encode(kind, sh["off"], sh["ids"], ctx)
        before = image(kind, old)
        res.append(do_remove(kind, old, ln, rm))
        same(image(kind, old), before, f"{what}: the old object changed")
    m = remove_ref.remove(sh["off"], expected_flat(kind, sh, oracle, name), ln, rm)
    assert m.removed > 0 and m.missing > 0 and (mode == "any" or m.invalid > 0)
    for new, mask, missing, invalid in res:
        assert np.array_equal(mask, m.mask), f"{what}: the removed mask differs from the model"
        assert (missing, invalid) == (m.missing, m.invalid) and new.ntotal == sh["ids"].size - m.removed, what
    got = image(kind, res[0][0])
    same(got, image(kind, res[1][0]), f"{what}: one CU against the default context")
    same(got, image(kind, encode(kind, m.offsets, m.ids, None)), f"{what}: against the encoder's object of the surviving lists")


def id_bits_of(kind):
    return {"packed": BITS, "roc": 32}.get(kind, 64)


@pytest.mark.parametrize("mode", ["pairs", "any"])
@pytest.mark.parametrize("kind,name", BATCH_CASES)
def test_locate(small, oracle, kind, name, mode):
    """pairs mode names only some lists (the others are chunks with an empty run: the early `continue` of k_loc_mark)"""
    from vector_db_id_compression_amd import locate

    sh = shape(name)
    n = N_PAIRS_SHORT if name == "short" else N_PAIRS
    ln, ids = pair_batch(sh["off"], sh["ids"], n, seed=2 * n + len(kind), absent=sh["ids"].size if name == "perm" else 1)
    if mode == "pairs" and name != "short":  # (every pair of the lists 3 k + 1 becomes a skipped pair: those lists have no run)
        ln[(ln >= 0) & (ln % 3 == 1)] = -1
    ln = ln if mode == "pairs" else None
    what = f"{kind} {name} locate ({mode})"
    flat = expected_flat(kind, sh, oracle, name)
    labels, missing, invalid = locate_ref.locate(sh["off"], flat, ln, ids, id_bits_of(kind))
    assert (labels >= 0).sum() > n // 4 and missing > 0
    for ctx in (small[0], None):
        obj = encode(kind, sh["off"], sh["ids"], ctx)
        before = image(kind, obj)
        d_ln, d_ids, mis, inv = None if ln is None else dev_i64(ln), dev(ids), zeros1(), zeros1()
        whole, view = cr.guarded(ids.size, np.int64, device="cuda")
        sync()
        out = locate.locate(obj, d_ln, d_ids, out=view, missing=mis, invalid=inv)
        sync()
        assert out is view
        cr.assert_guards_intact(whole, view, what)
        cr.assert_view_equals(view, labels, what)
        assert (int(mis.item()), int(inv.item())) == (missing, invalid), f"{what}: (missing, invalid)"
        hit = labels >= 0
        back = obj.translate_labels(dev_i64(labels[hit]))
        sync()
        assert np.array_equal(back.cpu().numpy().view(np.uint64), ids[hit]), f"{what}: translate_labels does not lead back to the ids"
        same(image(kind, obj), before, f"{what}: the object changed")


# -------------------------------------------------------------------------------------------------------------------- save and load
def test_save_and_load_once(small, oracle, tmp_path):
    """one object of every container through its flat image, loaded on the one-CU context (the import passes: k_ef_hrank_from_high, the
    wavelet tree's block check, the ROC import)"""
    from vector_db_id_compression_amd import persist

    import test_gpu_roc_segmented as seg

    for kind, name in (("packed", "chunky"), ("ef", "chunky"), ("roc", "chunky"), ("wt", "perm"), ("wt1", "perm")):
        sh = shape(name)
        obj = encode(kind, sh["off"], sh["ids"], small[0])
        back = persist.load(persist.save(obj, str(tmp_path / f"{kind}")), ctx=small[0])
        assert type(back) is type(obj) and back.ctx is small[0]
        want = default_image(kind, name)
        if kind in ("ef", "roc"):  # (an image keeps no permutation)
            want = {k: v for k, v in want.items() if k != "perm"}
        same(image(kind, back, want_perm=False), want, f"{kind}: loaded on one CU against the default context's object")
        sync()
        assert np.array_equal(back.decode_all().cpu().numpy().view(np.uint64), expected_flat(kind, sh, oracle, name)), f"{kind}: decode after load"
    ref = seg_reference(oracle)
    cls = _codecs().RocSegLists
    obj = cls.encode(ref["off"], dev(ref["ids"]), seg_ids=SEG_T, universe_bits=SEG_B, ctx=small[0])
    back = persist.load(persist.save(obj, str(tmp_path / "seg")), ctx=small[0])
    for a, b in zip(seg.export(back), seg.export(obj)):
        assert np.array_equal(a, b)
    sync()
    assert np.array_equal(back.decode_all().cpu().numpy().view(np.uint64), ref["dec"])


# ---------------------------------------------------------------------------------------------------------------------- graph rows
def rows_cls(codec):
    cd = _codecs()
    return {"compact": cd.CompactRows, "ef": cd.EfLists, "roc": cd.RocLists}[codec]


def rows_image(codec, g):
    from vector_db_id_compression_amd import persist

    import test_gpu_graph_rows as gr

    sync()
    if codec == "compact":
        return dict(data=persist.compact_image(g), bits=g.bits, stride=g.stride, size=g.size_in_bytes)
    if codec == "ef":
        low, high = gr.ef_all_words(g)
        return dict(low=low, high=high, bytes=g.compressed_bytes, **g.info())
    return dict(words=g.all_words(), bytes=g.compressed_bytes, ntotal=g.ntotal, **g.info())


def check_rows(codec, g, R, ref, nodes, what):
    """the model's image (compact, Elias-Fano), every node in order, a host node list and a CUDA node tensor of 20 001 nodes"""
    N, K = R.shape
    if codec == "compact":
        assert (g.bits, g.stride) == (rr.compact_bits(N), rr.compact_stride(N, K))
        assert np.array_equal(rows_image(codec, g)["data"], rr.compact_rows(R)), f"{what}: the model's bytes"
    elif codec == "ef" and K <= 64:
        m = rr.ef_rows(R)
        info = g.info()
        assert np.array_equal(info["sizes"], m.n) and np.array_equal(info["low_bits"], m.l) and np.array_equal(info["universe"], m.u.astype(np.uint64))
        assert g.compressed_bytes == m.size_in_bytes, f"{what}: compressed_bytes"
        for i in np.random.default_rng(N).integers(0, N, 200):
            low, high, lb, hb = g.export(int(i))
            wl, wh = m.words(i)
            assert (lb, hb) == (int(m.low_nbits[i]), int(m.high_nbits[i])) and np.array_equal(low, wl) and np.array_equal(high, wh), f"{what}: row {i}"
    sync()
    want, cnt = ref.expected(None, K)
    every, c0 = g.decode_rows(None, K)
    assert np.array_equal(every.cpu().numpy(), want) and np.array_equal(c0, cnt), f"{what}: decode_rows(None)"
    host = nodes[(nodes >= 0) & (nodes < N)]
    want, cnt = ref.expected(host, K)
    sub, c1 = g.decode_rows(host.astype(np.uint64), K)
    assert np.array_equal(sub.cpu().numpy(), want) and np.array_equal(c1, cnt), f"{what}: decode_rows(host nodes)"
    want, cnt = ref.expected(nodes, K)
    d_nodes = dev_i64(nodes)
    sync()
    dsub, c2 = g.decode_rows(d_nodes, K)
    sync()
    assert np.array_equal(dsub.cpu().numpy(), want) and np.array_equal(c2.cpu().numpy(), cnt), f"{what}: decode_rows(CUDA nodes)"
    if codec == "ef":  # decode_lists: the arena rows become CSR streams first (k_ef_arena_geom, k_ef_arena_to_csr)
        want, cnt = ref.expected(None, K)
        req = np.arange(N)[::-1].astype(np.uint64)
        out, out_off = g.decode_lists(req)
        flat = np.concatenate([want[i, : cnt[i]] for i in req.astype(np.int64)]).astype(np.int64)
        assert np.array_equal(out.cpu().numpy(), flat) and np.array_equal(out_off, csr(cnt[req.astype(np.int64)])), f"{what}: decode_lists"


ROWS_CASES = [("compact", "rows"), ("ef", "rows"), ("roc", "rows"), ("compact", "rows_wide"), ("ef", "rows_wide"), ("roc", "rows_wide"),
              ("compact", "rows_k7")]


@pytest.mark.parametrize("codec,name", ROWS_CASES)
def test_graph_rows_encode_decode_update(small, oracle, tmp_path, codec, name):
    """encode_rows, every decode form and update_rows (Elias-Fano and ROC update rows of up to 64 ids only); compact rows also through
    their flat image (k_compact_check_rows)"""
    from vector_db_id_compression_amd import persist

    sh = shape(name)
    rows, K = sh["rows"], ROWS_SHAPES[name]
    cls = rows_cls(codec)
    what = f"{codec} {name}"
    d_rows = _torch().from_numpy(rows).cuda()
    sync()
    g, g_def = cls.encode_rows(d_rows, ctx=small[0]), cls.encode_rows(d_rows)
    same(rows_image(codec, g), rows_image(codec, g_def), f"{what}: one CU against the default context")
    ref = cr.RowRef(codec, rows, oracle)
    check_rows(codec, g, rows, ref, sh["nodes"], what)
    if codec == "compact":
        back = persist.load(persist.save(g, str(tmp_path / "compact")), ctx=small[0])
        same(rows_image(codec, back), rows_image(codec, g_def), f"{what}: loaded on one CU against the default context's object")
    elif K > 64:
        return
    # update_rows: an untouched row keeps its record (ROC: its stream, which is the encoder's for the row's id set), a named one is encoded
    R, want_invalid, _ = ru.update_rows(rows, sh["upd_nodes"], sh["upd_rows"], sh["n_new"])
    before = rows_image(codec, g)
    news = []
    for old in (g, g_def):
        d_n, d_r, inv = dev_i64(sh["upd_nodes"]), _torch().from_numpy(sh["upd_rows"]).cuda(), zeros1()
        sync()
        new = _codecs().update_rows(old, d_n, d_r, n_new=sh["n_new"], invalid=inv)
        sync()
        assert int(inv.item()) == want_invalid, f"{what}: invalid nodes of the update"
        news.append(new)
    same(rows_image(codec, g), before, f"{what}: the old object changed")
    got = rows_image(codec, news[0])
    same(got, rows_image(codec, news[1]), f"{what} update: one CU against the default context")
    fresh = cls.encode_rows(_torch().from_numpy(R).cuda())
    same(got, rows_image(codec, fresh), f"{what} update: against the encoder's object of the updated rows")
    check_rows(codec, news[0], R, cr.RowRef(codec, R, oracle), sh["nodes"], f"{what} update")


# -------------------------------------------------------------------------------------------------------------------- sharded lists
def shard_images(kind, X):
    out = []
    for s in range(X.nshards):
        view = X.shard(s)
        out.append(None if view is None else image(kind, view))
    return out + [np.array(X.owner), np.array(X.local_no), np.array(X.loads), np.array(X.offsets)]


def same_shards(a, b, what):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, dict):
            same(x, y, f"{what}: shard {s}")
        else:
            assert (x is None and y is None) or np.array_equal(x, y), f"{what}: entry {s}"


def shard_args(kind):
    return {"bits": BITS} if kind == "packed" else {"want_perm": True}


@pytest.mark.parametrize("kind", ["packed", "ef", "roc"])
def test_two_shards_encode_append_remove_rebalance(small, oracle, kind):
    """a two-shard object whose home and shard contexts are all one-CU contexts, next to one on ordinary contexts"""
    import rebalance_ref as rb
    from vector_db_id_compression_amd.sharding import DeviceShards, lpt_partition

    L = _lib()
    sh = shape("chunky")
    what = f"{kind} shards"
    flat = expected_flat(kind, sh, oracle, "chunky")
    d_ids = dev(sh["ids"])
    plain = [L.Context(0), L.Context(0)]
    owner = lpt_partition(sh["sizes"], 2)
    ln_a, add = append_batch(kind, sh, N_PAIRS, seed=77, only=np.flatnonzero(owner == 0))  # (every pair to shard 0: the map goes stale)
    ln_r, rm = pair_batch(sh["off"], sh["ids"], N_PAIRS, seed=78)
    runs = []
    for home, ctxs in ((small[0], small[1:]), (None, plain)):
        sync()
        S = DeviceShards.encode(kind, sh["off"], d_ids, ctxs=ctxs, home=home, **shard_args(kind))
        sync()
        assert np.array_equal(S.owner, owner)
        inv = zeros1()
        d_ln, d_add = dev_i64(ln_a), dev(add)
        sync()
        S1, lab = S.append(d_ln, d_add, labels=True, invalid=inv, **({} if kind == "packed" else {"want_perm": True}))
        sync()
        R, moved = S1.rebalance(want_perm=kind != "packed")
        sync()
        mis, inv_r = zeros1(), zeros1()
        d_lr, d_rm = dev_i64(ln_r), dev(rm)
        sync()
        S2, mask = S.remove(d_lr, d_rm, removed=True, missing=mis, invalid=inv_r, **({} if kind == "packed" else {"want_perm": True}))
        sync()
        runs.append(dict(S=S, S1=S1, R=R, S2=S2, moved=moved, lab=lab.cpu().numpy(), inv=int(inv.item()), mask=mask.cpu().numpy(),
                         counts=(int(mis.item()), int(inv_r.item()))))
    a, b = runs
    for key in ("S", "S1", "R", "S2"):
        same_shards(shard_images(kind, a[key]), shard_images(kind, b[key]), f"{what} {key}: one CU against ordinary contexts")
    # encode: the unsharded reference
    sync()
    assert np.array_equal(a["S"].decode_all().cpu().numpy().view(np.uint64), flat), f"{what}: decode_all"
    check_requests(kind, a["S"], sh, flat, what)
    # append: the merged lists
    m = ar.merge(sh["off"], flat, ln_a, add)
    assert a["inv"] == b["inv"] == m.invalid
    want_lab = ar.labels(kind, m, oracle)
    assert np.array_equal(a["lab"], want_lab) and np.array_equal(b["lab"], want_lab), f"{what}: append labels"
    single = encode(kind, m.offsets, m.ids, None)
    sync()
    merged_dec = single.decode_all().cpu().numpy()
    assert np.array_equal(a["S1"].decode_all().cpu().numpy(), merged_dec), f"{what}: decode_all after the append"
    assert a["S1"].compressed_bytes == single.compressed_bytes
    # rebalance: the model's map, the same answers
    sizes1 = (m.offsets[1:] - m.offsets[:-1]).astype(np.int64)
    model = rb.Rebalance(sizes1, 2, owner)
    R = a["R"]
    assert np.array_equal(R.owner, model.new_owner) and np.array_equal(R.local_no, model.new_local), f"{what}: the re-balanced map"
    assert np.array_equal(R.loads, model.loads.astype(np.uint64)) and a["moved"] == b["moved"] == model.moved_ids and model.moved_ids > 0
    sync()
    assert np.array_equal(R.decode_all().cpu().numpy(), merged_dec), f"{what}: decode_all after the re-balance"
    req = np.arange(sizes1.size)[::-1].astype(np.uint64)
    got, ro = R.decode_lists(req)
    want, wo = single.decode_lists(req)
    sync()
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(ro, wo), f"{what}: decode_lists after the re-balance"
    # remove: the surviving lists
    r = remove_ref.remove(sh["off"], flat, ln_r, rm)
    for run in runs:
        assert np.array_equal(run["mask"], r.mask) and run["counts"] == (r.missing, r.invalid), f"{what}: remove mask / counts"
    left = encode(kind, r.offsets, r.ids, None)
    sync()
    assert np.array_equal(a["S2"].decode_all().cpu().numpy(), left.decode_all().cpu().numpy()), f"{what}: decode_all after the remove"
    assert a["S2"].compressed_bytes == left.compressed_bytes
    for c in plain:
        c.synchronize()
