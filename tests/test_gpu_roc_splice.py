"""The seams of the one ROC splice (roc_splice, csrc/roc.hip), pinned in one place.

Append, remove, subset, merge, regroup and update_rows all end in the same three kernels -- k_roc_regroup_meta (a thread per list, the
non-empty count through a wavefront ballot), one scan launch set (tiles of VIDC_SCAN_TILE = 4096 lists), k_roc_regroup_copy and
k_roc_regroup_perm (a wavefront per chunk of APP_COPY_UNIT = 1024 words / ids of one list) -- and differ in the lookup that says where
a list comes from.  The shapes sit at the edges of those kernels:

* nlist in {0, 1, 63, 64, 65, 4096, 4097}: a partly filled last wavefront of the ballot, one and two scan tiles;
* lists whose stream is exactly 1023, 1024 and 1025 words (found with the CPU oracle) and lists of 1023, 1024 and 1025 ids, each
  once as a list the new object takes from an old object and once as a list it takes from the small object of re-encoded lists;
* every list from the small object, none (the small object does not exist), and only the small object's trailing empty list
  (the positional subset that empties one list);
* update_rows growing N past the batch: rows without a source in the last, partial wavefront.

Every result is compared with the encoder's own object of the expected lists (metadata and words), the host reference of the offsets
and of the decode order (append_ref, remove_ref, rows_update_ref, the CPU oracle), the size invariants, the permutation contract, and
-- list by list -- the words of the source object for every list that was not re-encoded.  The file runs twice: on the default context
and on a context sized for one compute unit (as tests/test_gpu_small_grid.py), where the grid-stride loops take more than one trip.
"""
import numpy as np
import pytest

import append_ref as ar
import contract_ref as cr
import remove_ref
import rows_ref as rr
import rows_update_ref as ru

pytestmark = pytest.mark.gpu

NLISTS = (0, 1, 63, 64, 65, 4096, 4097)
EDGES = (1023, 1024, 1025)
LOW = 1 << 30  # the lists' own ids lie below; the ids a remove / an id-range subset takes away again lie at or above
KEYS = ("sizes", "precision", "heads", "nwords", "mt_draws")


# ------------------------------------------------------------------------------------------------------------------ shapes (CPU side)
def csr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.uint64)


def tiny_lists(nlist, seed, lo=0):
    """lo .. 3 distinct ids 6 k + 3 per list, every id in one list only"""
    rng = np.random.default_rng(seed)
    return [(6 * (8 * l + rng.permutation(8)[: rng.integers(lo, 4)]) + 3).astype(np.uint64) for l in range(nlist)]


_POOL, _EDGE = {}, {}


def pool(seed):
    if seed not in _POOL:
        rng = np.random.default_rng(seed)
        _POOL[seed] = rng.permutation(np.unique(rng.integers(1 << 20, LOW, 4000).astype(np.uint64)))
    return _POOL[seed]


def nwords_of(oracle, li):
    return oracle.roc_encode(li, oracle.list_precision(li))["words"].size


def word_list(oracle, target):
    """a list whose ROC stream is exactly `target` words: a prefix of a fixed random pool (about 0.6 words an id)"""
    p = pool(target)
    n, seen = int(target / 0.65), set()
    while nwords_of(oracle, p[:n]) != target:
        assert n not in seen and 0 < n < p.size, f"no prefix of the pool encodes to {target} words"
        seen.add(n)
        n += 1 if nwords_of(oracle, p[:n]) < target else -1
    return p[:n].copy()


def edge_lists(oracle):
    """70 lists (a full wavefront and one of six lanes): tiny ones, and at W / I the lists of 1023, 1024, 1025 words / ids"""
    if not _EDGE:
        lists = tiny_lists(70, 70, lo=1)
        W, I = dict(zip(EDGES, (3, 41, 64))), dict(zip(EDGES, (7, 33, 69)))
        for n in EDGES:
            lists[W[n]] = word_list(oracle, n)
            lists[I[n]] = pool(7)[:n].copy()
        _EDGE.update(lists=lists, W=W, I=I, special=sorted(list(W.values()) + list(I.values())))
    return _EDGE


def extra_id(l, j=0):
    """(never a power of two: a list whose largest id is one is lossy under the reference precision, include/vidc.h)"""
    return np.uint64(LOW + 8 * l + j + 1)


# --------------------------------------------------------------------------------------------------------------------------- GPU side
def _torch():
    import torch

    return torch


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


@pytest.fixture(scope="module", params=["default", "one_cu"])
def ctx(request):
    """None (the default context), or a context whose grids are sized for one compute unit, pool poison on"""
    if request.param == "default":
        yield None
        return
    from vector_db_id_compression_amd import _lib as L

    torch = _torch()
    torch.cuda.set_device(0)
    mp = pytest.MonkeyPatch()
    mp.setenv("VIDC_NUM_CU", "1")
    c = L.Context(0)
    mp.undo()
    assert c.num_cu() == 1
    c.set_pool_poison(True)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    sync()
    c.synchronize()
    c.close()


def flat(lists):
    return np.concatenate(list(lists) + [np.zeros(0, np.uint64)]).astype(np.uint64)


def encode(lists, ctx, want_perm=True):
    d = dev(flat(lists))
    sync()
    return _codecs().RocLists.encode(csr([len(l) for l in lists]), d, want_perm=want_perm, ctx=ctx)


def decoded(obj):
    """the object's lists in its own order"""
    sync()
    dec = obj.decode_all().cpu().numpy().view(np.uint64)
    off = obj.offsets.astype(np.int64)
    return [dec[off[l]:off[l + 1]] for l in range(off.size - 1)]


def streams(obj):
    """-> (all words, word offsets)"""
    return obj.all_words(), csr(obj.info()["nwords"]).astype(np.int64)


def same_metadata(info, finfo, sizes, msg):
    """sizes and word counts of every list; precision, head and draws of the lists that hold ids (an empty list has no stream: what
    its other fields hold is not part of the format, tests/test_gpu_small_grid.py check_roc_streams)"""
    ne = np.asarray(sizes) > 0
    for k in KEYS:
        pick = slice(None) if k in ("sizes", "nwords") else ne
        assert np.array_equal(info[k][pick], finfo[k][pick]), msg.format(k)


def check(new, want, oracle, what, kept=(), want_perm=True):
    """new: the operation's object.  want: the expected lists, each in the order the operation states it (what a fresh encode takes).
    kept: (list of new, source object, list of it) for every list that is not re-encoded."""
    ctx = new.ctx
    sizes = np.array([len(l) for l in want], dtype=np.int64)
    fresh = encode(want, ctx)
    sync()
    info, finfo = new.info(), fresh.info()
    assert np.array_equal(new.offsets, csr(sizes)), f"{what}: offsets differ from the host reference"
    same_metadata(info, finfo, sizes, f"{what}: {{}} differs from the encoder's object of the expected lists")
    words = new.all_words()
    assert np.array_equal(words, fresh.all_words()), f"{what}: the words differ from the encoder's object of the expected lists"
    assert int(info["nwords"].astype(np.int64).sum()) == new.total_words == words.size, f"{what}: total_words"
    assert new.compressed_bytes == 8 * int((sizes > 0).sum()) + 4 * new.total_words, f"{what}: compressed_bytes"
    assert new.ntotal == int(sizes.sum()), f"{what}: ntotal"
    order = [oracle.roc_encode(l, oracle.list_precision(l))["order"] if l.size else l for l in want]
    sync()
    assert np.array_equal(new.decode_all().cpu().numpy().view(np.uint64), flat(order)), f"{what}: decode_all differs from the oracle's order"
    assert new.last_decode_nonclean == 0
    off = csr(sizes).astype(np.int64)
    if want_perm:
        perm = new.perm().astype(np.int64)
        start = np.repeat(off[:-1], sizes)
        key = np.sort(start * (1 << 32) + perm)  # (sorted inside every list: the positions 0 .. n - 1 of that list)
        assert np.array_equal(key - start * (1 << 32), np.arange(perm.size) - start), f"{what}: not a permutation of each list's positions"
    woff = csr(info["nwords"]).astype(np.int64)
    cache = {}
    for j, src, k in kept:
        if id(src) not in cache:
            cache[id(src)] = streams(src)
        sw, so = cache[id(src)]
        assert np.array_equal(words[woff[j]:woff[j + 1]], sw[so[k]:so[k + 1]]), f"{what}: list {j} is not list {k} of its source, word for word"
        if want_perm:
            assert np.array_equal(perm[off[j]:off[j + 1]], np.arange(sizes[j])), f"{what}: the permutation of the kept list {j} is not the identity"
    return fresh


def touch_sets(lists, special=()):
    """name -> the lists an operation re-encodes: every one, none, the special ones and a few others, the others alone"""
    n = len(lists)
    some = set(range(0, n, 3)) | {n - 1} if n else set()
    return {"all": set(range(n)), "none": set(), "special": (some | set(special)), "others": some - set(special)}


# ----------------------------------------------------------------------------------------------------------------------------- append
def run_append(lists, touched, ctx, oracle, what):
    """the touched lists lose their last ids (all of them for every third one: a list that was empty), the batch brings them back"""
    cut = {l: (len(lists[l]) if l % 3 == 0 else min(2, len(lists[l]))) for l in touched}
    old_lists = [li[: len(li) - cut.get(l, 0)] for l, li in enumerate(lists)]
    old = encode(old_lists, ctx)
    ln = np.concatenate([np.full(cut[l], l, np.int64) for l in sorted(touched)] + [np.zeros(0, np.int64)])
    add = flat([lists[l][len(lists[l]) - cut[l]:] for l in sorted(touched)])
    r = np.random.default_rng(len(lists)).permutation(ln.size)
    ln, add = ln[r], add[r]
    old_dec = decoded(old)
    new, lab = old.append(dev_i64(ln), dev(add), want_perm=True)
    sync()
    m = ar.merge(old.offsets, flat(old_dec), ln, add)
    mo = m.offsets.astype(np.int64)
    want = [m.ids[mo[l]:mo[l + 1]] for l in range(len(lists))]
    really = {l for l in touched if cut[l]}
    check(new, want, oracle, what, kept=[(l, old, l) for l in range(len(lists)) if l not in really])
    assert np.array_equal(lab.cpu().numpy(), ar.labels("roc", m, oracle)), f"{what}: labels"


@pytest.mark.parametrize("nlist", NLISTS)
def test_append_at_every_list_count(ctx, oracle, nlist):
    lists = tiny_lists(nlist, nlist)
    for name, t in touch_sets(lists).items():
        run_append(lists, t, ctx, oracle, f"append nlist={nlist} touched={name}")


@pytest.mark.parametrize("which", ["special", "others"])
def test_append_chunk_edges(ctx, oracle, which):
    """special: the 1023 / 1024 / 1025 word and id lists are what the append produces (from the small object); others: they are kept"""
    e = edge_lists(oracle)
    run_append(e["lists"], touch_sets(e["lists"], e["special"])[which], ctx, oracle, f"append edges {which}")


# ------------------------------------------------------------------------------------------------------------------ remove and subset
def with_extras(lists, touched):
    """every touched list also holds one or two ids >= LOW (an empty list: only those)"""
    return [np.concatenate([li, [extra_id(l, j) for j in range(1 + l % 2)]]).astype(np.uint64) if l in touched else li
            for l, li in enumerate(lists)]


def run_remove(lists, touched, ctx, oracle, what, any_list):
    from vector_db_id_compression_amd import removal

    old = encode(with_extras(lists, touched), ctx)
    ln = np.array([l for l in sorted(touched) for _ in range(1 + l % 2)] + [0] * (2 if lists else 0), dtype=np.int64)
    rm = np.array([extra_id(l, j) for l in sorted(touched) for j in range(1 + l % 2)] + [extra_id(len(lists), j) for j in range(ln.size and 2)],
                  dtype=np.uint64)  # (the last two pairs name ids that no list holds: missing)
    old_dec = decoded(old)
    new, mask = removal.remove(old, None if any_list else dev_i64(ln), dev(rm), want_perm=True)
    sync()
    m = remove_ref.remove(old.offsets, flat(old_dec), None if any_list else ln, rm)
    assert np.array_equal(mask.cpu().numpy()[: m.mask.size], m.mask), f"{what}: the removed mask"
    mo = m.offsets.astype(np.int64)
    check(new, [m.ids[mo[l]:mo[l + 1]] for l in range(len(lists))], oracle, what, kept=[(l, old, l) for l in range(len(lists)) if l not in touched])


def run_subset_by_id(lists, touched, ctx, oracle, what):
    from vector_db_id_compression_amd import subset

    old = encode(with_extras(lists, touched), ctx)
    old_dec = decoded(old)
    new, mask = subset.subset(old, subset.ID_RANGE, 0, LOW, want_perm=True)
    sync()
    assert np.array_equal(mask.cpu().numpy()[: old.ntotal], (flat(old_dec) < LOW).astype(np.uint8)), f"{what}: the taken mask"
    check(new, [li[li < LOW] for li in old_dec], oracle, what, kept=[(l, old, l) for l in range(len(lists)) if l not in touched])


@pytest.mark.parametrize("nlist", NLISTS)
def test_remove_and_subset_by_id_at_every_list_count(ctx, oracle, nlist):
    lists = tiny_lists(nlist, nlist + 1)
    for name, t in touch_sets(lists).items():
        run_remove(lists, t, ctx, oracle, f"remove nlist={nlist} touched={name}", any_list=name == "all")
        run_subset_by_id(lists, t, ctx, oracle, f"subset by id nlist={nlist} touched={name}")


@pytest.mark.parametrize("which", ["special", "others"])
def test_remove_and_subset_by_id_chunk_edges(ctx, oracle, which):
    e = edge_lists(oracle)
    t = touch_sets(e["lists"], e["special"])[which]
    run_remove(e["lists"], t, ctx, oracle, f"remove edges {which}", any_list=False)
    run_subset_by_id(e["lists"], t, ctx, oracle, f"subset by id edges {which}")


def run_subset_positional(lists, stype, a1, a2, ctx, oracle, what):
    """INVLIST: the lists outside a1 .. a2 keep nothing; INVLIST_FRACTION: every list keeps its positions n a2 // a1 .. n (a2 + 1) // a1"""
    from vector_db_id_compression_amd import subset

    old = encode(lists, ctx)
    old_dec = decoded(old)
    new, mask = subset.subset(old, stype, a1, a2, want_perm=True)
    sync()
    if stype == subset.INVLIST:
        bounds = [(0, len(li)) if a1 <= l < a2 else (0, 0) for l, li in enumerate(old_dec)]
    else:
        bounds = [(len(li) * a2 // a1, len(li) * (a2 + 1) // a1) for li in old_dec]
    want = [li[i1:i2] for li, (i1, i2) in zip(old_dec, bounds)]
    taken = flat([(np.arange(len(li)) >= i1) & (np.arange(len(li)) < i2) for li, (i1, i2) in zip(old_dec, bounds)]).astype(np.uint8)
    assert np.array_equal(mask.cpu().numpy()[: old.ntotal], taken), f"{what}: the taken mask"
    check(new, want, oracle, what, kept=[(l, old, l) for l, li in enumerate(old_dec) if len(want[l]) == len(li)])


@pytest.mark.parametrize("nlist", NLISTS)
def test_subset_positional_at_every_list_count(ctx, oracle, nlist):
    """the last list alone emptied (the only flagged list takes the small object's trailing empty list); nothing emptied; everything
    emptied; half of every list (every list of two ids and more from the small object, the lists of one id from its empty list)"""
    from vector_db_id_compression_amd import subset

    lists = tiny_lists(nlist, nlist + 2, lo=1)
    for a1, a2 in ((0, max(nlist - 1, 0)), (0, nlist), (nlist, nlist)):
        run_subset_positional(lists, subset.INVLIST, a1, a2, ctx, oracle, f"subset INVLIST {a1} .. {a2} of {nlist}")
    run_subset_positional(lists, subset.INVLIST_FRACTION, 2, 1, ctx, oracle, f"subset INVLIST_FRACTION 2, 1 nlist={nlist}")


def test_subset_positional_chunk_edges(ctx, oracle):
    """the long lists kept whole (from the old object) next to emptied ones, and cut to halves (from the small object)"""
    from vector_db_id_compression_amd import subset

    e = edge_lists(oracle)
    run_subset_positional(e["lists"], subset.INVLIST, 3, 70, ctx, oracle, "subset INVLIST edges")
    # doubled lists: the upper half of each is a list of 1023 / 1024 / 1025 ids taken from the small object
    lists = list(e["lists"])
    for n in EDGES:
        lists[e["I"][n]] = pool(8)[: 2 * n].copy()
    run_subset_positional(lists, subset.INVLIST_FRACTION, 2, 1, ctx, oracle, "subset INVLIST_FRACTION edges")


# ------------------------------------------------------------------------------------------------------------------------------ merge
def run_merge(lists, touched, ctx, oracle, what):
    """a touched list of two ids and more is split between a and b (re-encoded); the others lie in a or in b alone (kept: add_id 0)"""
    from vector_db_id_compression_amd import merge

    la, lb, kept_from = [], [], {}
    for l, li in enumerate(lists):
        if l in touched and len(li) >= 2:
            h = 1 if len(li) < 8 else len(li) - 3
            la.append(li[:h]); lb.append(li[h:])
        elif l % 2:
            la.append(li[:0]); lb.append(li); kept_from[l] = 1
        else:
            la.append(li); lb.append(li[:0]); kept_from[l] = 0
    a, b = encode(la, ctx), encode(lb, ctx)
    da, db = decoded(a), decoded(b)
    torch = _torch()
    src = torch.empty(a.ntotal + b.ntotal, dtype=torch.int64, device="cuda")
    new = merge.merge(a, b, 0, src=src, want_perm=True)
    sync()
    want = [np.concatenate([x, y]) for x, y in zip(da, db)]
    check(new, want, oracle, what, kept=[(l, (a, b)[s], l) for l, s in kept_from.items()])
    # src leads every entry of the new object back to its id
    s = src.cpu().numpy()
    both = np.concatenate([flat(da), flat(db)])
    sync()
    assert np.array_equal(new.decode_all().cpu().numpy().view(np.uint64), both[np.where(s >= 0, s, a.ntotal + ~s)]), f"{what}: src"


@pytest.mark.parametrize("nlist", NLISTS)
def test_merge_at_every_list_count(ctx, oracle, nlist):
    lists = tiny_lists(nlist, nlist + 3, lo=2)
    for name, t in touch_sets(lists).items():
        run_merge(lists, t, ctx, oracle, f"merge nlist={nlist} touched={name}")


@pytest.mark.parametrize("which", ["special", "others"])
def test_merge_chunk_edges(ctx, oracle, which):
    e = edge_lists(oracle)
    run_merge(e["lists"], touch_sets(e["lists"], e["special"])[which], ctx, oracle, f"merge edges {which}")


# ---------------------------------------------------------------------------------------------------------------------------- regroup
def run_regroup(srcs_lists, src_no, list_no, ctx, oracle, what):
    cd = _codecs()
    srcs = [encode(ls, ctx) for ls in srcs_lists]
    dec = [decoded(s) for s in srcs]
    new = cd.roc_regroup(srcs, src_no, list_no, want_perm=True, ctx=ctx)
    sync()
    want = [dec[s][k] for s, k in zip(src_no, list_no)]
    check(new, want, oracle, what, kept=[(j, srcs[s], int(k)) for j, (s, k) in enumerate(zip(src_no, list_no))])


@pytest.mark.parametrize("m", NLISTS)
def test_regroup_at_every_list_count(ctx, oracle, m):
    """m lists drawn from two sources of 50 and 77 lists, with repeats"""
    rng = np.random.default_rng(m)
    srcs = [tiny_lists(50, 50), tiny_lists(77, 77)]
    src_no = rng.integers(0, 2, m).astype(np.uint32)
    list_no = (rng.integers(0, 50, m) + 27 * src_no * rng.integers(0, 2, m)).astype(np.uint64)
    run_regroup(srcs, src_no, list_no, ctx, oracle, f"regroup m={m}")


def test_regroup_chunk_edges(ctx, oracle):
    e = edge_lists(oracle)
    rng = np.random.default_rng(5)
    list_no = np.concatenate([rng.permutation(70), e["special"]]).astype(np.uint64)
    src_no = (np.arange(list_no.size) % 2).astype(np.uint32)
    run_regroup([e["lists"], e["lists"][::-1]], src_no, np.where(src_no == 0, list_no, 69 - list_no).astype(np.uint64), ctx, oracle, "regroup edges")


# ------------------------------------------------------------------------------------------------------------------------ update_rows
@pytest.mark.parametrize("n_old,n_new", [(1, 1), (60, 63), (60, 64), (60, 65), (4090, 4096), (4090, 4097), (4097, 4097)])
def test_update_rows_at_every_row_count(ctx, oracle, n_old, n_new):
    """the batch names a third of the old rows and, where the graph grows, its first new node alone: every other new node has no source
    (RocUpdateSlots answers "nowhere"), in the last wavefront -- a partial one for 63, 65 and 4097 rows"""
    cd = _codecs()
    torch = _torch()
    K = 16
    rows = rr.family("uniform", max(n_old, 1), K, seed=n_old)[:n_old]
    nodes = np.concatenate([np.arange(0, n_old, 3), [n_old] if n_new > n_old else []]).astype(np.int64)
    batch = rr.family("uniform", max(n_old, 1), K, seed=n_new + 1, nrows=max(nodes.size, 1))[: nodes.size]
    R, invalid, _ = ru.update_rows(rows, nodes, batch, n_new)
    assert invalid == 0
    g = cd.RocLists.encode_rows(torch.from_numpy(rows).cuda().reshape(n_old, K), ctx=ctx)
    sync()
    new = cd.update_rows(g, dev_i64(nodes), torch.from_numpy(batch).cuda().reshape(nodes.size, K), n_new=n_new)
    fresh = cd.RocLists.encode_rows(torch.from_numpy(R).cuda(), ctx=ctx)
    sync()
    what = f"update_rows {n_old} -> {n_new}"
    info, finfo = new.info(), fresh.info()
    counts = (R >= 0).sum(axis=1)
    assert np.array_equal(info["sizes"], counts) and np.array_equal(new.offsets, csr(counts)), f"{what}: sizes / offsets differ from the host reference"
    same_metadata(info, finfo, counts, f"{what}: {{}} differs from the encoder's object of the updated rows")
    words = new.all_words()
    assert np.array_equal(words, fresh.all_words()), f"{what}: the words differ from the encoder's object of the updated rows"
    assert int(info["nwords"].astype(np.int64).sum()) == new.total_words == words.size
    assert new.compressed_bytes == 8 * int((counts > 0).sum()) + 4 * new.total_words and new.ntotal == int(counts.sum())
    out, cnt = new.decode_rows(None, K)
    want, want_cnt = cr.RowRef("roc", R, oracle).expected(None, K)  # (the oracle's decode of every updated row, its lossy cases included)
    sync()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cnt, want_cnt) and np.array_equal(cnt, counts), f"{what}: decode_rows"
    gw, go = streams(g)
    woff = csr(info["nwords"]).astype(np.int64)
    named = set(nodes.tolist())
    for i in range(n_old):
        if i not in named:
            assert np.array_equal(words[woff[i]:woff[i + 1]], gw[go[i]:go[i + 1]]), f"{what}: the untouched row {i} lost its words"
