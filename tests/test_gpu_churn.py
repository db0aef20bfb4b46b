"""Chains of add, remove and locate on one object: every id keeps its payload.

Every entry carries a payload that is a function of its id alone (churn_ref.code: the bytes of id * 0x9E3779B97F4A7C15), so a row of
codes_all that is shifted, swapped or left behind by a mutation cannot match by accident.  One designed chain of twelve steps
(tests/churn_ref.py; tests/test_churn_ref_cpu.py asserts what it contains) runs on every container of custom_invlists, on sharded
objects at the codec level, and a shorter one on the IVF index against a twin on plain lists.  After EVERY step the whole object is
compared with the numpy model: codes, offsets, list contents and order, a locate sample through every lookup the containers have, and
the size attributes of a from-scratch object; at the last step the codec image equals the from-scratch encode word for word.  Every
comparison is exact.  The chains also run with the pool poison on, the blocks of every predecessor handed out again in between."""
import functools

import numpy as np
import pytest

import churn_ref as ch
from test_gpu_append import dev_i64, encode, image
from test_gpu_dev_offsets import dev
from test_gpu_remove import check_roundtrips, zeros1

pytestmark = pytest.mark.gpu

CONTAINERS = {"packed-bits": ("packed", "dense"), "elias-fano": ("ef", "sparse"), "roc": ("roc", "sparse"),
              "wavelet-tree": ("wt", "perm"), "wavelet-tree-1": ("wt1", "perm")}
SIZE_ATTRS = ("compressed_ids_size_in_bytes", "codes_size_in_bytes", "bits", "id_symbol_precision", "overhead_in_bytes")
GOLDEN_I64 = ch.GOLDEN - (1 << 64)  # the multiplier as the int64 the device multiplies by (the product wraps as in churn_ref.code)


def _torch():
    import torch

    return torch


def _lib():
    from vector_db_id_compression_amd import _lib

    return _lib


def _ci():
    from vector_db_id_compression_amd import custom_invlists

    return custom_invlists


@functools.lru_cache(maxsize=None)
def schedule(scheme):
    return ch.schedule(scheme)


def dev_ids(a):
    a = np.asarray(a, dtype=np.uint64)
    return dev(a) if a.size else _torch().zeros(0, dtype=_torch().int64, device="cuda")


def dev_code(ids):
    """payload of an int64 CUDA tensor of ids, on the device"""
    return ids * GOLDEN_I64


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


class poison:
    """the pool poison of the default context: a block handed out again is filled with 0xFF first"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        L = _lib()
        L.check(L.lib().vidc_ctx_debug_pool_poison(L.default_context().h, 1 if self.on else 0))

    def __exit__(self, *exc):
        L = _lib()
        _torch().cuda.synchronize()
        L.check(L.lib().vidc_ctx_debug_pool_poison(L.default_context().h, 0))


def recycle(kind, model, bits=None):
    """one throw-away object of the model's size: the blocks the last step freed are handed out again, poisoned, and freed"""
    ids = model.ids()
    if kind.startswith("wt"):  # (a tree wants a permutation, ascending inside every list: the model's ids by rank)
        rank = np.empty(ids.size, np.uint64)
        rank[np.argsort(ids, kind="stable")] = np.arange(ids.size, dtype=np.uint64)
        off = model.offsets().astype(np.int64)
        for l in range(model.nlist):
            rank[off[l]:off[l + 1]].sort()
        ids = rank
    junk = encode(kind, model.offsets(), ids, True, bits)
    junk.decode_all()
    del junk
    _torch().cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- the containers
def build_container(name, lists):
    from vector_db_id_compression_amd.invlists import ArrayInvertedLists

    ci = _ci()
    il = ArrayInvertedLists(len(lists), ch.CODE_SIZE)
    for l, li in enumerate(lists):
        if li.size:
            il.add_entries(l, li.view(np.int64), ch.code(li).view(np.uint8).reshape(-1, ch.CODE_SIZE))
    if name == "wavelet-tree-1":
        return ci.CompressedIDInvertedListsWaveletTree(il, 1)
    return ci.AVAILABLE_COMPRESSED_IVFS[name](il)


def locate_sample(scheme, model, touched, removed_pairs, step_no):
    """(list numbers, ids): every id of the touched lists, 200 ids of the others, every pair removed so far, 50 ids that never were"""
    rng = np.random.default_rng(1000 + step_no)
    ln = [np.full(model.lists[l].size, l, np.int64) for l in touched]
    ids = [model.lists[l] for l in touched]
    rest = [l for l in range(model.nlist) if l not in touched]
    if rest:
        rl = np.concatenate([np.full(model.lists[l].size, l, np.int64) for l in rest])
        ri = np.concatenate([model.lists[l] for l in rest])
        pick = rng.choice(ri.size, min(200, ri.size), replace=False)
        ln.append(rl[pick])
        ids.append(ri[pick])
    if removed_pairs:
        ln.append(np.array([p[0] for p in removed_pairs], np.int64))
        ids.append(np.array([p[1] for p in removed_pairs], np.uint64))
    ln.append(np.arange(50, dtype=np.int64) % model.nlist)
    ids.append(ch.never(scheme, 50))
    ln, ids = np.concatenate(ln), np.concatenate(ids).astype(np.uint64)
    order = rng.permutation(ln.size)
    return ln[order], ids[order]


def check_container(name, il, model, touched, removed_pairs, step_no, oracle, last=False):
    torch = _torch()
    kind, scheme = CONTAINERS[name]
    what = f"{name} step {step_no}"
    off = model.offsets()
    o = off.astype(np.int64)
    # -- offsets
    assert np.array_equal(np.asarray(il._offsets).astype(np.uint64), off), f"{what}: offsets"
    assert il.ntotal == model.ntotal == il.compute_ntotal() and [il.list_size(l) for l in range(model.nlist)] == model.sizes().tolist()
    # -- codes: every row carries the payload of the id the container reports for it
    ids_all = il.get_ids_all()
    assert ids_all.numel() == model.ntotal and tuple(il.codes_all.shape) == (model.ntotal, ch.CODE_SIZE)
    rows = il.codes_all.view(torch.int64).reshape(-1)
    bad = int((rows != dev_code(ids_all)).sum().item())
    assert bad == 0, f"{what}: {bad} rows of codes_all carry another id's payload"
    # -- list contents
    dec = ids_all.cpu().numpy().view(np.uint64)
    for l in range(model.nlist):
        got, want = dec[o[l]:o[l + 1]], model.lists[l]
        if kind == "roc":
            assert np.array_equal(np.sort(got), np.sort(want)), f"{what}: list {l} holds other ids"
        elif kind == "ef":
            assert np.array_equal(got, np.sort(want)), f"{what}: list {l} is not the model's ids, ascending"
        else:
            assert np.array_equal(got, want), f"{what}: list {l} is not in the model's order"
    if kind == "roc":
        check_roundtrips(oracle, off, model.ids())
    # -- the locate sample, through every lookup
    ln, ids = locate_sample(scheme, model, touched, removed_pairs, step_no)
    d_off = torch.from_numpy(o).cuda()
    for mode in ("any", "pairs"):
        held = model.find(None if mode == "any" else ln, ids)
        labels = il.locate_batch(None if mode == "any" else dev_i64(ln), dev_ids(ids))
        lab = labels.cpu().numpy()
        assert np.array_equal(lab < 0, held < 0), f"{what} ({mode}): -1 for other ids than the absent ones"
        hit = held >= 0
        assert hit.sum() >= 200 and (~hit).sum() >= 50
        ll, oo = lab[hit] >> 32, lab[hit] & 0xFFFFFFFF
        assert np.array_equal(ll, held[hit]), f"{what} ({mode}): a label names another list"
        assert (oo < model.sizes()[ll]).all()
        if kind != "roc":  # the place inside the list is the model's
            for l in np.unique(ll):
                li = model.lists[l] if kind != "ef" else np.sort(model.lists[l])
                assert np.array_equal(oo[ll == l], ch.positions(li, ids[hit][ll == l])), f"{what} ({mode}): offsets in list {l}"
        want = ids[hit].view(np.int64)
        d_lab = labels[torch.from_numpy(hit).cuda()]
        assert np.array_equal(il.translate_labels(d_lab).cpu().numpy(), want), f"{what} ({mode}): translate_labels"
        assert np.array_equal(host(il.get_single_ids(ll, oo)), want), f"{what} ({mode}): get_single_ids"
        uniq, slot = np.unique(ll, return_inverse=True)
        assert np.array_equal(host(il.decode_gather(uniq, slot.reshape(-1), oo)), want), f"{what} ({mode}): decode_gather"
        got = il.codes_all[d_off[d_lab >> 32] + (d_lab & 0xFFFFFFFF)].view(torch.int64).reshape(-1).cpu().numpy()
        assert np.array_equal(got, ch.code(ids[hit])), f"{what} ({mode}): codes_all at the labels"
    # -- the size attributes of a from-scratch object over the same lists in the same order
    own = [dec[o[l]:o[l + 1]] for l in range(model.nlist)]
    if kind == "packed":  # (at the codec level: the constructor refuses the ids >= ntotal that survive a removal)
        from vector_db_id_compression_amd.codecs import PackedLists

        scratch = PackedLists.encode(off, dev_ids(dec), bits=il.bits)
        assert (il.bits, il.compressed_ids_size_in_bytes) == (scratch.bits, scratch.compressed_bytes), f"{what}: size attributes"
        assert torch.equal(scratch.decode_all(), ids_all)
        for a in SIZE_ATTRS[1:]:
            assert a == "bits" or not hasattr(il, a)
    else:
        scratch = build_container(name, own)
        for a in SIZE_ATTRS:
            assert np.array_equal(np.asarray(getattr(il, a, None)), np.asarray(getattr(scratch, a, None))), f"{what}: {a}"
        assert torch.equal(scratch.get_ids_all(), ids_all), f"{what}: a from-scratch container decodes in another order"
        assert torch.equal(scratch.codes_all, il.codes_all), f"{what}: a from-scratch container keeps other codes"
    # -- the codec image, word for word (the permutation is over the last call's input: left out, as in test_gpu_append)
    if last:
        once = encode(kind, off, model.ids(), True, il.bits if kind == "packed" else None)
        a, b = image(kind, il._c, False), image(kind, once, False)
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), f"{what}: {k} differs from the from-scratch encode"


def run_container_chain(name, poisoned, oracle):
    torch = _torch()
    kind, scheme = CONTAINERS[name]
    init, steps = schedule(scheme)
    model = ch.Model(init)
    il = build_container(name, init)
    removed_pairs = []
    widths = []
    for no, st in enumerate(steps):
        if st.kind == "add":
            before = image(kind, il._c, False) if st.name == "empty" else None
            codes_before = il.codes_all.cpu().numpy() if st.name == "empty" else None
            payload = torch.from_numpy(ch.code(st.ids).view(np.uint8).reshape(-1, ch.CODE_SIZE).copy()).cuda()
            labels = il.add_batch(dev_i64(st.list_nos), dev_ids(st.ids), payload)
            assert model.add(st.list_nos, st.ids) == st.touched
            assert np.array_equal(labels.cpu().numpy() < 0, st.list_nos < 0), f"{name}: labels of the skipped pairs"
            if st.name == "empty":
                after = image(kind, il._c, False)
                assert all(np.array_equal(np.asarray(before[k]), np.asarray(after[k])) for k in before), f"{name}: an empty batch changed the object"
                assert np.array_equal(il.codes_all.cpu().numpy(), codes_before)
                del after
            del payload, labels, before, codes_before
        elif st.kind == "remove":
            was = model.copy()
            n = il.remove_batch(None if st.list_nos is None else dev_i64(st.list_nos), dev_ids(st.ids))
            c = model.remove(st.list_nos, st.ids)
            assert n == c.removed == st.expect.removed, f"{name} {st.name}: removed {n}, the model {c.removed}"
            for l in c.touched:
                removed_pairs += [(l, int(v)) for v in np.setdiff1d(was.lists[l], model.lists[l])]
        assert np.array_equal(model.sizes(), st.sizes)
        if poisoned:
            recycle(kind, model, il.bits if kind == "packed" else None)
        check_container(name, il, model, st.touched, removed_pairs, no, oracle, last=no == len(steps) - 1)
        widths.append(getattr(il, "bits", None))
    if kind == "packed":  # 14 bits until the ids ever handed out pass 16 384 (ntotal never does before), then 15 for good
        assert widths == [14] * ch.S_ADD_600 + [15] * (len(steps) - ch.S_ADD_600), widths
    if kind.startswith("wt"):
        with pytest.raises(RuntimeError, match="permutation"):
            il.remove_batch(None, dev_ids(model.lists[0][:2]))
        check_container(name, il, model, [], removed_pairs, len(steps), oracle)


@pytest.mark.parametrize("poisoned", [False, True], ids=["plain", "pool_poison"])
@pytest.mark.parametrize("name", list(CONTAINERS))
def test_container_chain(name, poisoned, oracle):
    with poison(poisoned):
        run_container_chain(name, poisoned, oracle)


@pytest.mark.parametrize("poisoned", [False, True], ids=["plain", "pool_poison"])
@pytest.mark.parametrize("hook", ["VIDC_FORCE_GENERAL", "VIDC_NO_LANE"])
def test_roc_chain_on_the_other_kernel_families(hook, poisoned, oracle, monkeypatch):
    for h in ("VIDC_FORCE_GENERAL", "VIDC_NO_LANE"):
        monkeypatch.delenv(h, raising=False)
    monkeypatch.setenv(hook, "1")
    with poison(poisoned):
        run_container_chain("roc", poisoned, oracle)


# ------------------------------------------------------------------------------------------------------------- sharded objects
SHARD_KINDS = {"packed": "dense", "ef": "sparse", "roc": "sparse"}
PACKED_SHARD_BITS = 15  # every id the dense chain hands out is below 2^15


def _gather_by_perm(torch, merged, sizes, perm):
    """position q of list l holds entry perm[q] of that list's part of `merged`"""
    off = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)])
    base = torch.repeat_interleave(off[:-1], sizes)
    return merged[base + torch.from_numpy(perm.astype(np.int64)).to(merged.device)]


def _codec_args(kind):
    return {} if kind == "packed" else {"want_perm": True}


def _remove(kind, obj, ln, ids, missing, invalid):
    from vector_db_id_compression_amd import removal
    from vector_db_id_compression_amd.sharding import DeviceShards

    if isinstance(obj, DeviceShards):
        return obj.remove(ln, ids, missing=missing, invalid=invalid, **_codec_args(kind))
    return removal.remove(obj, ln, ids, want_perm=True, missing=missing, invalid=invalid)


def run_codec_chain(kind, obj, payload, rebalance_after=()):
    """the schedule on a codec-level object (PackedLists / EfLists / RocLists or DeviceShards); the int64 payload tensor follows in
    object order, moved by nothing but what the calls return -> the last object"""
    torch = _torch()
    init, steps = schedule(SHARD_KINDS[kind])
    model = ch.Model(init)
    nlist = model.nlist
    lists = torch.arange(nlist, device="cuda")

    def sizes_of(o):
        return torch.from_numpy((o.offsets[1:] - o.offsets[:-1]).astype(np.int64)).cuda()

    for no, st in enumerate(steps):
        what = f"{kind} step {no}"
        if st.kind == "add":
            ln, add = dev_i64(st.list_nos), dev_ids(st.ids)
            old_n = sizes_of(obj)
            new, lab = obj.append(ln, add, **_codec_args(kind))
            model.add(st.list_nos, st.ids)
            new_n = sizes_of(new)
            valid = ln >= 0
            assert np.array_equal(lab.cpu().numpy() < 0, st.list_nos < 0)
            # the merged input, list by list: the old object's order, then the batch in batch order
            order = torch.argsort(ln[valid], stable=True)
            batch_l, batch_code = ln[valid][order], dev_code(add[valid][order])
            merged = torch.empty(int(new_n.sum().item()), dtype=torch.int64, device="cuda")
            l_old = torch.repeat_interleave(lists, old_n)
            new_off = torch.cat([new_n.new_zeros(1), torch.cumsum(new_n, 0)])
            old_off = torch.cat([old_n.new_zeros(1), torch.cumsum(old_n, 0)])
            merged[torch.arange(payload.numel(), device="cuda") + (new_off[:-1] - old_off[:-1])[l_old]] = payload
            add_off = (new_off - old_off)[:-1]
            rank = torch.arange(batch_l.numel(), device="cuda") - add_off[batch_l]
            merged[new_off[batch_l] + old_n[batch_l] + rank] = batch_code
            payload = merged if kind == "packed" else _gather_by_perm(torch, merged, new_n, new.perm())
            # (the labels say the same about the batch)
            at = new_off[ln[valid]] + (lab[valid] & 0xFFFFFFFF)
            assert torch.equal(payload[at], dev_code(add[valid])), f"{what}: the labels lead to other rows than the permutation"
            obj = new
            del new, lab, merged
        elif st.kind == "remove":
            mis, inv = zeros1(), zeros1()
            new, mask = _remove(kind, obj, None if st.list_nos is None else dev_i64(st.list_nos), dev_ids(st.ids), mis, inv)
            c = model.remove(st.list_nos, st.ids)
            assert (int(mask.sum().item()), int(mis.item()), int(inv.item())) == (c.removed, c.missing, c.invalid), f"{what}: counts"
            payload = payload[mask == 0]
            if kind != "packed":
                payload = _gather_by_perm(torch, payload, sizes_of(new), new.perm())
            obj = new
            del new, mask
        assert np.array_equal(obj.offsets, model.offsets()), f"{what}: offsets"
        dec = obj.decode_all()
        bad = int((payload != dev_code(dec)).sum().item())
        assert payload.numel() == dec.numel() and bad == 0, f"{what}: {bad} payload rows no longer sit at their id"
        h_dec, o = dec.cpu().numpy().view(np.uint64), model.offsets().astype(np.int64)
        for l in range(nlist):
            got, want = h_dec[o[l]:o[l + 1]], model.lists[l]
            assert np.array_equal(got if kind == "packed" else np.sort(got), want if kind == "packed" else np.sort(want)), f"{what}: list {l}"
        pos = np.arange(no % 7, h_dec.size, 7)
        l_of = np.searchsorted(o, pos, side="right") - 1
        back = obj.translate_labels(dev_i64((l_of << 32) | (pos - o[l_of]))).cpu().numpy().view(np.uint64)
        assert np.array_equal(back, h_dec[pos]), f"{what}: translate_labels"
        if no + 1 in rebalance_after:  # behind the fourth and the ninth step
            new, _moved = obj.rebalance(**_codec_args(kind))
            if kind != "packed":
                sz = model.sizes()
                assert np.array_equal(new.perm(), np.concatenate([np.arange(n) for n in sz]).astype(np.uint32)), f"{what}: rebalance"
            assert torch.equal(new.decode_all(), dec), f"{what}: the re-balanced object decodes differently"
            obj = new
            del new
        del dec
    return obj, model


@pytest.mark.parametrize("kind", list(SHARD_KINDS))
def test_sharded_chain(kind, oracle):
    from vector_db_id_compression_amd.sharding import DeviceShards

    torch = _torch()
    init, _ = schedule(SHARD_KINDS[kind])
    m0 = ch.Model(init)
    off, ids = m0.offsets(), m0.ids()
    if kind == "roc":
        check_roundtrips(oracle, off, ids)
    sizes = torch.from_numpy(m0.sizes()).cuda()
    code0 = torch.from_numpy(ch.code(ids)).cuda()
    args = {"bits": PACKED_SHARD_BITS} if kind == "packed" else {"want_perm": True}
    sh = DeviceShards.encode(kind, off, dev_ids(ids), nshards=3, **args)
    assert sh.nshards == 3 and len(set(sh.owner.tolist())) == 3
    payload = code0 if kind == "packed" else _gather_by_perm(torch, code0, sizes, sh.perm())
    sh, model = run_codec_chain(kind, sh, payload, rebalance_after=(4, 9))
    # the unsharded chain: id for id, list for list
    one = encode(kind, off, ids, True, PACKED_SHARD_BITS if kind == "packed" else None)
    payload = code0 if kind == "packed" else _gather_by_perm(torch, code0, sizes, one.perm())
    one, _ = run_codec_chain(kind, one, payload)
    assert np.array_equal(sh.offsets, one.offsets) and np.array_equal(one.offsets, model.offsets())
    assert torch.equal(sh.decode_all(), one.decode_all()), f"{kind}: the sharded chain ends in other lists than the unsharded one"


# ------------------------------------------------------------------------------------------------------------- the index on top
INDEX_D, INDEX_NLIST, HEAVY = 4, 8, 0
INDEX_BATCHES = ([300] + [100] * 7, [3400] + [480] * 7, [1300] + [243] * 7, [700] + [186] * 7)  # a seed batch, then the three adds


def _index_data():
    rng = np.random.default_rng(61)
    cent = (3.0 * rng.standard_normal((INDEX_NLIST, INDEX_D))).astype(np.float32)
    batches = []
    for counts in INDEX_BATCHES:
        c = np.repeat(np.arange(INDEX_NLIST), counts)
        rng.shuffle(c)
        batches.append((cent[c] + 0.3 * rng.standard_normal((c.size, INDEX_D))).astype(np.float32))
    xq = (cent[rng.integers(0, INDEX_NLIST, 20)] + 0.3 * rng.standard_normal((20, INDEX_D))).astype(np.float32)
    return cent, batches, xq


def _new_index(cent):
    from vector_db_id_compression_amd.ivf import IVFIndex

    idx = IVFIndex(INDEX_D, INDEX_NLIST, "Flat")
    idx.centroids = _torch().from_numpy(cent).cuda()
    idx.nprobe = 3
    idx.parallel_mode = 3
    return idx


def check_index(a, twin, rows, live, gone, xq, what):
    torch = _torch()
    il = a.invlists
    assert a.ntotal == twin.ntotal == il.ntotal == live.size
    assert np.array_equal(np.sort(il.get_ids_all().cpu().numpy()), live), f"{what}: the live ids"
    for l in range(INDEX_NLIST):
        assert il.list_size(l) == twin.invlists.list_size(l)
    # Flat codes: the stored vector of every live id, bit for bit
    order = np.random.default_rng(live.size).permutation(live)
    got = a.reconstruct_batch(torch.from_numpy(order).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.int32), rows[order].view(np.int32)), f"{what}: reconstruct_batch returns another vector"
    for bad in (gone[:1], gone[-1:], np.array([rows.shape[0] + 5])):
        if bad.size:
            with pytest.raises(RuntimeError, match="not in the index"):
                a.reconstruct_batch(np.concatenate([live[:3], bad]).astype(np.int64))
    for search in (lambda i: i.search(xq, 10), lambda i: i.search_defer_id_decoding(xq, 10),
                   lambda i: i.search_defer_id_decoding(xq, 10, decode_1by1=True)):
        Da, Ia = search(a)
        Db, Ib = search(twin)
        assert np.array_equal(Da, Db), f"{what}: distances"
        assert not np.isin(Ia, gone).any(), f"{what}: a removed id came back"
        assert np.isin(Ia[Ia >= 0], live).all()
        for q in range(xq.shape[0]):
            assert sorted(zip(Da[q].tolist(), Ia[q].tolist())) == sorted(zip(Db[q].tolist(), Ib[q].tolist())), (what, q)


@pytest.mark.parametrize("name", ["packed-bits", "elias-fano", "roc", "wavelet-tree"])
def test_index_chain(name):
    """add, remove_ids of 1 500, add, remove_ids with ids of the second batch, add -- in step with a twin on plain lists (the wavelet
    tree: the adds alone, and remove_ids raises)"""
    cent, batches, xq = _index_data()
    rows = np.concatenate(batches)
    a, twin = _new_index(cent), _new_index(cent)
    a.add(batches[0])
    twin.add(batches[0])
    _ci().apply_id_compression(a, name)
    rng = np.random.default_rng(63)
    live, gone = np.arange(batches[0].shape[0]), np.zeros(0, np.int64)
    heavy_sizes, removes = [], name != "wavelet-tree"

    def add(x):
        nonlocal live
        first = live.size + gone.size  # the vectors ever added: a fresh id never repeats one that was handed out
        a.add(x)
        twin.add(x)
        live = np.concatenate([live, np.arange(first, first + x.shape[0])])

    def remove(sel):
        nonlocal live, gone
        if not removes:
            with pytest.raises(RuntimeError, match="permutation"):
                a.remove_ids(sel)
            return
        arg = np.concatenate([sel, gone[:5], [rows.shape[0] + 9]]).astype(np.int64)  # (some already gone, one never handed out)
        assert a.remove_ids(_torch().from_numpy(arg).cuda()) == sel.size == twin.remove_ids(arg)
        live, gone = np.setdiff1d(live, sel), np.concatenate([gone, sel])

    second = np.arange(batches[0].shape[0] + batches[1].shape[0], batches[0].shape[0] + batches[1].shape[0] + batches[2].shape[0])
    plan = [lambda: add(batches[1]),
            lambda: remove(rng.choice(live, 1500, replace=False)),
            lambda: add(batches[2]),
            lambda: remove(np.concatenate([rng.choice(second, 400, replace=False), rng.choice(live[live < second[0]], 600, replace=False)])),
            lambda: add(batches[3])]
    for no, step in enumerate(plan):
        step()
        check_index(a, twin, rows, live, gone, xq, f"{name} step {no + 1}")
        heavy_sizes.append(a.invlists.list_size(HEAVY))
    sizes = [a.invlists.list_size(l) for l in range(INDEX_NLIST)]
    assert max(heavy_sizes) > 4096 and min(heavy_sizes) < 4096, heavy_sizes
    assert sum(700 < s < 1300 for s in sizes) >= 5, sizes
