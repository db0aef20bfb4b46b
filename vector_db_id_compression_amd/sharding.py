"""Inverted lists sharded over the GPUs of one node.

Every list is an independent codec unit: encode and decode need no exchange, so each rank owns a subset of
the lists (balanced by total length, not by count: list sizes are Zipf-like) and compresses / decompresses it
with its own GPU.  The only communication is the variable-size gather of decoded ids to the rank that runs a
search (custom_invlists_impl.cpp:477-525 decodes the lists a search touched): one point-to-point message per owning
rank over its direct xGMI link (RCCL send/recv posted as one batch; `gloo` in the CPU tests).  The
list -> (rank, local number) map is replicated (nlist * 12 bytes), so message sizes are known without a size exchange.

Nothing here loops over lists in Python except the LPT assignment (a heap pop per list): shards are cut with index
arithmetic and the gathered lists land in request order with one indexed copy per owning rank.

`ShardedInvLists` is the multi-process form (one process per GPU, torch.distributed).  `DeviceShards` is the single-process form
over the C-ABI's vidc_shards: one process drives every context, the cut / placement / label routing are HIP kernels, and no index
arithmetic happens in Python.  `DeviceShards.append` adds a batch of (list number, id) pairs without re-encoding the index: the map
stays, `DeviceShards.loads` shows how the balance drifts; `DeviceShards.remove` takes a batch out the same way, and
`DeviceShards.rebalance` moves the lists to the map a fresh encode would choose (ROC lists as streams, without encoding).  It has been exercised with several contexts on one device; never run on
more than one GPU.
"""
import heapq

import numpy as np


def lpt_partition(sizes, world):
    """Longest-processing-time greedy: lists sorted by length, each to the currently lightest rank.
    -> owner int32[nlist]"""
    sizes = np.asarray(sizes, dtype=np.int64)
    owner = np.zeros(sizes.size, dtype=np.int32)
    if world <= 1 or sizes.size == 0:
        return owner
    heap = [(0, r) for r in range(world)]
    order = np.argsort(-sizes, kind="stable")
    sz = sizes[order].tolist()
    own = [0] * len(sz)
    for i, s in enumerate(sz):
        load, r = heap[0]
        own[i] = r
        heapq.heapreplace(heap, (load + s, r))
    owner[order] = np.asarray(own, dtype=np.int32)
    return owner


def _segment_index(starts, sizes, xp):
    """Concatenated index ranges [starts[k], starts[k] + sizes[k]) (numpy or torch)."""
    total = int(sizes.sum())
    if xp is np:
        cum = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if sizes.size else np.zeros(0, np.int64)
        return np.repeat(starts - cum, sizes) + np.arange(total, dtype=np.int64)
    import torch

    cum = torch.cumsum(sizes, 0) - sizes
    return torch.repeat_interleave(starts - cum, sizes) + torch.arange(total, dtype=torch.int64, device=sizes.device)


class ShardedInvLists:
    """One shard of a CSR set of lists per rank + gather of decoded ids.

    encode_fn(local_offsets uint64 numpy, local_ids) -> codec object with
    decode_lists(local_list_nos) -> (ids tensor, out_offsets)   [RocLists / EfLists / PackedLists have exactly this]
    `ids` may be a host array (uint64 / int64) or a CUDA int64 tensor (the shard is then cut on the device).
    """

    def __init__(self, offsets, ids, rank, world, encode_fn, group=None, device="cuda"):
        offsets = np.asarray(offsets, dtype=np.uint64)
        self.rank, self.world, self.group, self.device = rank, world, group, device
        self.sizes = (offsets[1:] - offsets[:-1]).astype(np.int64)
        self.nlist = self.sizes.size
        self.owner = lpt_partition(self.sizes, world)
        # local numbering: lists of a rank in increasing global number (rank of the list among its owner's lists)
        order = np.argsort(self.owner, kind="stable")
        counts = np.bincount(self.owner, minlength=world).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        self.local_no = np.empty(self.nlist, dtype=np.int64)
        self.local_no[order] = np.arange(self.nlist, dtype=np.int64) - np.repeat(first, counts)
        self.my_lists = order[first[rank]:first[rank] + counts[rank]]
        loc_sizes = self.sizes[self.my_lists]
        self.local_offsets = np.concatenate([[0], np.cumsum(loc_sizes)]).astype(np.uint64)
        starts = offsets[:-1].astype(np.int64)[self.my_lists]
        if isinstance(ids, np.ndarray):
            if ids.dtype.kind not in "iu":
                raise TypeError(f"ids must be an integer array, got {ids.dtype}")
            # 8-byte ids are reinterpreted, narrower ones (int32 / uint32 id arrays) converted: a view of those would
            # halve the length and encode garbage
            cut = np.ascontiguousarray(ids[_segment_index(starts, loc_sizes, np)]) if loc_sizes.size else np.zeros(0, dtype=np.uint64)
            local_ids = cut.view(np.uint64) if cut.dtype.itemsize == 8 else cut.astype(np.uint64)
        else:  # CUDA tensor
            import torch

            st = torch.from_numpy(starts).to(ids.device)
            sz = torch.from_numpy(loc_sizes).to(ids.device)
            local_ids = ids[_segment_index(st, sz, torch)] if loc_sizes.size else ids[:0]
        self.codec = encode_fn(self.local_offsets, local_ids)
        self.load = np.bincount(self.owner, weights=self.sizes, minlength=world).astype(np.int64)
        self._p2p_ready = False

    def _ensure_p2p(self):
        """The first operation of a process group must not be a batch of point-to-point operations: PyTorch documents batched
        send / recv as undefined when they are a group's first call (the NCCL / RCCL communicators of the pairs are created
        lazily and at different moments on the two sides).  One collective brings every rank's communicator up first."""
        if self._p2p_ready or self.world <= 1:
            return
        import torch
        import torch.distributed as dist

        t = torch.zeros(1, dtype=torch.int64, device=self.device)
        dist.all_reduce(t, group=self.group)
        self._p2p_ready = True

    def decode_local(self, list_nos):
        """Decode the requested GLOBAL list numbers this rank owns (request order, repeats kept)
        -> (their global numbers, ids tensor, offsets of the lists inside it)."""
        ln = np.asarray(list_nos, dtype=np.int64)
        ln = ln[self.owner[ln] == self.rank]
        ids, off = self.codec.decode_lists(self.local_no[ln].astype(np.uint64))
        return ln, ids, off

    def gather_ids(self, list_nos, dst=0):
        """Decoded ids of `list_nos` (global numbers, any owners) assembled on rank `dst`.
        -> (int64 tensor in request order, offsets) on dst, (None, None) elsewhere."""
        import torch
        import torch.distributed as dist

        ln = np.asarray(list_nos, dtype=np.int64)
        sizes = self.sizes[ln]
        req_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        owners = self.owner[ln]
        _, ids, _ = self.decode_local(ln)
        ids = ids.to(self.device).view(torch.int64) if ids.numel() else torch.zeros(0, dtype=torch.int64, device=self.device)
        self._ensure_p2p()
        if self.world > 1 and self.rank != dst:
            if ids.numel():  # (the same batched form as the receiving side: one group call per rank and gather)
                for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, ids.contiguous(), dst, self.group)]):
                    w.wait()
            return None, None
        out = torch.empty(int(req_off[-1]), dtype=torch.int64, device=self.device)
        bufs = {self.rank: ids}
        if self.world > 1:  # one message per owning rank, sizes known from the replicated map; all receives posted at once
            ops = []
            for r in range(self.world):
                n = int(sizes[owners == r].sum())
                if r == dst or n == 0:
                    continue
                bufs[r] = torch.empty(n, dtype=torch.int64, device=self.device)
                ops.append(dist.P2POp(dist.irecv, bufs[r], r, self.group))
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
        for r, buf in bufs.items():  # the lists of rank r, in request order, to their slots: one indexed copy
            items = np.nonzero(owners == r)[0]
            if items.size == 0:
                continue
            st = torch.from_numpy(req_off[items]).to(self.device)
            sz = torch.from_numpy(sizes[items]).to(self.device)
            out[_segment_index(st, sz, torch)] = buf
        return out, req_off


_KINDS = {"packed": 0, "ef": 1, "roc": 2, "wt": 3}


class DeviceShards:
    """vidc_shards: one CSR set of lists cut over several contexts of ONE process (include/vidc.h), with the method names and return
    shapes of the single-object containers (PackedLists / EfLists / RocLists), so IVFIndex.search_defer_id_decoding takes it as it is.

    Exercised with several contexts on one device; never run on more than one GPU."""

    def __init__(self, handle, home, ctxs, kind):
        self.h, self.ctx, self.ctxs, self.kind = handle, home, list(ctxs), kind
        self._offsets = self._owner = self._local_no = None

    def __del__(self):
        try:  # may run during interpreter shutdown, after module globals are gone
            if getattr(self, "h", None):
                from ._lib import lib

                lib().vidc_shards_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @classmethod
    def encode(cls, kind, offsets, ids, devices=None, ctxs=None, nshards=None, home=None, **codec_args):
        """kind: "packed" / "ef" / "roc".  Contexts: `ctxs` (a list of _lib.Context, kept alive by the object), or one new context per
        entry of `devices` (device numbers, repeats allowed), or `nshards` new contexts on the current device.  home: the context whose
        device holds `ids` and every request's arrays (default: the current device's default context).  codec_args: bits (packed),
        want_perm (ef, roc), precision_mode (roc).  offsets: host array, or an int64 / uint64 CUDA tensor on the home device."""
        import ctypes as C

        from . import _lib, codecs

        k = _KINDS[kind] if isinstance(kind, str) else int(kind)
        home = _lib.default_context() if home is None else home
        if ctxs is None:
            if devices is None:
                import torch

                devices = [torch.cuda.current_device()] * int(1 if nshards is None else nshards)
            ctxs = [_lib.Context(int(d)) for d in devices]
        ctxs = list(ctxs)
        param, flags = 0, 0
        if k == 0:
            param = int(codec_args.pop("bits", None) or 0)
        elif k == 1:
            flags = _lib.VIDC_EF_WANT_PERM if codec_args.pop("want_perm", False) else 0
        elif k == 2:
            param = int(codec_args.pop("precision_mode", _lib.VIDC_PREC_REFERENCE))
            flags = _lib.VIDC_ROC_WANT_PERM if codec_args.pop("want_perm", False) else 0
        if codec_args:
            raise TypeError(f"unknown codec arguments for {kind}: {sorted(codec_args)}")
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        h = C.c_void_p()
        d_off = codecs._cuda_offsets(offsets, home)
        if d_off is not None:
            d_ids = codecs._dev_ids_dev(ids, d_off)
            _lib.check(_lib.lib().vidc_shards_encode_dev(home.h, len(ctxs), arr, k, param, flags, d_off.numel() - 1, _lib.ptr(d_off),
                                                         d_ids.numel(), _lib.ptr(d_ids) if d_ids.numel() else None, C.byref(h)))
            obj = cls(h, home, ctxs, k)
        else:
            off = codecs._as_offsets(offsets)
            d_ids = codecs._dev_ids(ids, int(off[-1])) if off[-1] else None
            _lib.check(_lib.lib().vidc_shards_encode(home.h, len(ctxs), arr, k, param, flags, off.size - 1, _lib.ptr(off), _lib.ptr(d_ids),
                                                     C.byref(h)))
            obj = cls(h, home, ctxs, k)
            obj._offsets = off
        return obj

    # -- host-side accessors
    @property
    def nshards(self):
        from ._lib import lib

        return int(lib().vidc_shards_count(self.h))

    @property
    def nlist(self):
        from ._lib import lib

        return int(lib().vidc_shards_nlist(self.h))

    @property
    def ntotal(self):
        from ._lib import lib

        return int(lib().vidc_shards_ntotal(self.h))

    @property
    def compressed_bytes(self):
        from ._lib import lib

        return int(lib().vidc_shards_compressed_bytes(self.h))

    @property
    def offsets(self):
        if self._offsets is None:
            from ._lib import check, lib, ptr

            off = np.zeros(self.nlist + 1, np.uint64)
            check(lib().vidc_shards_offsets(self.h, ptr(off)))
            self._offsets = off
        return self._offsets

    def _map(self):
        if self._owner is None:
            from ._lib import check, lib, ptr

            owner, local = np.zeros(max(self.nlist, 1), np.int32), np.zeros(max(self.nlist, 1), np.uint32)
            check(lib().vidc_shards_map(self.h, ptr(owner), ptr(local)))
            self._owner, self._local_no = owner[: self.nlist], local[: self.nlist]
        return self._owner, self._local_no

    @property
    def owner(self):
        """int32[nlist]: the shard of every list (== lpt_partition(sizes, nshards))"""
        return self._map()[0]

    @property
    def local_no(self):
        """uint32[nlist]: a list's number inside its shard"""
        return self._map()[1]

    def shard(self, i):
        """Shard i as a borrowed PackedLists / EfLists / RocLists view (None for a shard without lists): the view never destroys the
        handle and keeps this object alive."""
        from . import _lib, codecs

        h = _lib.lib().vidc_shards_shard(self.h, int(i))
        if not h:
            return None
        base = (codecs.PackedLists, codecs.EfLists, codecs.RocLists)[self.kind]
        view_cls = type("Borrowed" + base.__name__, (base,), {"__del__": lambda self: None})
        mine = self.owner == int(i)
        sizes = (self.offsets[1:] - self.offsets[:-1])[mine]
        view = view_cls(_lib._vp(h), self.ctxs[int(i)], np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64))
        view._shards = self
        return view

    # -- requests (home context; arrays on the home device)
    def decode_all(self, out=None):
        import torch

        from . import codecs
        from ._lib import check, lib, ptr

        if out is None:
            out = torch.empty(max(self.ntotal, 1), dtype=torch.int64, device="cuda")
        codecs._on_torch_stream(self.ctx)
        check(lib().vidc_shards_decode_all(self.ctx.h, self.h, ptr(out)))
        return out[: self.ntotal]

    def decode_lists(self, list_nos):
        """-> (int64 CUDA tensor: the requested lists back to back, request order and repeats kept; offsets uint64[m + 1])"""
        import torch

        from . import codecs
        from ._lib import check, lib, ptr

        ln = np.ascontiguousarray(list_nos, dtype=np.uint64)
        ok = ln[ln < self.nlist].astype(np.int64)
        total = int((self.offsets[1:] - self.offsets[:-1])[ok].sum()) if ok.size else 0
        out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
        out_off = np.zeros(ln.size + 1, np.uint64)
        codecs._on_torch_stream(self.ctx)
        check(lib().vidc_shards_decode_lists(self.ctx.h, self.h, ln.size, ptr(ln), ptr(out), ptr(out_off)))
        return out[:total], out_off

    def decode_gather(self, list_nos, item_slot, item_off):
        from . import codecs
        from ._lib import lib

        return codecs._decode_gather(lib().vidc_shards_decode_gather, self, list_nos, item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids, on the device; `out` may be `labels`.  Waits for its join."""
        from . import codecs
        from ._lib import lib

        return codecs._translate_labels(lib().vidc_shards_translate_labels_dev, self, labels, out, invalid)

    @property
    def loads(self):
        """uint64[nshards]: ids per shard (the sum of its lists' sizes).  Appends keep the map, so the balance drifts: compare with
        ntotal / nshards to decide when `rebalance` is worth it."""
        from ._lib import check, lib, ptr

        loads = np.zeros(self.nshards, np.uint64)
        check(lib().vidc_sharded_loads(self.h, ptr(loads)))
        return loads

    def append(self, list_nos, ids, labels=True, invalid=None, **codec_args):
        """A batch of (GLOBAL list number, id) pairs behind the lists of this object -> (NEW DeviceShards over the same contexts and the
        same map, labels); this object stays valid and unchanged (vidc_sharded_append_dev).  Every shard runs its own append on the pairs
        routed to it.  codec_args as in the single-object appends: bits (packed; None / 0 keeps the width), want_perm (ef, roc),
        precision_mode (roc: the mode this object was built with).  See codecs._append for list_nos / ids / labels / invalid: the arrays
        live on the home device, the labels carry global list numbers.  The call waits."""
        from . import _lib, codecs

        param, flags = 0, 0
        if self.kind == 0:
            param = int(codec_args.pop("bits", None) or 0)
        elif self.kind == 1:
            flags = _lib.VIDC_EF_WANT_PERM if codec_args.pop("want_perm", False) else 0
        elif self.kind == 2:
            param = int(codec_args.pop("precision_mode", _lib.VIDC_PREC_REFERENCE))
            flags = _lib.VIDC_ROC_WANT_PERM if codec_args.pop("want_perm", False) else 0
        if codec_args:
            raise TypeError(f"unknown codec arguments: {sorted(codec_args)}")
        h, lab = codecs._append(_lib.lib().vidc_sharded_append_dev, self, list_nos, ids, (param, flags), labels, invalid)
        return type(self)(h, self.ctx, self.ctxs, self.kind), lab  # (the offsets are fetched from the new object on first use)

    def remove(self, list_nos, ids, removed=True, missing=None, invalid=None, **codec_args):
        """A batch of (GLOBAL list number, id) pairs, or of ids alone (list_nos None: any-list mode), leaves the lists of this object ->
        (NEW DeviceShards over the same contexts and the same map, removed mask or None); this object stays valid and unchanged
        (vidc_remove_sharded_dev).  Every shard runs its own remove; the mask is in this object's decode_all order, `missing` counts the
        valid pairs no shard matched.  codec_args as in append, minus bits: want_perm (ef, roc), precision_mode (roc: the mode this
        object was built with).  See removal.remove for list_nos / ids / removed / missing / invalid: the arrays live on the home
        device.  The call waits."""
        from . import _lib, removal

        param, flags = 0, 0
        if self.kind == 1:
            flags = _lib.VIDC_EF_WANT_PERM if codec_args.pop("want_perm", False) else 0
        elif self.kind == 2:
            param = int(codec_args.pop("precision_mode", _lib.VIDC_PREC_REFERENCE))
            flags = _lib.VIDC_ROC_WANT_PERM if codec_args.pop("want_perm", False) else 0
        if codec_args:
            raise TypeError(f"unknown codec arguments: {sorted(codec_args)}")
        h, mask = removal._call(_lib.lib().vidc_remove_sharded_dev, self, (param, flags), list_nos, ids, removed, missing, invalid)
        return type(self)(h, self.ctx, self.ctxs, self.kind), mask  # (the offsets are fetched from the new object on first use)

    def rebalance(self, want_perm=False):
        """The lists of this object under the map `encode` would choose for what it decodes to -> (NEW DeviceShards over the same
        contexts, moved_ids); this object stays valid and unchanged (vidc_rebalance_sharded).  Every request answers on the new object
        as on this one; `owner`, `local_no` and `loads` are the new map's; moved_ids counts the ids whose owner changed.  Packed bits
        and Elias-Fano are rebuilt from decode_all on the device; ROC lists move as streams, no list is encoded again.  want_perm
        (ef, roc): the new object's permutation, the identity inside every list.  The call waits."""
        import ctypes as C

        from . import _lib, codecs

        flags = 0
        if want_perm:
            if self.kind == 0:
                raise TypeError("packed lists keep no permutation")
            flags = _lib.VIDC_EF_WANT_PERM if self.kind == 1 else _lib.VIDC_ROC_WANT_PERM
        h, moved = C.c_void_p(), C.c_uint64(0)
        codecs._on_torch_stream(self.ctx)
        _lib.check(_lib.lib().vidc_rebalance_sharded(self.ctx.h, self.h, flags, C.byref(h), C.byref(moved)))
        new = type(self)(h, self.ctx, self.ctxs, self.kind)
        new._offsets = self._offsets
        return new, int(moved.value)

    def perm(self):
        from ._lib import check, lib, ptr

        p = np.zeros(max(self.ntotal, 1), np.uint32)
        check(lib().vidc_shards_perm(self.ctx.h, self.h, ptr(p)))
        return p[: self.ntotal]
