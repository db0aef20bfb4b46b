"""Device-resident codec objects over the C-ABI (one object = every list of one index / graph).

IDs live in HBM as torch int64 tensors (faiss::idx_t); list boundaries are a CSR `offsets[nlist+1]`, on the host
(numpy / list) or on the GPU (an int64 / uint64 CUDA tensor, routed to the vidc_*_encode_dev entry points).  All heavy work
happens in the HIP kernels behind libvidc.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VIDC_PREC_EXACT, VIDC_PREC_REFERENCE, check, lib, ptr


def _torch():
    import torch

    return torch


def _as_offsets(offsets):
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    assert off.ndim == 1 and off.size >= 1
    return off


def _cuda_offsets(offsets, ctx):
    """The offsets as a contiguous int64 / uint64 CUDA tensor on the context's device, or None for host offsets (numpy, lists).
    (Real exceptions, not asserts: the C call reads 8 * numel bytes of device memory.)"""
    if type(offsets).__module__.split(".")[0] != "torch":
        return None
    torch = _torch()
    if not offsets.is_cuda:
        return None
    if offsets.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"device offsets must be int64 or uint64, not {offsets.dtype}")
    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("device offsets must be a 1-D tensor of nlist + 1 entries")
    want = getattr(ctx, "device", -1)
    want = torch.cuda.current_device() if want is None or want < 0 else want
    if offsets.device.index != want:
        raise ValueError(f"device offsets live on cuda:{offsets.device.index}, the context on cuda:{want}")
    return offsets.contiguous()


def _dev_ids_dev(ids, d_off):
    """ids of a device-offsets call: a 64-bit CUDA tensor on the offsets' device (checked with exceptions: the kernels read 8 bytes
    per id)."""
    torch = _torch()
    if isinstance(ids, np.ndarray):
        ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint64).view(np.int64)).cuda()
    if not ids.is_cuda or ids.dtype not in (torch.int64, torch.uint64):
        raise TypeError("ids must be an int64 / uint64 CUDA tensor")
    ids = _dev_ids(ids, _count(ids))
    if ids.device != d_off.device:
        raise ValueError("ids and offsets must live on the same device")
    return ids


def _count(ids):
    """number of ids in a tensor or an array"""
    return int(ids.numel()) if hasattr(ids, "numel") else int(np.asarray(ids).size)


def _dev_ids(ids, ntotal):
    """int64/uint64 CUDA tensor (or numpy array, uploaded) of ntotal ids."""
    torch = _torch()
    if isinstance(ids, np.ndarray):
        ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    assert ids.is_cuda, "ids must live on the GPU"
    assert ids.dtype in (torch.int64, torch.uint64)
    ids = ids.contiguous()
    assert ids.numel() == ntotal
    return ids



def _is_cuda(x):
    """a CUDA tensor (a device-resident request)"""
    return type(x).__module__.split(".")[0] == "torch" and x.is_cuda


def _on_torch_stream(ctx):
    """The producer of a device-resident request is torch's current stream: the default context follows it, as
    _lib.default_context does when it hands the context out."""
    torch = _torch()
    if _lib._default_ctx.get(torch.cuda.current_device()) is ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def _dev_array(x, ctx, what):
    """x as a contiguous CUDA tensor on the context's device (real exceptions: the C call reads 8 bytes per entry)."""
    want = getattr(ctx, "device", -1)
    want = _torch().cuda.current_device() if want is None or want < 0 else want
    if x.device.index != want:
        raise ValueError(f"{what} live on cuda:{x.device.index}, the context on cuda:{want}")
    return x.contiguous()


def _translate_labels(fn, obj, labels, out, invalid):
    """vidc_*_translate_labels_dev: Faiss labels (list_no << 32 | offset, -1 = no result) -> ids, on the device.  labels: int64 CUDA
    tensor of any shape; out (optional, may be labels itself): int64 CUDA tensor of the same size; invalid (optional): 1-element int64
    CUDA tensor the number of invalid labels is added to.  Nothing is synchronised (ROC plans on the host: it waits)."""
    torch = _torch()
    if not _is_cuda(labels) or labels.dtype != torch.int64:
        raise TypeError("labels must be an int64 CUDA tensor")
    if out is not None and out is labels and not labels.is_contiguous():
        raise ValueError("in-place translation needs contiguous labels")
    lab = _dev_array(labels, obj.ctx, "labels")
    if out is None:
        out = torch.empty_like(lab)
    elif not _is_cuda(out) or out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != lab.numel():
        raise ValueError("out must be a contiguous int64 CUDA tensor with one entry per label")
    elif out.device != lab.device:
        raise ValueError("out and labels must live on the same device")
    if invalid is not None and (not _is_cuda(invalid) or invalid.dtype != torch.int64 or invalid.numel() != 1
                                or not invalid.is_contiguous() or invalid.device != lab.device):
        raise ValueError("invalid must be a 1-element int64 CUDA tensor on the labels' device")
    _on_torch_stream(obj.ctx)
    check(fn(obj.ctx.h, obj.h, lab.numel(), ptr(lab) if lab.numel() else None, ptr(out) if lab.numel() else None, ptr(invalid)))
    return out


def _append(fn, obj, list_nos, ids, extra, labels, invalid):
    """vidc_*_append_dev: a batch of (list number, id) pairs placed behind the lists of `obj`, in batch order inside every list -> (handle
    of the NEW object, labels).  list_nos: int64 CUDA tensor (negative = not assigned, skipped), ids: int64 / uint64 CUDA tensor of the
    same size; numpy arrays are uploaded.  labels: True (a new int64 CUDA tensor), False / None (none) or an int64 CUDA tensor to fill:
    list_no << 32 | offset of every batch entry in the new object, -1 for a skipped one.  invalid (optional): 1-element int64 CUDA tensor
    the number of list numbers >= nlist is added to.  Runs on torch's current stream; the call synchronises."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.VidcError("no HIP device: append needs an MI355X (there is no CPU fallback)")
    if isinstance(list_nos, np.ndarray):
        list_nos = torch.from_numpy(np.ascontiguousarray(list_nos, dtype=np.int64)).cuda()
    if isinstance(ids, np.ndarray):
        ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    if not _is_cuda(list_nos) or list_nos.dtype != torch.int64:
        raise TypeError("list_nos must be an int64 CUDA tensor")
    if not _is_cuda(ids) or ids.dtype not in (torch.int64, torch.uint64):
        raise TypeError("ids must be an int64 / uint64 CUDA tensor")
    if list_nos.numel() != ids.numel():
        raise ValueError("list_nos and ids must have one entry per pair")
    ln = _dev_array(list_nos.reshape(-1), obj.ctx, "list_nos")
    di = _dev_array(ids.reshape(-1), obj.ctx, "ids")
    n = ln.numel()
    lab = None
    if labels is True:
        lab = torch.empty(max(n, 1), dtype=torch.int64, device=ln.device)
    elif labels is not None and labels is not False:
        if not _is_cuda(labels) or labels.dtype != torch.int64 or not labels.is_contiguous() or labels.numel() != n or labels.device != ln.device:
            raise ValueError("labels must be a contiguous int64 CUDA tensor with one entry per pair, on the batch's device")
        lab = labels
    if invalid is not None and (not _is_cuda(invalid) or invalid.dtype != torch.int64 or invalid.numel() != 1
                                or not invalid.is_contiguous() or invalid.device != ln.device):
        raise ValueError("invalid must be a 1-element int64 CUDA tensor on the batch's device")
    _on_torch_stream(obj.ctx)
    h = C.c_void_p()
    check(fn(obj.ctx.h, obj.h, n, ptr(ln) if n else None, ptr(di) if n else None, *extra, C.byref(h),
             ptr(lab) if lab is not None and n else None, ptr(invalid)))
    return h, (None if lab is None else lab[:n])


def _update_rows(fn, obj, K, n_old, nodes, rows, n_new, extra, invalid):
    """vidc_*_update_rows_dev: rows of a graph object replaced, and nodes added -> (handle of the NEW object, its node count).  nodes:
    integer CUDA tensor [m] (negative = skipped; the LAST mention of a node wins), rows: int32 CUDA tensor [m, K], -1 terminated; numpy
    arrays are uploaded.  n_new: node count of the new object (None: the old one); new nodes without a batch row are empty.  invalid
    (optional): 1-element int64 CUDA tensor the number of nodes >= n_new is added to.  Runs on torch's current stream; the call
    synchronises."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.VidcError("no HIP device: update_rows needs an MI355X (there is no CPU fallback)")
    if isinstance(nodes, (np.ndarray, list, tuple)):
        nodes = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)).cuda()
    if isinstance(rows, np.ndarray):
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
    if not _is_cuda(nodes) or nodes.dtype.is_floating_point or nodes.dtype == torch.bool:
        raise TypeError("nodes must be an integer CUDA tensor")
    if not _is_cuda(rows) or rows.dtype != torch.int32:
        raise TypeError("rows must be an int32 CUDA tensor")
    nd = _dev_array(nodes.reshape(-1).long(), obj.ctx, "nodes")
    m = nd.numel()
    if rows.numel() != m * K or (m and rows.dim() == 2 and rows.shape[1] != K):
        raise ValueError(f"rows must hold one row of K = {K} entries per node")
    rw = _dev_array(rows.reshape(-1), obj.ctx, "rows")
    if invalid is not None and (not _is_cuda(invalid) or invalid.dtype != torch.int64 or invalid.numel() != 1
                                or not invalid.is_contiguous() or invalid.device != nd.device):
        raise ValueError("invalid must be a 1-element int64 CUDA tensor on the batch's device")
    n_new = int(n_old if n_new is None else n_new)
    _on_torch_stream(obj.ctx)
    h = C.c_void_p()
    check(fn(obj.ctx.h, obj.h, m, ptr(nd) if m else None, ptr(rw) if m else None, n_new, *extra, C.byref(h), ptr(invalid)))
    return h, n_new


def _decode_rows_dev(fn, obj, nodes, K, want_counts, pass_K=True):
    """vidc_*_decode_rows_dev / vidc_compact_rows_decode_dev: rows of a CUDA tensor of nodes (-1 rows for negative nodes and nodes
    >= N) -> (int32 [m, K] CUDA tensor, int32 CUDA counts or None)."""
    torch = _torch()
    if nodes.dtype.is_floating_point or nodes.dtype == torch.bool:
        raise TypeError("nodes must be an integer CUDA tensor")
    nd = _dev_array(nodes.reshape(-1).long(), obj.ctx, "nodes")
    m = nd.numel()
    out = torch.empty((max(m, 1), K), dtype=torch.int32, device=nd.device)
    counts = torch.empty(max(m, 1), dtype=torch.int32, device=nd.device) if want_counts else None
    _on_torch_stream(obj.ctx)
    args = (obj.ctx.h, obj.h, m, ptr(nd) if m else None) + ((K,) if pass_K else ()) + (ptr(out), ptr(counts), None)
    check(fn(*args))
    return out[:m], (counts[:m] if want_counts else None)


def _decode_gather(fn, obj, list_nos, item_slot, item_off):
    """vidc_*_decode_gather: decode the touched lists on the device, pick the requested ids there, copy 8 bytes per item
    (the decode section of the deferred search, custom_invlists_impl.cpp:508-525) -> numpy int64[n_items]."""
    ln = np.ascontiguousarray(list_nos, dtype=np.uint64)
    sl = np.ascontiguousarray(item_slot, dtype=np.uint64)
    of = np.ascontiguousarray(item_off, dtype=np.uint64)
    assert sl.size == of.size
    out = np.zeros(max(sl.size, 1), np.int64)
    check(fn(obj.ctx.h, obj.h, ln.size, ptr(ln), sl.size, ptr(sl), ptr(of), ptr(out)))
    return out[: sl.size]


class _ListCodec:
    """What the four list codecs share: the handle and its release, the lazily fetched host offsets, ntotal, and the calls that differ
    only in the C symbol (`_prefix` + "_decode_all", ...).  Each class picks how its offsets are fetched in its own `offsets`."""

    _prefix = None  # "vidc_packed", ...

    def __init__(self, handle, ctx, offsets, nlist=None, ntotal=None):
        self.h = handle
        self.ctx = ctx
        self._offsets = offsets
        self._nlist = nlist
        self._ntotal = ntotal

    def _fn(self, name):
        return getattr(lib(), f"{self._prefix}_{name}")

    def __del__(self):
        try:  # may run during interpreter shutdown, after module globals are gone
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    def _offsets_from_symbol(self):
        """the object's own offsets array (vidc_*_offsets), fetched once"""
        if self._offsets is None:
            off = np.zeros(self._nlist + 1, np.uint64)
            check(self._fn("offsets")(self.ctx.h, self.h, ptr(off)))
            self._offsets = off
        return self._offsets

    def _offsets_from_info(self):
        """the prefix sum of info()["sizes"], computed once"""
        if self._offsets is None:
            sizes = self.info()["sizes"]
            self._offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.uint64)]).astype(np.uint64)
        return self._offsets

    @property
    def ntotal(self):
        return self._ntotal if self._ntotal is not None else int(self.offsets[-1])

    def decode_all(self, out=None):
        torch = _torch()
        if out is None:
            out = torch.empty(max(self.ntotal, 1), dtype=torch.int64, device="cuda")
        check(self._fn("decode_all")(self.ctx.h, self.h, ptr(out)))
        return out[: self.ntotal]

    def decode_lists(self, list_nos):
        """Decode the requested lists back to back (work proportional to their sizes) -> (int64 CUDA tensor, offsets)."""
        torch = _torch()
        ln = np.ascontiguousarray(list_nos, dtype=np.uint64)
        sizes = (self.offsets[1:] - self.offsets[:-1])[ln.astype(np.int64)] if ln.size else np.zeros(0, np.uint64)
        total = int(sizes.sum())
        out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
        out_off = np.zeros(ln.size + 1, np.uint64)
        check(self._fn("decode_lists")(self.ctx.h, self.h, ln.size, ptr(ln), ptr(out), ptr(out_off)))
        return out[:total], out_off

    def _get(self, name, list_nos, offs):
        """ids[i] = list_nos[i][offs[i]] (vidc_*_get / vidc_wt_select) -> numpy int64"""
        ln = np.ascontiguousarray(list_nos, dtype=np.uint64)
        of = np.ascontiguousarray(offs, dtype=np.uint64)
        out = np.zeros(max(ln.size, 1), np.int64)
        check(self._fn(name)(self.ctx.h, self.h, ln.size, ptr(ln), ptr(of), ptr(out)))
        return out[: ln.size]


class RocLists(_ListCodec):
    """ROC-compressed lists (vidc_roc): bit-identical streams to codec.cpp."""

    _prefix = "vidc_roc"

    @property
    def offsets(self):
        """CSR offsets of the decoded output.  Graph objects fetch the edge counts from the device on first use
        (the per-node metadata stays on the GPU otherwise)."""
        return self._offsets_from_info()

    # -- construction
    @classmethod
    def encode(cls, offsets, ids, precision_mode=VIDC_PREC_REFERENCE, want_perm=False, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        d_off = _cuda_offsets(offsets, ctx)
        if d_off is not None:  # device offsets: ntotal = ids.numel(), checked against offsets[-1] on the device
            d_ids = _dev_ids_dev(ids, d_off)
            h = C.c_void_p()
            check(lib().vidc_roc_encode_dev(ctx.h, d_off.numel() - 1, ptr(d_off), d_ids.numel(), ptr(d_ids) if d_ids.numel() else None,
                                            int(precision_mode), _lib.VIDC_ROC_WANT_PERM if want_perm else 0, C.byref(h)))
            return cls(h, ctx, None)
        off = _as_offsets(offsets)
        nlist = off.size - 1
        d_ids = _dev_ids(ids, int(off[-1] - off[0])) if off[-1] > off[0] else None
        assert off[0] == 0
        h = C.c_void_p()
        check(lib().vidc_roc_encode(ctx.h, nlist, ptr(off), ptr(d_ids), int(precision_mode),
                                    _lib.VIDC_ROC_WANT_PERM if want_perm else 0, C.byref(h)))
        return cls(h, ctx, off)

    @classmethod
    def encode_rows(cls, rows, precision_mode=VIDC_PREC_REFERENCE, ctx=None):
        """rows: int32 CUDA tensor [N, K], -1 terminated (nsg::Graph<int32_t> layout)."""
        torch = _torch()
        ctx = _lib.default_context() if ctx is None else ctx
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2
        rows = rows.contiguous()
        N, K = rows.shape
        h = C.c_void_p()
        check(lib().vidc_roc_encode_rows(ctx.h, N, K, ptr(rows) if N else None, int(precision_mode), 0, C.byref(h)))
        obj = cls(h, ctx, None)
        obj.K = K
        return obj

    @classmethod
    def from_streams(cls, offsets, precisions, heads, nwords, words_concat, mt_draws=None, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        off = _as_offsets(offsets)
        nlist = off.size - 1
        prec = np.ascontiguousarray(precisions, dtype=np.uint32)
        hd = np.ascontiguousarray(heads, dtype=np.uint64)
        nw = np.ascontiguousarray(nwords, dtype=np.uint32)
        wc = np.ascontiguousarray(words_concat, dtype=np.uint32)
        dr = None if mt_draws is None else np.ascontiguousarray(mt_draws, dtype=np.uint32)
        h = C.c_void_p()
        check(lib().vidc_roc_import(ctx.h, nlist, ptr(off), ptr(prec), ptr(hd), ptr(nw), ptr(dr),
                                    ptr(wc) if wc.size else None, C.byref(h)))
        return cls(h, ctx, off)

    def append(self, list_nos, ids, precision_mode=VIDC_PREC_REFERENCE, want_perm=False, labels=True, invalid=None):
        """A batch of (list number, id) pairs behind the lists of this object -> (NEW RocLists, labels); this object stays valid and
        unchanged (vidc_roc_append_dev).  Only the lists the batch touches are decoded and re-encoded; the streams of the others are
        copied on the device.  precision_mode: the mode this object was built with.  See _append for the arguments."""
        h, lab = _append(lib().vidc_roc_append_dev, self, list_nos, ids,
                         (int(precision_mode), _lib.VIDC_ROC_WANT_PERM if want_perm else 0), labels, invalid)
        return type(self)(h, self.ctx, None), lab

    # -- flat on-disk / wire image (the reference keeps compressed lists in memory only)
    def save(self, path):
        """{offsets, precision, heads, nwords, mt_draws, words} as one .npz; `load` rebuilds the device object."""
        info = self.info()
        nw = info["nwords"]
        words = self.all_words()
        np.savez(path, offsets=self.offsets, precision=info["precision"], heads=info["heads"], nwords=nw,
                 mt_draws=info["mt_draws"], words=words, K=np.int64(getattr(self, "K", 0)))

    @classmethod
    def load(cls, path, ctx=None):
        z = np.load(path)
        obj = cls.from_streams(z["offsets"], z["precision"], z["heads"], z["nwords"], z["words"], z["mt_draws"], ctx=ctx)
        if "K" in z.files and int(z["K"]):  # a graph object: the row width its decode_rows defaults to
            obj.K = int(z["K"])
        return obj

    # -- properties
    @property
    def nlist(self):
        return int(lib().vidc_roc_nlist(self.h))

    @property
    def ntotal(self):
        return int(lib().vidc_roc_ntotal(self.h))

    @property
    def compressed_bytes(self):
        return int(lib().vidc_roc_compressed_bytes(self.h))

    @property
    def total_words(self):
        return int(lib().vidc_roc_total_words(self.h))

    def info(self):
        n = self.nlist
        sizes = np.zeros(n, np.uint32)
        prec = np.zeros(n, np.uint32)
        heads = np.zeros(n, np.uint64)
        nwords = np.zeros(n, np.uint32)
        draws = np.zeros(n, np.uint32)
        check(lib().vidc_roc_list_info(self.h, ptr(sizes), ptr(prec), ptr(heads), ptr(nwords), ptr(draws)))
        return dict(sizes=sizes, precision=prec, heads=heads, nwords=nwords, mt_draws=draws)

    def words(self, list_no, nwords=None):
        if nwords is None:
            nwords = int(self.info()["nwords"][list_no])
        w = np.zeros(max(nwords, 1), np.uint32)
        check(lib().vidc_roc_export_words(self.ctx.h, self.h, list_no, ptr(w), nwords))
        return w[:nwords]

    def all_words(self):
        """the compact stream of every list back to back (word offsets = cumsum of info()['nwords'])"""
        tw = self.total_words
        w = np.zeros(max(tw, 1), np.uint32)
        check(lib().vidc_roc_export_all_words(self.ctx.h, self.h, ptr(w), tw))
        return w[:tw]

    def perm(self):
        p = np.zeros(max(self.ntotal, 1), np.uint32)
        check(lib().vidc_roc_perm(self.ctx.h, self.h, ptr(p)))
        return p[: self.ntotal]

    # -- decode (decode_all, decode_lists: _ListCodec)
    def decode_gather(self, list_nos, item_slot, item_off):
        """ids[i] = list_nos[item_slot[i]][item_off[i]]: the touched lists decoded and the results picked on the device,
        8 bytes per result copied to the host (vidc_roc_decode_gather)."""
        return _decode_gather(lib().vidc_roc_decode_gather, self, list_nos, item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids (int64 CUDA tensor), on the device: the decode section of
        a search whose labels come from a GPU top-k (vidc_roc_translate_labels_dev).  Negative labels and labels outside the
        object give -1; the latter are added to `invalid` (optional 1-element int64 CUDA tensor).  `out` may be `labels`."""
        return _translate_labels(lib().vidc_roc_translate_labels_dev, self, labels, out, invalid)

    def decode_rows(self, nodes, K=None, want_counts=True):
        """-> (int32 [m, K] CUDA tensor, -1 padded; edge counts or None).  `want_counts=False` keeps the per-node
        edge counts on the device (no metadata crosses PCIe)."""
        torch = _torch()
        K = K or self.K
        if nodes is not None and _is_cuda(nodes):  # device nodes (vidc_roc_decode_rows_dev): counts stay on the device too
            return _decode_rows_dev(lib().vidc_roc_decode_rows_dev, self, nodes, K, want_counts)
        if nodes is None:  # every node, in order: no index array at all
            nd, m = None, self.nlist
        else:
            nd = np.ascontiguousarray(nodes, dtype=np.uint64)
            m = nd.size
        out = torch.empty((max(m, 1), K), dtype=torch.int32, device="cuda")
        counts = np.zeros(max(m, 1), np.uint32) if want_counts else None
        check(lib().vidc_roc_decode_rows(self.ctx.h, self.h, m, ptr(nd), K, ptr(out), ptr(counts)))
        return out[:m], (counts[:m] if want_counts else None)

    @property
    def last_decode_nonclean(self):
        return int(lib().vidc_roc_last_decode_nonclean(self.h))

    @property
    def last_decode_handed_back(self):
        """Work items of the last decode call that a bucket-row decoder handed back (a full member row) and that the call decoded
        again on the general kernel: same output, a serial chain more (vidc_roc_last_decode_handed_back)."""
        return int(lib().vidc_roc_last_decode_handed_back(self.h))


def roc_regroup(sources, src_no, list_no, want_perm=False, ctx=None):
    """A NEW RocLists made of whole lists of other objects, without encoding (vidc_roc_regroup): list j is list list_no[j] of
    sources[src_no[j]], stream and metadata bit for bit.  sources: up to 8 RocLists on one device, None allowed where no src_no names
    it; lists may repeat.  want_perm: the identity permutation in every list.  ctx: the context the new object is built through
    (default: the first source's).  A function of the module, like removal.remove: the method set of the list classes is pinned
    (tests/test_gpu_call_contract.py)."""
    sources = list(sources)
    if ctx is None:
        ctx = next((s.ctx for s in sources if s is not None), None)
        ctx = _lib.default_context() if ctx is None else ctx
    sn = np.ascontiguousarray(src_no, dtype=np.uint32)
    ln = np.ascontiguousarray(list_no, dtype=np.uint64)
    assert sn.size == ln.size
    arr = (C.c_void_p * max(len(sources), 1))(*[None if s is None else s.h for s in sources])
    h = C.c_void_p()
    check(lib().vidc_roc_regroup(ctx.h, len(sources), arr, sn.size, ptr(sn) if sn.size else None, ptr(ln) if ln.size else None,
                                 _lib.VIDC_ROC_WANT_PERM if want_perm else 0, C.byref(h)))
    return RocLists(h, ctx, None)


class PackedLists(_ListCodec):
    """Fixed-width packed ids (vidc_packed): ceil(log2(ntotal+1)) bits per id, LSB-first."""

    _prefix = "vidc_packed"

    @property
    def offsets(self):
        """CSR offsets (host).  Objects built from device offsets copy the object's own device array on first use."""
        return self._offsets_from_symbol()

    @staticmethod
    def bits_for(ntotal):
        return int(lib().vidc_packed_bits_for(int(ntotal)))

    @classmethod
    def encode(cls, offsets, ids, bits=None, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        d_off = _cuda_offsets(offsets, ctx)
        if d_off is not None:  # device offsets: ntotal = ids.numel(), checked against offsets[-1] on the device
            d_ids = _dev_ids_dev(ids, d_off)
            ntotal, nlist = d_ids.numel(), d_off.numel() - 1
            if bits is None:
                bits = cls.bits_for(ntotal)
            h = C.c_void_p()
            check(lib().vidc_packed_encode_dev(ctx.h, nlist, ptr(d_off), ntotal, ptr(d_ids) if ntotal else None, int(bits),
                                               C.byref(h)))
            return cls(h, ctx, None, nlist, ntotal)
        off = _as_offsets(offsets)
        ntotal = int(off[-1])
        if bits is None:
            bits = cls.bits_for(ntotal)
        d_ids = _dev_ids(ids, ntotal) if ntotal else None
        h = C.c_void_p()
        check(lib().vidc_packed_encode(ctx.h, off.size - 1, ptr(off), ptr(d_ids), int(bits), C.byref(h)))
        return cls(h, ctx, off)

    def append(self, list_nos, ids, bits=None, labels=True, invalid=None):
        """A batch of (list number, id) pairs behind the lists of this object -> (NEW PackedLists, labels); this object stays valid and
        unchanged (vidc_packed_append_dev).  bits=None keeps this object's width; a larger one re-packs every list.  See _append."""
        h, lab = _append(lib().vidc_packed_append_dev, self, list_nos, ids, (0 if bits is None else int(bits),), labels, invalid)
        return type(self)(h, self.ctx, None, self._nlist if self._offsets is None else self._offsets.size - 1, None), lab

    @property
    def bits(self):
        return int(lib().vidc_packed_bits(self.h))

    @property
    def compressed_bytes(self):
        return int(lib().vidc_packed_compressed_bytes(self.h))

    def decode_gather(self, list_nos, item_slot, item_off):
        """ids[i] = list_nos[item_slot[i]][item_off[i]]: the touched lists decoded and the results picked on the device,
        8 bytes per result copied to the host (vidc_packed_decode_gather)."""
        return _decode_gather(lib().vidc_packed_decode_gather, self, list_nos, item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids (int64 CUDA tensor), on the device: the decode section of
        a search whose labels come from a GPU top-k (vidc_packed_translate_labels_dev).  Negative labels and labels outside the
        object give -1; the latter are added to `invalid` (optional 1-element int64 CUDA tensor).  `out` may be `labels`."""
        return _translate_labels(lib().vidc_packed_translate_labels_dev, self, labels, out, invalid)

    def get(self, list_nos, offs):
        return self._get("get", list_nos, offs)

    # -- flat on-disk / wire image (the reference keeps compressed lists in memory only)
    def save(self, path):
        tw = int(lib().vidc_packed_total_words(self.h))
        words = np.zeros(max(tw, 1), np.uint64)
        check(lib().vidc_packed_export_all(self.ctx.h, self.h, ptr(words), tw))
        np.savez(path, offsets=self.offsets, bits=np.int64(self.bits), words=words[:tw])

    @classmethod
    def load(cls, path, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        z = np.load(path)
        off = _as_offsets(z["offsets"])
        words = np.ascontiguousarray(z["words"], dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vidc_packed_import(ctx.h, off.size - 1, ptr(off), int(z["bits"]), ptr(words) if words.size else None,
                                       words.size, C.byref(h)))
        return cls(h, ctx, off)

    def export_bytes(self, list_no):
        n = int(self.offsets[list_no + 1] - self.offsets[list_no])
        nb = (n * self.bits + 7) // 8
        buf = np.zeros(max(nb, 1), np.uint8)
        check(lib().vidc_packed_export(self.ctx.h, self.h, list_no, ptr(buf), nb))
        return buf[:nb]


class EfLists(_ListCodec):
    """Elias-Fano coded lists (vidc_ef), succinct::elias_fano geometry."""

    _prefix = "vidc_ef"

    @property
    def offsets(self):
        """CSR offsets of the decoded output (graph objects fetch the edge counts from the device on first use)."""
        return self._offsets_from_info()

    @classmethod
    def encode(cls, offsets, ids, want_perm=False, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        d_off = _cuda_offsets(offsets, ctx)
        if d_off is not None:  # device offsets: ntotal = ids.numel(), checked against offsets[-1] on the device
            d_ids = _dev_ids_dev(ids, d_off)
            ntotal, nlist = d_ids.numel(), d_off.numel() - 1
            h = C.c_void_p()
            check(lib().vidc_ef_encode_dev(ctx.h, nlist, ptr(d_off), ntotal, ptr(d_ids) if ntotal else None,
                                           _lib.VIDC_EF_WANT_PERM if want_perm else 0, C.byref(h)))
            return cls(h, ctx, None, nlist, ntotal)
        off = _as_offsets(offsets)
        ntotal = int(off[-1])
        d_ids = _dev_ids(ids, ntotal) if ntotal else None
        h = C.c_void_p()
        check(lib().vidc_ef_encode(ctx.h, off.size - 1, ptr(off), ptr(d_ids),
                                   _lib.VIDC_EF_WANT_PERM if want_perm else 0, C.byref(h)))
        return cls(h, ctx, off)

    def append(self, list_nos, ids, want_perm=False, labels=True, invalid=None):
        """A batch of (list number, id) pairs merged into the lists of this object -> (NEW EfLists, labels); this object stays valid
        and unchanged (vidc_ef_append_dev).  A label's offset is the entry's place in the ascending merged list.  See _append."""
        h, lab = _append(lib().vidc_ef_append_dev, self, list_nos, ids, (_lib.VIDC_EF_WANT_PERM if want_perm else 0,), labels, invalid)
        return type(self)(h, self.ctx, None, self._nlist if self._offsets is None else self._offsets.size - 1, None), lab

    @property
    def compressed_bytes(self):
        return int(lib().vidc_ef_compressed_bytes(self.h))

    def info(self):
        n = self._nlist if self._offsets is None else self._offsets.size - 1
        sizes = np.zeros(max(n, 1), np.uint32)
        lb = np.zeros(max(n, 1), np.uint32)
        uni = np.zeros(max(n, 1), np.uint64)
        check(lib().vidc_ef_list_info(self.h, ptr(sizes), ptr(lb), ptr(uni)))
        return dict(sizes=sizes[:n], low_bits=lb[:n], universe=uni[:n])

    def get(self, list_nos, offs):
        return self._get("get", list_nos, offs)

    def perm(self):
        p = np.zeros(max(self.ntotal, 1), np.uint32)
        check(lib().vidc_ef_perm(self.ctx.h, self.h, ptr(p)))
        return p[: self.ntotal]

    @classmethod
    def encode_rows(cls, rows, ctx=None):
        """rows: int32 CUDA tensor [N, K], -1 terminated (EliasFanoNSGGraph, altid_impl.cpp:53-90)."""
        torch = _torch()
        ctx = _lib.default_context() if ctx is None else ctx
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2
        rows = rows.contiguous()
        N, K = rows.shape
        h = C.c_void_p()
        check(lib().vidc_ef_encode_rows(ctx.h, N, K, ptr(rows) if N else None, C.byref(h)))
        obj = cls(h, ctx, None)
        obj._nlist = N
        obj.K = K
        return obj

    def decode_rows(self, nodes, K=None, want_counts=True):
        """-> (int32 [m, K] CUDA tensor, -1 padded; edge counts or None).  `want_counts=False` keeps the per-node
        edge counts on the device."""
        torch = _torch()
        K = K or self.K
        if nodes is not None and _is_cuda(nodes):  # device nodes (vidc_ef_decode_rows_dev): counts stay on the device too
            return _decode_rows_dev(lib().vidc_ef_decode_rows_dev, self, nodes, K, want_counts)
        if nodes is None:  # every node, in order
            nd, m = None, self._nlist if self._offsets is None else self._offsets.size - 1
        else:
            nd = np.ascontiguousarray(nodes, dtype=np.uint64)
            m = nd.size
        out = torch.empty((max(m, 1), K), dtype=torch.int32, device="cuda")
        counts = np.zeros(max(m, 1), np.uint32) if want_counts else None
        check(lib().vidc_ef_decode_rows(self.ctx.h, self.h, m, ptr(nd), K, ptr(out), ptr(counts)))
        return out[:m], (counts[:m] if want_counts else None)

    def decode_gather(self, list_nos, item_slot, item_off):
        """ids[i] = list_nos[item_slot[i]][item_off[i]]: the touched lists decoded and the results picked on the device,
        8 bytes per result copied to the host (vidc_ef_decode_gather)."""
        return _decode_gather(lib().vidc_ef_decode_gather, self, list_nos, item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids (int64 CUDA tensor), on the device: the decode section of
        a search whose labels come from a GPU top-k (vidc_ef_translate_labels_dev).  Negative labels and labels outside the
        object give -1; the latter are added to `invalid` (optional 1-element int64 CUDA tensor).  `out` may be `labels`."""
        return _translate_labels(lib().vidc_ef_translate_labels_dev, self, labels, out, invalid)

    # -- flat on-disk / wire image (the reference keeps compressed lists in memory only)
    def save(self, path):
        lw, hw = C.c_uint64(), C.c_uint64()
        check(lib().vidc_ef_stream_words(self.h, C.byref(lw), C.byref(hw)))
        low, high = np.zeros(lw.value, np.uint64), np.zeros(hw.value, np.uint64)
        check(lib().vidc_ef_export_all(self.ctx.h, self.h, ptr(low), low.size, ptr(high), high.size))
        info = self.info()
        np.savez(path, offsets=self.offsets, low_bits=info["low_bits"], universe=info["universe"], low=low, high=high,
                 K=np.int64(getattr(self, "K", 0)))

    @classmethod
    def load(cls, path, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        z = np.load(path)
        off = _as_offsets(z["offsets"])
        lb = np.ascontiguousarray(z["low_bits"], dtype=np.uint32)
        uni = np.ascontiguousarray(z["universe"], dtype=np.uint64)
        low = np.ascontiguousarray(z["low"], dtype=np.uint64)
        high = np.ascontiguousarray(z["high"], dtype=np.uint64)
        h = C.c_void_p()
        check(lib().vidc_ef_import(ctx.h, off.size - 1, ptr(off), ptr(lb) if lb.size else None, ptr(uni) if uni.size else None,
                                   ptr(low), low.size, ptr(high), high.size, C.byref(h)))
        obj = cls(h, ctx, off)
        if int(z["K"]):
            obj.K = int(z["K"])
        return obj

    def export(self, list_no):
        """-> (low words, high words, low_nbits, high_nbits) of one list."""
        lb, hb = C.c_uint64(), C.c_uint64()
        check(lib().vidc_ef_export(self.ctx.h, self.h, list_no, None, 0, None, 0, C.byref(lb), C.byref(hb)))
        lw, hw = (lb.value + 63) // 64, (hb.value + 63) // 64
        low = np.zeros(max(lw, 1), np.uint64)
        high = np.zeros(max(hw, 1), np.uint64)
        check(lib().vidc_ef_export(self.ctx.h, self.h, list_no, ptr(low), lw, ptr(high), hw, C.byref(lb), C.byref(hb)))
        return low[:lw], high[:hw], int(lb.value), int(hb.value)


class CompactRows:
    """CompactBitNSGGraph storage (vidc_compact): N rows x ceil(K*bits/8) bytes, sentinel N ends a row."""

    def __init__(self, handle, ctx, N, K):
        self.h, self.ctx, self.N, self.K = handle, ctx, N, K

    def __del__(self):
        try:  # may run during interpreter shutdown, after module globals are gone
            if getattr(self, "h", None):
                lib().vidc_compact_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @classmethod
    def encode_rows(cls, rows, ctx=None):
        torch = _torch()
        ctx = _lib.default_context() if ctx is None else ctx
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).cuda()
        assert rows.is_cuda and rows.dtype == torch.int32 and rows.dim() == 2
        rows = rows.contiguous()
        N, K = rows.shape
        h = C.c_void_p()
        check(lib().vidc_compact_rows_encode(ctx.h, N, K, ptr(rows) if N else None, C.byref(h)))
        return cls(h, ctx, N, K)

    def update_rows(self, nodes, rows, n_new=None, invalid=None):
        """Rows replaced and nodes added -> a NEW CompactRows; this object stays valid and unchanged: update_rows(self, ...) below."""
        return update_rows(self, nodes, rows, n_new=n_new, invalid=invalid)

    @property
    def bits(self):
        return int(lib().vidc_compact_bits(self.h))

    @property
    def stride(self):
        return int(lib().vidc_compact_stride(self.h))

    @property
    def size_in_bytes(self):
        return int(lib().vidc_compact_size_in_bytes(self.h))

    def decode_rows(self, nodes, K=None, want_counts=True):
        """nodes=None: every node in order (no index array).  A CUDA tensor of nodes takes vidc_compact_rows_decode_dev: the counts
        then come back as an int32 CUDA tensor (or None)."""
        torch = _torch()
        if nodes is not None and _is_cuda(nodes):
            return _decode_rows_dev(lib().vidc_compact_rows_decode_dev, self, nodes, self.K, want_counts, pass_K=False)
        if nodes is None:
            nd, m = None, self.N
        else:
            nd = np.ascontiguousarray(nodes, dtype=np.uint64)
            m = nd.size
        out = torch.empty((max(m, 1), self.K), dtype=torch.int32, device="cuda")
        counts = np.zeros(max(m, 1), np.uint32) if want_counts else None
        check(lib().vidc_compact_rows_decode(self.ctx.h, self.h, m, ptr(nd), ptr(out), ptr(counts)))
        return out[:m], (counts[:m] if want_counts else None)

    def export_row(self, node):
        buf = np.zeros(self.stride, np.uint8)
        check(lib().vidc_compact_export_row(self.ctx.h, self.h, node, ptr(buf), self.stride))
        return buf


def update_rows(obj, nodes, rows, n_new=None, invalid=None, precision_mode=VIDC_PREC_REFERENCE):
    """Rows of a graph object replaced and nodes added -> a NEW object of obj's class; obj stays valid and unchanged
    (vidc_{compact,ef,roc}_update_rows_dev).  obj: what CompactRows / EfLists / RocLists.encode_rows built (Elias-Fano and ROC: K <= 64).
    CompactRows re-packs every row (the sentinel is the node count) at the width of the new count; EfLists encodes the batch rows into
    scratch and rewrites its arena at the geometry a fresh object of the updated rows would have; RocLists encodes only the batch rows
    and copies every other row's stream (precision_mode: the mode obj was built with; ignored by the other two).  See _update_rows for
    the arguments.  (A function, as removal.remove is: the list classes keep the methods they had.)"""
    if isinstance(obj, CompactRows):
        h, n = _update_rows(lib().vidc_compact_update_rows_dev, obj, obj.K, obj.N, nodes, rows, n_new, (), invalid)
        return type(obj)(h, obj.ctx, n, obj.K)
    K = getattr(obj, "K", 0)
    if isinstance(obj, EfLists):
        n_old = obj._nlist if obj._offsets is None else obj._offsets.size - 1
        h, n = _update_rows(lib().vidc_ef_update_rows_dev, obj, K, n_old, nodes, rows, n_new, (), invalid)
        new = type(obj)(h, obj.ctx, None)
        new._nlist = n
    elif isinstance(obj, RocLists):
        h, _ = _update_rows(lib().vidc_roc_update_rows_dev, obj, K, obj.nlist, nodes, rows, n_new, (int(precision_mode),), invalid)
        new = type(obj)(h, obj.ctx, None)
    else:
        raise _lib.VidcError(f"update_rows: {type(obj).__name__} holds no graph rows")
    new.K = K
    return new


class WaveletTreeLists(_ListCodec):
    """Wavelet tree over list_nos[id] (vidc_wt): id = select(offset + 1, list_no)."""

    _prefix = "vidc_wt"

    @property
    def offsets(self):
        """CSR offsets (host).  Objects built from device offsets copy the object's own device array on first use."""
        return self._offsets_from_symbol()

    @classmethod
    def build(cls, offsets, ids, wt_type=0, ctx=None):
        ctx = _lib.default_context() if ctx is None else ctx
        d_off = _cuda_offsets(offsets, ctx)
        if d_off is not None:  # device offsets: ntotal = ids.numel(), checked against offsets[-1] on the device
            d_ids = _dev_ids_dev(ids, d_off)
            ntotal, nlist = d_ids.numel(), d_off.numel() - 1
            h = C.c_void_p()
            check(lib().vidc_wt_build_dev(ctx.h, nlist, ptr(d_off), ntotal, ptr(d_ids) if ntotal else None, int(wt_type),
                                          C.byref(h)))
            return cls(h, ctx, None, nlist, ntotal)
        off = _as_offsets(offsets)
        ntotal = int(off[-1])
        d_ids = _dev_ids(ids, ntotal) if ntotal else None
        h = C.c_void_p()
        check(lib().vidc_wt_build(ctx.h, off.size - 1, ptr(off), ptr(d_ids), int(wt_type), C.byref(h)))
        return cls(h, ctx, off)

    def append(self, list_nos, ids, labels=True, invalid=None):
        """A batch of (list number, id) pairs behind the lists of this object -> (NEW WaveletTreeLists, labels); this object stays
        valid and unchanged (vidc_wt_append_dev).  The merged lists must be what `build` demands: a permutation of 0 .. ntotal - 1,
        ascending inside every list (a batch of ids ntotal .. ntotal + n - 1 in add order is).  See _append."""
        h, lab = _append(lib().vidc_wt_append_dev, self, list_nos, ids, (), labels, invalid)
        return type(self)(h, self.ctx, None, self._nlist if self._offsets is None else self._offsets.size - 1, None), lab

    @property
    def size_in_bytes(self):
        return int(lib().vidc_wt_size_in_bytes(self.h))

    @property
    def levels(self):
        return int(lib().vidc_wt_levels(self.h))

    def decode_gather(self, list_nos, item_slot, item_off):
        """ids[i] = list_nos[item_slot[i]][item_off[i]]: the touched lists decoded and the results picked on the device,
        8 bytes per result copied to the host (vidc_wt_decode_gather)."""
        return _decode_gather(lib().vidc_wt_decode_gather, self, list_nos, item_slot, item_off)

    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids (int64 CUDA tensor), on the device: the decode section of
        a search whose labels come from a GPU top-k (vidc_wt_translate_labels_dev).  Negative labels and labels outside the
        object give -1; the latter are added to `invalid` (optional 1-element int64 CUDA tensor).  `out` may be `labels`."""
        return _translate_labels(lib().vidc_wt_translate_labels_dev, self, labels, out, invalid)

    def select(self, list_nos, offs):
        return self._get("select", list_nos, offs)


class _BorrowedRoc(RocLists):
    """The inner object of a RocSegLists: a RocLists view of a handle its owner destroys (the owner is kept alive meanwhile)."""

    def __init__(self, handle, ctx, owner):
        super().__init__(handle, ctx, None)
        self._owner = owner

    def __del__(self):
        self.h = None


def _check_seg_params(seg_ids, universe_bits):
    """seg_ids: None (the library's default) or a power of two in [16, 65536]; universe_bits: None (from the ids) or 1 .. 31 -> the
    C call's two integers (0 = the default).  Real exceptions: a bad value must not reach the library as a 0."""
    T = 0 if seg_ids is None else int(seg_ids)
    B = 0 if universe_bits is None else int(universe_bits)
    if seg_ids is not None and (T < 16 or T > 65536 or T & (T - 1)):
        raise ValueError(f"seg_ids must be a power of two in [16, 65536], not {seg_ids}")
    if universe_bits is not None and not 1 <= B <= 31:
        raise ValueError(f"universe_bits must be in 1 .. 31, not {universe_bits}")
    return T, B


class RocSegLists(_ListCodec):
    """Segmented ROC lists (vidc_rocseg): every list longer than seg_ids is cut by value range into 2^k segments, each an independent
    ANS chain of the inner RocLists (`inner`, encoded with VIDC_PREC_EXACT).  Opt-in and not reference-identical; append, remove,
    regroup and sharding are out of scope."""

    _prefix = "vidc_rocseg"

    @property
    def offsets(self):
        """CSR offsets of the decoded output: the inner object's offsets at the first segment of every list"""
        if self._offsets is None:
            seg_first, _ = self.seg_info()
            self._offsets = np.ascontiguousarray(self.inner.offsets[seg_first.astype(np.int64)], dtype=np.uint64)
        return self._offsets

    @classmethod
    def encode(cls, offsets, ids, seg_ids=None, universe_bits=None, want_perm=False, ctx=None):
        """offsets: host (numpy / list) or an int64 / uint64 CUDA tensor; ids: int64 / uint64 CUDA tensor (numpy arrays are uploaded)"""
        T, B = _check_seg_params(seg_ids, universe_bits)
        ctx = _lib.default_context() if ctx is None else ctx
        flags = _lib.VIDC_ROC_WANT_PERM if want_perm else 0
        h = C.c_void_p()
        d_off = _cuda_offsets(offsets, ctx)
        if d_off is not None:
            d_ids = _dev_ids_dev(ids, d_off)
            check(lib().vidc_rocseg_encode_dev(ctx.h, d_off.numel() - 1, ptr(d_off), d_ids.numel(), ptr(d_ids) if d_ids.numel() else None,
                                               T, B, flags, C.byref(h)))
            return cls(h, ctx, None)
        off = _as_offsets(offsets)
        if off[0] != 0:
            raise ValueError("offsets must start at 0")
        d_ids = _dev_ids(ids, int(off[-1])) if off[-1] else None
        check(lib().vidc_rocseg_encode(ctx.h, off.size - 1, ptr(off), ptr(d_ids), T, B, flags, C.byref(h)))
        return cls(h, ctx, off)

    @classmethod
    def wrap(cls, inner, seg_first, shift, seg_ids, universe_bits):
        """vidc_rocseg_wrap: a segmented object over an imported RocLists and an untrusted map.  On success `inner` is consumed (its
        handle moves into the new object); on a VidcError it stays usable."""
        T, B = _check_seg_params(seg_ids, universe_bits)
        sf = np.ascontiguousarray(seg_first, dtype=np.uint64)
        sh = np.ascontiguousarray(shift, dtype=np.uint8)
        if sf.ndim != 1 or sf.size != sh.size + 1:
            raise ValueError("seg_first needs one entry more than shift")
        h = C.c_void_p()
        check(lib().vidc_rocseg_wrap(inner.ctx.h, inner.h, sh.size, ptr(sf), ptr(sh) if sh.size else None, T, B, C.byref(h)))
        inner.h = None  # (owned by the new object now)
        return cls(h, inner.ctx, None)

    # -- flat image: the inner object's ROC export plus the map
    def save(self, path):
        inner = self.inner
        info = inner.info()
        seg_first, shift = self.seg_info()
        np.savez(path, kind=np.array("rocseg"), offsets=inner.offsets, precision=info["precision"], heads=info["heads"], nwords=info["nwords"],
                 mt_draws=info["mt_draws"], words=inner.all_words(), seg_first=seg_first, shift=shift, seg_ids=np.int64(self.seg_ids),
                 universe_bits=np.int64(self.universe_bits))

    @classmethod
    def load(cls, path, ctx=None):
        with np.load(path) as z:
            inner = RocLists.from_streams(z["offsets"], z["precision"], z["heads"], z["nwords"], z["words"], z["mt_draws"], ctx=ctx)
            return cls.wrap(inner, z["seg_first"], z["shift"], int(z["seg_ids"]), int(z["universe_bits"]))

    # -- properties
    @property
    def nlist(self):
        return int(lib().vidc_rocseg_nlist(self.h))

    @property
    def ntotal(self):
        return int(lib().vidc_rocseg_ntotal(self.h))

    @property
    def compressed_bytes(self):
        """the inner object's bytes + 4 per segment of every list that is split"""
        return int(lib().vidc_rocseg_compressed_bytes(self.h))

    @property
    def seg_ids(self):
        return int(lib().vidc_rocseg_seg_ids(self.h))

    @property
    def universe_bits(self):
        return int(lib().vidc_rocseg_universe_bits(self.h))

    @property
    def inner(self):
        """the inner RocLists (borrowed): info, words, all_words serve parity checks and saving"""
        return _BorrowedRoc(C.c_void_p(lib().vidc_rocseg_inner(self.h)), self.ctx, self)

    def seg_info(self):
        """-> (seg_first uint64[nlist + 1], shift uint8[nlist]): the first inner list of every list and its shift"""
        n = self.nlist
        seg_first = np.zeros(n + 1, np.uint64)
        shift = np.zeros(max(n, 1), np.uint8)
        check(lib().vidc_rocseg_seg_info(self.h, ptr(seg_first), ptr(shift)))
        return seg_first, shift[:n]

    def info(self):
        """the map, the parameters and the inner object's per-segment metadata"""
        seg_first, shift = self.seg_info()
        return dict(seg_first=seg_first, shift=shift, seg_ids=self.seg_ids, universe_bits=self.universe_bits, inner=self.inner.info())

    def perm(self):
        """output position -> input position within the list (objects encoded with want_perm)"""
        p = np.zeros(max(self.ntotal, 1), np.uint32)
        check(lib().vidc_rocseg_perm(self.ctx.h, self.h, ptr(p)))
        return p[: self.ntotal]

    # -- decode (decode_all, decode_lists: _ListCodec)
    def translate_labels(self, labels, out=None, invalid=None):
        """Faiss labels (int64 CUDA tensor, list_no << 32 | offset) -> ids, on the device (vidc_rocseg_translate_labels_dev): only the
        touched SEGMENTS decode.  Negative labels and labels outside the object give -1; the latter are added to `invalid`.  `out` may
        be `labels`."""
        return _translate_labels(lib().vidc_rocseg_translate_labels_dev, self, labels, out, invalid)

    def decode_gather(self, list_nos, item_slot, item_off):
        """ids[i] = list_nos[item_slot[i]][item_off[i]] -> numpy int64: the labels are built on the device and go through
        translate_labels; 8 bytes per result come back.  An item outside its list is a VidcError, as in the other containers."""
        torch = _torch()
        ln = np.ascontiguousarray(list_nos, dtype=np.int64)
        sl = np.ascontiguousarray(item_slot, dtype=np.int64)
        of = np.ascontiguousarray(item_off, dtype=np.int64)
        if sl.size != of.size:
            raise ValueError("item_slot and item_off must have one entry per item")
        if not sl.size:
            return np.zeros(0, np.int64)
        if ln.size == 0 or int(sl.min()) < 0 or int(sl.max()) >= ln.size or int(of.min()) < 0 or int(of.max()) >= 1 << 32:
            raise _lib.VidcError("decode_gather: an item names no list of the request")
        d_ln = torch.from_numpy(ln).cuda()
        labels = (d_ln[torch.from_numpy(sl).cuda()] << 32) | torch.from_numpy(of).cuda()
        invalid = torch.zeros(1, dtype=torch.int64, device=labels.device)
        ids = self.translate_labels(labels, out=labels, invalid=invalid)
        if int(invalid.item()):
            raise _lib.VidcError(f"decode_gather: {int(invalid.item())} items are outside their list")
        return ids.cpu().numpy()

    @property
    def last_decode_handed_back(self):
        return int(lib().vidc_rocseg_last_decode_handed_back(self.h))
