"""Removal of (list number, id) batches from the compressed list containers (vidc_*_remove_dev).

    new_obj, mask = removal.remove(obj, list_nos, ids)      # pairs mode: entry of list l leaves iff (l, id) is in the batch
    new_obj, mask = removal.remove(obj, None, ids)          # any-list mode: Faiss's remove_ids over an IDSelectorBatch

Objects are immutable: `obj` stays valid and unchanged.  The new object is, word for word, what the codec's encoder builds from the
surviving lists (order kept).  mask[p] (uint8 CUDA tensor, ntotal_old entries) is 1 where position p of obj.decode_all() was removed:
a caller that keeps per-entry payload (the vector codes) drops the same rows.  Packed bits and Elias-Fano are rebuilt on the device;
ROC re-encodes only the lists that lose an entry and copies the streams of the others.  A wavelet tree holds a permutation of
0 .. ntotal - 1, which a removal breaks: it has no remove.  A sharding.DeviceShards is forwarded to DeviceShards.remove
(vidc_remove_sharded_dev): every shard removes from its own lists, the mask and the counters are the unsharded object's.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import VIDC_PREC_REFERENCE, VidcError, check, lib, ptr
from .sharding import DeviceShards
from .codecs import EfLists, PackedLists, RocLists, WaveletTreeLists, _dev_array, _is_cuda, _on_torch_stream, _torch


def _counter(x, what, device):
    torch = _torch()
    if x is not None and (not _is_cuda(x) or x.dtype != torch.int64 or x.numel() != 1 or not x.is_contiguous() or x.device != device):
        raise ValueError(f"{what} must be a 1-element int64 CUDA tensor on the batch's device")
    return x


def _call(fn, obj, extra, list_nos, ids, removed, missing, invalid):
    """The argument handling every remove shares -> (handle of the new object, mask or None).  fn(ctx, obj, n, list_nos, ids, *extra,
    &out, removed, missing, invalid); obj has .ctx, .h and .ntotal."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: remove needs an MI355X (there is no CPU fallback)")
    if isinstance(list_nos, np.ndarray):
        list_nos = torch.from_numpy(np.ascontiguousarray(list_nos, dtype=np.int64)).cuda()
    if isinstance(ids, np.ndarray):
        ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    if not _is_cuda(ids) or ids.dtype not in (torch.int64, torch.uint64):
        raise TypeError("ids must be an int64 / uint64 CUDA tensor")
    di = _dev_array(ids.reshape(-1), obj.ctx, "ids")
    n = di.numel()
    ln = None
    if list_nos is not None:
        if not _is_cuda(list_nos) or list_nos.dtype != torch.int64:
            raise TypeError("list_nos must be an int64 CUDA tensor (or None: any-list mode)")
        if list_nos.numel() != n:
            raise ValueError("list_nos and ids must have one entry per pair")
        ln = _dev_array(list_nos.reshape(-1), obj.ctx, "list_nos")
        if n == 0:  # (a NULL list array would select any-list mode: the same empty result)
            ln = None
    ntotal = 0
    mask = None
    if removed is not None and removed is not False:
        ntotal = obj.ntotal
    if removed is True:
        mask = torch.empty(max(ntotal, 1), dtype=torch.uint8, device=di.device)
    elif removed is not None and removed is not False:
        if not _is_cuda(removed) or removed.dtype != torch.uint8 or not removed.is_contiguous() or removed.numel() != ntotal \
                or removed.device != di.device:
            raise ValueError("removed must be a contiguous uint8 CUDA tensor with one entry per id of the object, on the batch's device")
        mask = removed
    _counter(missing, "missing", di.device)
    _counter(invalid, "invalid", di.device)
    _on_torch_stream(obj.ctx)
    h = C.c_void_p()
    check(fn(obj.ctx.h, obj.h, n, ptr(ln), ptr(di) if n else None, *extra, C.byref(h), ptr(mask), ptr(missing), ptr(invalid)))
    return h, (None if mask is None else mask[:ntotal])


def remove(obj, list_nos, ids, *, precision_mode=VIDC_PREC_REFERENCE, want_perm=False, removed=True, missing=None, invalid=None):
    """-> (NEW object of obj's class, removed mask or None).

    list_nos: int64 CUDA tensor (negative = skipped, >= nlist = skipped and counted in `invalid`), or None for any-list mode; ids:
    int64 / uint64 CUDA tensor with one entry per pair; numpy arrays are uploaded once.  precision_mode (ROC): the mode the object was
    built with; want_perm (ROC, Elias-Fano): keep the permutation of the new object.  removed: True (a new uint8 CUDA tensor), False /
    None (none) or a contiguous uint8 CUDA tensor of obj.ntotal entries to fill.  missing / invalid (optional): 1-element int64 CUDA
    tensors the number of valid pairs that matched nothing / of list numbers >= nlist is added to.  Runs on torch's current stream;
    the call synchronises.  A DeviceShards goes to DeviceShards.remove (global list numbers, arrays on the home device)."""
    if isinstance(obj, WaveletTreeLists):
        raise VidcError("remove: a wavelet tree holds a permutation of 0 .. ntotal - 1, which a removal breaks")
    if isinstance(obj, DeviceShards):
        args = {} if obj.kind == 0 else {"want_perm": want_perm}
        if obj.kind == 2:
            args["precision_mode"] = precision_mode
        return obj.remove(list_nos, ids, removed=removed, missing=missing, invalid=invalid, **args)
    if isinstance(obj, RocLists):
        fn, extra = lib().vidc_roc_remove_dev, (int(precision_mode), _lib.VIDC_ROC_WANT_PERM if want_perm else 0)
    elif isinstance(obj, EfLists):
        fn, extra = lib().vidc_ef_remove_dev, (_lib.VIDC_EF_WANT_PERM if want_perm else 0,)
    elif isinstance(obj, PackedLists):
        fn, extra = lib().vidc_packed_remove_dev, ()
    else:
        raise VidcError(f"remove: {type(obj).__name__} holds no removable lists")
    h, mask = _call(fn, obj, extra, list_nos, ids, removed, missing, invalid)
    if isinstance(obj, RocLists):
        new = type(obj)(h, obj.ctx, None)
    else:
        new = type(obj)(h, obj.ctx, None, obj._nlist if obj._offsets is None else obj._offsets.size - 1, None)
    return new, mask
