"""Location of (list number, id) batches in the compressed list containers (vidc_*_locate_dev): id -> label, the inverse of
translate_labels and what Faiss keeps a DirectMap for (reconstruct, reconstruct_batch, update_vectors).

    labels = locate.locate(obj, list_nos, ids)      # pairs mode: id i is looked for in list list_nos[i] only
    labels = locate.locate(obj, None, ids)          # any-list mode: id i is looked for in every list

labels[i] = list_no << 32 | offset of an entry equal to ids[i], the offset in the object's own order (what decode_lists and
translate_labels use), or -1.  Of several matching entries the smallest label wins (lowest list, then lowest offset); wherever
labels[i] >= 0, obj.translate_labels(labels)[i] == ids[i].  The object is not changed.  Packed bits, Elias-Fano and ROC sort the
batch and search it from the decoded lists (ROC decodes only the lists the batch names; any-list mode decodes the whole object); a
wavelet tree walks every id down its levels.  Segmented ROC lists, sharded containers and graph objects are out of scope.
The search inside compressed Elias-Fano lists and graph rows, which decodes nothing, is rank.rank (vidc_ef_rank_dev).
"""
import numpy as np

from ._lib import VidcError, check, lib, ptr
from .codecs import EfLists, PackedLists, RocLists, WaveletTreeLists, _dev_array, _is_cuda, _on_torch_stream, _torch
from .removal import _counter


def locate(obj, list_nos, ids, *, out=None, missing=None, invalid=None):
    """-> labels (int64 CUDA tensor, one per pair, batch order).

    list_nos: int64 CUDA tensor (negative = skipped, >= nlist = skipped and counted in `invalid`), or None for any-list mode; ids:
    int64 / uint64 CUDA tensor with one entry per pair; numpy arrays are uploaded once.  out (optional): a contiguous int64 CUDA tensor
    with one entry per pair to fill (it must not overlap the inputs).  missing / invalid (optional): 1-element int64 CUDA tensors the
    number of valid pairs that got -1 / of list numbers >= nlist is added to.  Runs on torch's current stream; packed bits, Elias-Fano
    and ROC wait for their last kernel, a wavelet tree only enqueues."""
    fns = {PackedLists: "vidc_packed_locate_dev", EfLists: "vidc_ef_locate_dev", WaveletTreeLists: "vidc_wt_locate_dev",
           RocLists: "vidc_roc_locate_dev"}
    name = next((f for cls, f in fns.items() if isinstance(obj, cls)), None)
    if name is None:
        raise VidcError(f"locate: {type(obj).__name__} holds no lists to locate in (packed bits, Elias-Fano, ROC and wavelet-tree "
                        "lists do; segmented, sharded and graph objects are out of scope)")
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: locate needs an MI355X (there is no CPU fallback)")
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
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=di.device)
    elif not _is_cuda(out) or out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != n or out.device != di.device:
        raise ValueError("out must be a contiguous int64 CUDA tensor with one entry per pair, on the batch's device")
    _counter(missing, "missing", di.device)
    _counter(invalid, "invalid", di.device)
    if n == 0:
        return out
    _on_torch_stream(obj.ctx)
    try:
        check(getattr(lib(), name)(obj.ctx.h, obj.h, n, ptr(ln), ptr(di), ptr(out), ptr(missing), ptr(invalid)))
    except VidcError as e:
        raise VidcError(f"locate: {type(obj).__name__}: {e}") from None
    return out
