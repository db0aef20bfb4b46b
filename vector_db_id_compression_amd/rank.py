"""Rank of (list number, id) batches inside compressed Elias-Fano lists and graph rows (vidc_ef_rank_dev): how many entries of list
list_nos[i] are smaller than ids[i], answered in the compressed streams -- nothing is decoded, nothing allocated by the library.

    r = rank.rank(obj, list_nos, ids)               # r[i] entries of list list_nos[i] are < ids[i]; -1 for a skipped / invalid list
    hit = rank.contains(obj, list_nos, ids)         # is ids[i] an entry of list list_nos[i]?
    c = rank.count_range(obj, list_nos, lo, hi)     # entries with lo[i] <= id < hi[i]

r is the offset of the first entry >= the id in the list's ascending order (what decode_lists and translate_labels use): where r is
below the list's size, list_no << 32 | r is a label whose translate_labels is the successor, and of equal entries r is the first (the
label locate.locate answers).  For graph objects the list is the node.  Only EfLists can be searched compressed: packed bits keep
input order, the wavelet tree has locate.locate, ROC streams have to be decoded.
"""
import numpy as np

from ._lib import VidcError, check, lib, ptr
from .codecs import EfLists, _dev_array, _is_cuda, _on_torch_stream, _torch
from .removal import _counter


def _ids_tensor(ids, obj, what):
    torch = _torch()
    if isinstance(ids, np.ndarray):
        ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int64)).cuda()
    if not _is_cuda(ids) or ids.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{what} must be an int64 / uint64 CUDA tensor")
    return _dev_array(ids.reshape(-1), obj.ctx, what)


def rank(obj, list_nos, ids, *, out=None, found=None, invalid=None):
    """-> ranks (int64 CUDA tensor, one per pair, batch order).

    list_nos: int64 CUDA tensor (negative = skipped, >= nlist = skipped and counted in `invalid`; both give -1); ids: int64 / uint64
    CUDA tensor with one entry per pair, compared as unsigned 64-bit numbers; numpy arrays are uploaded once.  out (optional): a
    contiguous int64 CUDA tensor with one entry per pair to fill; found (optional): a contiguous uint8 CUDA tensor with one entry per
    pair that gets 1 where the id is an entry of its list, else 0 (neither may overlap the inputs).  invalid (optional): 1-element int64
    CUDA tensor the number of list numbers >= nlist is added to.  Runs on torch's current stream; only enqueues."""
    if not isinstance(obj, EfLists):
        raise VidcError(f"rank: {type(obj).__name__} cannot be searched compressed (only Elias-Fano lists and rows can: packed bits are "
                        "unsorted, the wavelet tree has locate, ROC, segmented, sharded and compact-row objects are out of scope)")
    if list_nos is None:
        raise VidcError(f"rank: {type(obj).__name__}: list_nos=None: a rank is inside one list, there is no any-list mode")
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: rank needs an MI355X (there is no CPU fallback)")
    if isinstance(list_nos, np.ndarray):
        list_nos = torch.from_numpy(np.ascontiguousarray(list_nos, dtype=np.int64)).cuda()
    di = _ids_tensor(ids, obj, "ids")
    n = di.numel()
    if not _is_cuda(list_nos) or list_nos.dtype != torch.int64:
        raise TypeError("list_nos must be an int64 CUDA tensor")
    if list_nos.numel() != n:
        raise ValueError("list_nos and ids must have one entry per pair")
    ln = _dev_array(list_nos.reshape(-1), obj.ctx, "list_nos")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=di.device)
    elif not _is_cuda(out) or out.dtype != torch.int64 or not out.is_contiguous() or out.numel() != n or out.device != di.device:
        raise ValueError("out must be a contiguous int64 CUDA tensor with one entry per pair, on the batch's device")
    if found is not None and (not _is_cuda(found) or found.dtype != torch.uint8 or not found.is_contiguous() or found.numel() != n
                              or found.device != di.device):
        raise ValueError("found must be a contiguous uint8 CUDA tensor with one entry per pair, on the batch's device")
    _counter(invalid, "invalid", di.device)
    if n == 0:
        return out
    _on_torch_stream(obj.ctx)
    try:
        check(lib().vidc_ef_rank_dev(obj.ctx.h, obj.h, n, ptr(ln), ptr(di), ptr(out), ptr(found), ptr(invalid)))
    except VidcError as e:
        raise VidcError(f"rank: {type(obj).__name__}: {e}") from None
    return out


def contains(obj, list_nos, ids):
    """-> bool CUDA tensor, one per pair: ids[i] is an entry of list list_nos[i] (False for a skipped or invalid list number)."""
    torch = _torch()
    if not isinstance(obj, EfLists) or list_nos is None or not torch.cuda.is_available():
        return rank(obj, list_nos, ids)  # (raises: the refusals are rank's)
    di = _ids_tensor(ids, obj, "ids")
    found = torch.empty(di.numel(), dtype=torch.uint8, device=di.device)
    rank(obj, list_nos, di, found=found)
    return found.bool()


def count_range(obj, list_nos, lo, hi):
    """-> int64 CUDA tensor, one per pair: the entries of list list_nos[i] with lo[i] <= id < hi[i] (unsigned), 0 where hi[i] < lo[i] and
    for a skipped or invalid list number.  One call on the concatenated batch: rank(hi) - rank(lo)."""
    if not isinstance(obj, EfLists) or list_nos is None or not _torch().cuda.is_available():
        return rank(obj, list_nos, lo)  # (raises)
    torch = _torch()
    if isinstance(list_nos, np.ndarray):
        list_nos = torch.from_numpy(np.ascontiguousarray(list_nos, dtype=np.int64)).cuda()
    dlo, dhi = _ids_tensor(lo, obj, "lo").view(torch.int64), _ids_tensor(hi, obj, "hi").view(torch.int64)
    n = dlo.numel()
    if dhi.numel() != n or not _is_cuda(list_nos) or list_nos.numel() != n:
        raise ValueError("list_nos, lo and hi must have one entry per pair")
    ln = list_nos.reshape(-1)
    r = rank(obj, torch.cat([ln, ln]), torch.cat([dlo, dhi]))
    return torch.clamp(r[n:] - r[:n], min=0)  # (skipped pairs: -1 - -1 = 0; hi < lo: a negative difference)
