"""Subsets of the compressed list containers (vidc_*_subset_dev): Faiss's InvertedLists::copy_subset_to(other, subset_type, a1, a2).

    part, mask = subset.subset(obj, subset.ID_MOD, 3, 1)            # the entries whose id % 3 == 1, of every list, order kept
    part, mask = subset.subset(obj, subset.INVLIST, 0, nlist // 2)  # the lower half of the lists, whole

Objects are immutable: `obj` stays valid and unchanged.  The new object holds the same nlist lists and is, word for word, what the
codec's encoder builds from the taken entries.  mask[p] (uint8 CUDA tensor, obj.ntotal entries) is 1 where position p of
obj.decode_all() is in the subset: a caller that keeps per-entry payload (the vector codes) takes the same rows.  It is the inverse of
merge.merge: an index is split into shards by id range, id residue, list range or list fraction and merged back.  Packed bits and
Elias-Fano are rebuilt on the device; ROC copies the stream of every list that keeps all of its entries, empties the lists that keep
none and re-encodes only the rest.  With n = the size of list l, off[] = the offsets and T = ntotal, entry i of list l holding `id` is
taken iff

    ID_RANGE (0)          a1 <= id < a2
    ID_MOD (1)            id % a1 == a2                                        (a1 >= 1, a2 < a1)
    ELEMENT_RANGE (2)     i1 <= i < i2, i1 = off[l+1]*a1 // T - off[l]*a1 // T, i2 the same with a2   (a1 <= a2 <= T)
    INVLIST_FRACTION (3)  n*a2 // a1 <= i < n*(a2+1) // a1                     (1 <= a1 < 2^32, a2 < a1)
    INVLIST (4)           a1 <= l < a2

A wavelet tree holds a permutation of 0 .. ntotal - 1, which a subset breaks: it has no subset.  Segmented ROC lists, sharded
containers and graph objects are out of scope.
"""
import ctypes as C

from . import _lib
from ._lib import VIDC_PREC_REFERENCE, VidcError, check, lib, ptr
from .codecs import CompactRows, EfLists, PackedLists, RocLists, RocSegLists, WaveletTreeLists, _is_cuda, _on_torch_stream, _torch
from .sharding import DeviceShards

ID_RANGE, ID_MOD, ELEMENT_RANGE, INVLIST_FRACTION, INVLIST = range(5)


def subset(obj, subset_type, a1, a2, *, precision_mode=VIDC_PREC_REFERENCE, want_perm=False, taken=True):
    """-> (NEW object of obj's class, taken mask or None).

    subset_type: ID_RANGE .. INVLIST (0 .. 4); a1, a2: its arguments, in [0, 2^64).  precision_mode (ROC): the mode the object was
    built with; want_perm (ROC, Elias-Fano): keep the permutation of the new object, which is over the positions of the taken entries
    of each list.  taken: True (a new uint8 CUDA tensor), False / None (none) or a contiguous uint8 CUDA tensor of obj.ntotal entries
    to fill.  The size of the subset is the new object's ntotal.  Runs on torch's current stream; the call synchronises."""
    if isinstance(obj, WaveletTreeLists):
        raise VidcError("subset: WaveletTreeLists holds a permutation of 0 .. ntotal - 1, which a subset breaks")
    for cls in (RocSegLists, DeviceShards, CompactRows):
        if isinstance(obj, cls):
            raise VidcError(f"subset: {cls.__name__} is out of scope (segmented, sharded and graph objects have no subset)")
    if getattr(obj, "K", None) is not None:
        raise VidcError(f"subset: a graph-row {type(obj).__name__} holds no lists to take a subset of")
    if isinstance(obj, RocLists):
        name, extra = "vidc_roc_subset_dev", (int(precision_mode), _lib.VIDC_ROC_WANT_PERM if want_perm else 0)
    elif isinstance(obj, EfLists):
        name, extra = "vidc_ef_subset_dev", (_lib.VIDC_EF_WANT_PERM if want_perm else 0,)
    elif isinstance(obj, PackedLists):
        name, extra = "vidc_packed_subset_dev", ()
    else:
        raise VidcError(f"subset: {type(obj).__name__} holds no lists to take a subset of")
    subset_type, a1, a2 = int(subset_type), int(a1), int(a2)
    if min(a1, a2) < 0 or max(a1, a2) >> 64:
        raise ValueError("a1 and a2 must be in [0, 2^64)")
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: subset needs an MI355X (there is no CPU fallback)")
    ntotal = obj.ntotal
    mask = None
    if taken is True:
        mask = torch.empty(max(ntotal, 1), dtype=torch.uint8, device="cuda")
    elif taken is not None and taken is not False:
        if not _is_cuda(taken) or taken.dtype != torch.uint8 or not taken.is_contiguous() or taken.numel() != ntotal:
            raise ValueError("taken must be a contiguous uint8 CUDA tensor with one entry per id of the object")
        mask = taken
    _on_torch_stream(obj.ctx)
    h, n_taken = C.c_void_p(), C.c_uint64()
    try:
        check(getattr(lib(), name)(obj.ctx.h, obj.h, subset_type, a1, a2, *extra, C.byref(h), ptr(mask), C.byref(n_taken)))
    except VidcError as e:
        raise VidcError(f"subset: {type(obj).__name__}: {e}") from None
    if isinstance(obj, RocLists):
        new = type(obj)(h, obj.ctx, None, None, int(n_taken.value))
    else:
        new = type(obj)(h, obj.ctx, None, obj._nlist if obj._offsets is None else obj._offsets.size - 1, int(n_taken.value))
    return new, (None if mask is None else mask[:ntotal])
