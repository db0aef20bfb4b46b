"""Merge of two compressed list objects over the same lists (vidc_*_merge_dev): Faiss's InvertedLists::merge_from(other, add_id).

    new = merge.merge(a, b, add_id)                       # list l of the result = a_l ++ [x + add_id for x in b_l]
    src = torch.empty(a.ntotal + b.ntotal, dtype=torch.int64, device="cuda")
    new = merge.merge(a, b, add_id, src=src)              # src[q] = p >= 0: position p of a.decode_all(); ~p: position p of b's

`new` is the object the encoder builds from the merged lists, word for word; `a` and `b` stay valid and unchanged, and a is b is
allowed.  Nothing is sorted and no id crosses PCIe: packed bits, Elias-Fano and the wavelet tree decode both sides into scratch,
place them and run their device-offsets encoder; ROC re-encodes only the lists that hold ids of both sides (or shifted ids of b) and
copies every other list's stream.  A caller that keeps per-entry payload builds the merged payload with one gather through `src`.
Segmented ROC lists, sharded containers and graph objects are out of scope.
"""
import ctypes as C

from . import _lib
from ._lib import VIDC_PREC_REFERENCE, VidcError, check, lib, ptr
from .codecs import EfLists, PackedLists, RocLists, WaveletTreeLists, _is_cuda, _on_torch_stream, _torch

_CLASSES = (PackedLists, EfLists, WaveletTreeLists, RocLists)


def _class_of(obj):
    return next((cls for cls in _CLASSES if isinstance(obj, cls)), None)


def _nlist(obj):
    if obj._offsets is not None:
        return obj._offsets.size - 1
    return obj._nlist if obj._nlist is not None else obj.nlist


def _codec_call(cls, args):
    """-> (symbol name, the codec's arguments between add_id and out); args is emptied of what the codec takes"""
    if cls is PackedLists:
        bits = args.pop("bits", None)
        return "vidc_packed_merge_dev", (0 if bits is None else int(bits),)
    if cls is EfLists:
        return "vidc_ef_merge_dev", (_lib.VIDC_EF_WANT_PERM if args.pop("want_perm", False) else 0,)
    if cls is WaveletTreeLists:
        return "vidc_wt_merge_dev", ()
    return "vidc_roc_merge_dev", (int(args.pop("precision_mode", VIDC_PREC_REFERENCE)),
                                  _lib.VIDC_ROC_WANT_PERM if args.pop("want_perm", False) else 0)


def merge(a, b, add_id=0, *, src=None, **codec_args):
    """-> the merged object (of a's list class -- the base class for a subclass such as a segmented container's inner object --, on
    a's context; it owns its handle).

    a, b: two PackedLists, EfLists, WaveletTreeLists or RocLists of the same class and list count (a is b is allowed).  add_id is
    added to every id of b on the way (Faiss passes the number of vectors of the index merged into).  src (optional): a contiguous
    int64 CUDA tensor with a.ntotal + b.ntotal entries; every entry is written -- p >= 0 where position q of the new object's
    decode_all order holds position p of a's, ~p where it holds position p of b's.  codec_args, as the classes' own append takes them:
    bits (packed bits; None keeps a's width), want_perm (Elias-Fano, ROC), precision_mode (ROC: the mode both objects were built
    with).  Runs on torch's current stream; the call synchronises."""
    ca, cb = _class_of(a), _class_of(b)
    if ca is None or cb is None:
        bad = a if ca is None else b
        raise VidcError(f"merge: {type(bad).__name__} holds no lists to merge (packed bits, Elias-Fano, ROC and wavelet-tree lists do; "
                        "segmented, sharded and graph objects are out of scope)")
    if ca is not cb:
        raise VidcError(f"merge: {type(a).__name__} and {type(b).__name__} are different classes (re-encode one of them)")
    args = dict(codec_args)
    name, extra = _codec_call(ca, args)
    if args:
        raise TypeError(f"merge: {ca.__name__} takes no argument {sorted(args)[0]!r}")
    add_id = int(add_id)
    if add_id < 0 or add_id >> 64:
        raise ValueError("add_id must be in [0, 2^64)")
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: merge needs an MI355X (there is no CPU fallback)")
    if src is not None:
        n = a.ntotal + b.ntotal
        if not _is_cuda(src) or src.dtype != torch.int64 or not src.is_contiguous() or src.numel() != n:
            raise ValueError("src must be a contiguous int64 CUDA tensor with a.ntotal + b.ntotal entries")
    _on_torch_stream(a.ctx)
    h = C.c_void_p()
    try:
        check(getattr(lib(), name)(a.ctx.h, a.h, b.h, add_id, *extra, C.byref(h), ptr(src) if src is not None and src.numel() else None))
    except VidcError as e:
        raise VidcError(f"merge: {ca.__name__}: {e}") from None
    return ca(h, a.ctx, None, _nlist(a), None)  # (the matched list class: a subclass may own nothing, or construct differently)
