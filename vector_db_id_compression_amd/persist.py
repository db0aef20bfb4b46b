"""Flat images of the compressed objects: `save(obj, path)` writes one .npz per object, `load(path)` brings it back without re-encoding.

A wavelet tree (both wt_types) and compact graph rows are stored as the arrays of vidc_wt_export_all / vidc_compact_export_all plus
their geometry and a `kind` entry; the derived tables of a tree (rank directory, samples, node ranks) are not stored: vidc_wt_import
rebuilds them on the GPU and checks the image before any query kernel walks it (include/vidc.h).  RocLists, EfLists and PackedLists
keep their own save / load and file layout; `load` recognises their files by their keys.  RocSegLists writes kind "rocseg": its inner
object's ROC export plus the segment map, loaded through vidc_rocseg_wrap, which checks the map.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .codecs import CompactRows, EfLists, PackedLists, RocLists, RocSegLists, WaveletTreeLists, _as_offsets


def _npz_path(path):
    """the file np.savez(path) writes"""
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


def wt_image(w):
    """-> dict(offsets, wt_type, bits, cls, offs, off_bits): the image arrays of a WaveletTreeLists (vidc_wt_export_all)"""
    nb, nc, no = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().vidc_wt_image_words(w.h, C.byref(nb), C.byref(nc), C.byref(no)))
    bits = np.zeros(nb.value, np.uint64)
    cls = np.zeros(nc.value, np.uint32)
    offs = np.zeros(no.value, np.uint64)
    off_bits = np.zeros(w.levels, np.uint64)
    check(lib().vidc_wt_export_all(w.ctx.h, w.h, ptr(bits) if bits.size else None, bits.size, ptr(cls) if cls.size else None, cls.size,
                                   ptr(offs) if offs.size else None, offs.size, ptr(off_bits)))
    return dict(offsets=np.array(w.offsets, dtype=np.uint64), wt_type=int(lib().vidc_wt_type(w.h)), bits=bits, cls=cls, offs=offs,
                off_bits=off_bits)


def wt_from_image(offsets, wt_type, bits, cls, offs, off_bits, ctx=None):
    """vidc_wt_import -> WaveletTreeLists; VidcError (VIDC_ERR_INVALID) for an image the query kernels could not walk in bounds"""
    ctx = _lib.default_context() if ctx is None else ctx
    off = _as_offsets(offsets)
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    cls = np.ascontiguousarray(cls, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    off_bits = np.ascontiguousarray(off_bits, dtype=np.uint64)
    h = C.c_void_p()
    check(lib().vidc_wt_import(ctx.h, off.size - 1, ptr(off), int(wt_type), ptr(bits) if bits.size else None, bits.size,
                               ptr(cls) if cls.size else None, cls.size, ptr(offs) if offs.size else None, offs.size,
                               ptr(off_bits) if off_bits.size else None, C.byref(h)))
    return WaveletTreeLists(h, ctx, off)


def compact_image(c):
    """-> uint8 [N, stride]: the row bytes of a CompactRows (vidc_compact_export_all)"""
    buf = np.zeros((c.N, c.stride), np.uint8)
    check(lib().vidc_compact_export_all(c.ctx.h, c.h, ptr(buf) if buf.size else None, buf.size))
    return buf


def compact_from_image(N, K, data, ctx=None):
    """vidc_compact_import -> CompactRows; VidcError for a row that would decode an id above N"""
    ctx = _lib.default_context() if ctx is None else ctx
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    h = C.c_void_p()
    check(lib().vidc_compact_import(ctx.h, int(N), int(K), ptr(data) if data.size else None, data.size, C.byref(h)))
    return CompactRows(h, ctx, int(N), int(K))


def save(obj, path):
    """One .npz per object -> the path of the file written."""
    if isinstance(obj, WaveletTreeLists):
        im = wt_image(obj)
        np.savez(path, kind=np.array("wt"), wt_type=np.int64(im["wt_type"]), offsets=im["offsets"], wt_bits=im["bits"], cls=im["cls"],
                 offs=im["offs"], off_bits=im["off_bits"])
    elif isinstance(obj, CompactRows):
        np.savez(path, kind=np.array("compact"), N=np.int64(obj.N), K=np.int64(obj.K), data=compact_image(obj))
    elif isinstance(obj, (RocLists, RocSegLists, EfLists, PackedLists)):
        obj.save(path)
    else:
        raise TypeError(f"persist.save: {type(obj).__name__} has no image")
    return _npz_path(path)


def load(path, ctx=None):
    """The object of a file written by `save` (or by the save method of RocLists / EfLists / PackedLists)."""
    with np.load(path) as z:
        keys = set(z.files)
        if "kind" in keys:
            kind = str(z["kind"])
            if kind == "wt":
                return wt_from_image(z["offsets"], int(z["wt_type"]), z["wt_bits"], z["cls"], z["offs"], z["off_bits"], ctx)
            if kind == "compact":
                return compact_from_image(int(z["N"]), int(z["K"]), z["data"], ctx)
            if kind == "rocseg":
                return RocSegLists.load(path, ctx)
            raise ValueError(f"{path}: unknown image kind {kind!r}")
    if "heads" in keys:
        return RocLists.load(path, ctx)
    if "low" in keys:
        return EfLists.load(path, ctx)
    if "bits" in keys and "words" in keys:
        return PackedLists.load(path, ctx)
    raise ValueError(f"{path}: not an image of a vector_db_id_compression_amd object (keys {sorted(keys)})")
