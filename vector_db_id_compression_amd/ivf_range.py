"""Range search over an IVFIndex on the device (vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev): IndexIVF::range_search with
deferred id decoding -- every stored vector of the probed lists closer than a radius, the ids decoded only for what passed it.

    lims, D, labels = ivf_range.range_scan_device(index, xq, radius)      # labels = list_no << 32 | offset
    lims, D, I = ivf_range.range_search_device(index, xq, radius)         # ids

Query q's results are D[lims[q]:lims[q + 1]], in probe-row order and then offset order (not sorted by distance, as in Faiss).  A
result is a candidate whose squared L2 distance is strictly below the radius.  Works over the codes of a compressed container and
of ArrayInvertedLists, for "Flat" and ("PQ", M), raw or by_residual (the two *_residual_dev calls).  The only host traffic is the
total (8 bytes) between the two passes: the output is allocated from it.  Per-query radii, inner product and sharded containers are
out of scope.
"""
import ctypes as C

import numpy as np

from ._lib import VIDC_IVF_FLAT, VIDC_IVF_PQ8, VidcError, check, default_context, lib, ptr


def _torch():
    import torch

    return torch


def range_scan_device(index, xq, radius, probes=None):
    """-> (lims int64 [nq + 1], D float32 [total], labels int64 [total]) as CUDA tensors.  probes: an int64 [nq, nprobe] CUDA tensor
    of list numbers, used as it is (-1 = no list, a repeated list counts once); None picks them on the device with the cdist + topk
    of IVFIndex.scan_device.  Runs count, one 8-byte read-back of the total, the allocation, fill, on torch's current stream."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: range_scan_device needs an MI355X (there is no CPU fallback)")
    if not (isinstance(xq, torch.Tensor) and xq.is_cuda):
        xq = torch.from_numpy(np.array(xq, dtype=np.float32, order="C")).cuda()
    xq = xq.to(torch.float32).contiguous()
    if xq.dim() != 2 or xq.shape[1] != index.d:
        raise ValueError(f"xq must be [nq, {index.d}]")
    if probes is None:
        probes = torch.cdist(xq, index.centroids).topk(min(index.nprobe, index.nlist), largest=False).indices
    if not (isinstance(probes, torch.Tensor) and probes.is_cuda and probes.dtype == torch.int64 and probes.dim() == 2
            and probes.shape[0] == xq.shape[0]):
        raise ValueError("probes must be an int64 CUDA tensor [nq, nprobe]")
    probes = probes.contiguous()
    _, codes = index._device_lists()
    off, _ = index._device_offsets()
    nq, nprobe, radius = int(xq.shape[0]), int(probes.shape[1]), float(radius)
    pq = index.pq.to(torch.float32).contiguous() if index.M else None
    ctx = default_context()
    head = (ctx.h, index.nlist, ptr(off), int(codes.shape[0]), ptr(codes) if codes.numel() else None,
            VIDC_IVF_PQ8 if index.M else VIDC_IVF_FLAT, index.d, index.M, ptr(pq) if index.M else None, nq, ptr(xq) if nq else None,
            nprobe, ptr(probes) if probes.numel() else None, radius)
    count, fill = lib().vidc_ivf_range_count_dev, lib().vidc_ivf_range_fill_dev
    if getattr(index, "by_residual", False):  # residual PQ: no code kind, the centroids behind the codebooks
        cent = index.centroids.to(torch.float32).contiguous()
        head = head[:5] + (index.d, index.M, ptr(pq), ptr(cent)) + head[9:]
        count, fill = lib().vidc_ivf_range_count_residual_dev, lib().vidc_ivf_range_fill_residual_dev
    slot_lims = torch.empty(nq * nprobe + 1, dtype=torch.int64, device=xq.device)
    total = C.c_uint64(0)
    check(count(*head, ptr(slot_lims), C.byref(total)))
    n = int(total.value)
    D = torch.empty(n, dtype=torch.float32, device=xq.device)
    labels = torch.empty(n, dtype=torch.int64, device=xq.device)
    check(fill(*head, ptr(slot_lims), n, ptr(D) if n else None, ptr(labels) if n else None))
    return slot_lims[::nprobe].contiguous(), D, labels


def range_search_device(index, xq, radius):
    """range_scan_device, then the labels -> ids on the device (translate_labels of a compressed container, the segmented ROC one
    included; one gather of the ids of plain lists).  -> (lims, D, I) CUDA tensors."""
    torch = _torch()
    lims, D, labels = range_scan_device(index, xq, radius)
    il = index.invlists
    if labels.numel() == 0:
        return lims, D, labels
    if hasattr(il, "translate_labels"):
        return lims, D, il.translate_labels(labels)
    off, ids = index._device_offsets()
    if ids is None:
        raise RuntimeError("range_search_device: the inverted lists cannot translate labels")
    rows = off[labels >> 32] + (labels & 0xFFFFFFFF)
    return lims, D, ids[rows.clamp(max=ids.numel() - 1)]
