"""The coarse quantiser of an IVFIndex on the device (vidc_ivf_probe_dev): the nprobe nearest centroids of every query, in
ascending (squared L2 distance, list number) order, from float32 MFMA kernels -- the step torch.cdist + topk does otherwise.

    probes, cdist = ivf_probe.probe_device(index, xq)          # int64 [nq, nprobe], float32 [nq, nprobe]
    assign = ivf_probe.assign_device(index, x)                 # int64 [n]: the nprobe = 1 form

IVFIndex.coarse_device = True makes scan_device / search_device, ivf_range.range_scan_device / range_search_device and add take
their probe rows and list assignments from here (nprobe <= 256; above it they stay with torch).  Inner product, nprobe > 256 and
the PQ encoder's assignment are out of scope.
"""
import numpy as np

from ._lib import VidcError, check, default_context, lib, ptr

MAX_NPROBE = 256  # the pool limit of the kernels (ivs::MAX_K)


def _torch():
    import torch

    return torch


def probe_device(index, xq, nprobe=None):
    """-> (probes int64 [nq, nprobe], cdist float32 [nq, nprobe]) as CUDA tensors, -1 / +inf padded where nprobe > nlist.  nprobe
    defaults to min(index.nprobe, index.nlist).  Runs on torch's current stream."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: probe_device needs an MI355X (there is no CPU fallback)")
    if not (isinstance(xq, torch.Tensor) and xq.is_cuda):
        xq = torch.from_numpy(np.array(xq, dtype=np.float32, order="C")).cuda()
    xq = xq.to(torch.float32).contiguous()
    if xq.dim() != 2 or xq.shape[1] != index.d:
        raise ValueError(f"xq must be [nq, {index.d}]")
    nprobe = min(index.nprobe, index.nlist) if nprobe is None else int(nprobe)
    if not 0 <= nprobe < 2 ** 32:
        raise ValueError("nprobe is an unsigned 32-bit number")
    cent = index.centroids.to(torch.float32).contiguous()
    nq = int(xq.shape[0])
    probes = torch.empty((nq, nprobe), dtype=torch.int64, device=xq.device)
    cdist = torch.empty((nq, nprobe), dtype=torch.float32, device=xq.device)
    ctx = default_context()
    check(lib().vidc_ivf_probe_dev(ctx.h, index.nlist, ptr(cent), index.d, nq, ptr(xq) if nq else None, nprobe,
                                   ptr(probes) if probes.numel() else None, ptr(cdist) if cdist.numel() else None))
    return probes, cdist


def assign_device(index, x):
    """-> int64 [n]: the list of every vector, the nearest centroid (of equal distances the smaller list number)"""
    return probe_device(index, x, 1)[0].reshape(-1)
