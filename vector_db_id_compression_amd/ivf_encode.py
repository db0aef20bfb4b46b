"""The PQ encoder of an IVFIndex on the device (vidc_ivf_pq_encode_dev): the 8-bit codes of a vector batch from a float32 MFMA
kernel -- the step IVFIndex._encode_dev does otherwise with M calls of torch.cdist(...).argmin(1).

    codes = ivf_encode.pq_encode_device(x, pq)                       # uint8 [n, M], raw PQ
    codes = ivf_encode.pq_encode_device(x, pq, centroids, assign)    # the codes of x - centroids[assign]
    codes = ivf_encode.encode_device(index, x, assign)               # over an IVFIndex (raw or by_residual)
    codes = ivf_encode.pq_encode_bits_device(x, pq, nbits)           # uint8 [n, ceil(M * nbits / 8)], packed (vidc_ivf_pq_encode_bits_dev)

IVFIndex.pq_device = True makes add (and everything else that goes through _encode_dev) take its codes from here while
d / M <= 128; above it Python stays with torch.  ("PQ", M, nbits) codes always come from pq_encode_bits_device: packed codes have
no torch encoder.  Inner product is out of scope; the codebooks themselves come from ivf_train.py.
"""
import numpy as np

from ._lib import VidcError, check, default_context, lib, ptr

MAX_DSUB = 128  # the codebook of one sub-quantiser is held in LDS (ipe::MAX_DSUB)


def _torch():
    import torch

    return torch


def _f32(a):
    torch = _torch()
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        a = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()
    return a.to(torch.float32).contiguous()


def pq_encode_device(x, pq, centroids=None, assign=None):
    """x [n, d], pq [M, 256, d / M], optionally centroids [nlist, d] and assign int64 [n] -> uint8 CUDA tensor [n, M]; a row whose
    assign is outside [0, nlist) gets zero bytes.  Runs on torch's current stream."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: pq_encode_device needs an MI355X (there is no CPU fallback)")
    x, pq = _f32(x), _f32(pq)
    if x.dim() != 2 or pq.dim() != 3 or pq.shape[1] != 256 or pq.shape[0] * pq.shape[2] != x.shape[1]:
        raise ValueError("x must be [n, d] and pq [M, 256, d / M]")
    n, d, M = int(x.shape[0]), int(x.shape[1]), int(pq.shape[0])
    nlist = 0
    if centroids is not None:
        centroids = _f32(centroids)
        if centroids.dim() != 2 or centroids.shape[1] != d or assign is None:
            raise ValueError("centroids must be [nlist, d] and come with assign")
        assign = torch.as_tensor(assign).to(device=x.device, dtype=torch.int64).contiguous()
        if assign.shape != (n,):
            raise ValueError("assign must be [n]")
        nlist = int(centroids.shape[0])
    codes = torch.empty((n, M), dtype=torch.uint8, device=x.device)
    ctx = default_context()
    res = centroids is not None and n > 0  # (an empty batch has no assign array to point at)
    check(lib().vidc_ivf_pq_encode_dev(ctx.h, n, ptr(x) if n else None, d, M, ptr(pq), nlist, ptr(centroids) if res else None,
                                       ptr(assign) if res else None, ptr(codes) if n else None))
    return codes


def pq_encode_bits_device(x, pq, nbits, centroids=None, assign=None):
    """x [n, d], pq [M, 2^nbits, d / M], optionally centroids [nlist, d] and assign int64 [n] -> uint8 CUDA tensor
    [n, ceil(M * nbits / 8)] in the packed layout of include/vidc.h; a row whose assign is outside [0, nlist) gets zero bytes."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: pq_encode_bits_device needs an MI355X (there is no CPU fallback)")
    x, pq, nbits = _f32(x), _f32(pq), int(nbits)
    if x.dim() != 2 or pq.dim() != 3 or pq.shape[1] != 1 << nbits or pq.shape[0] * pq.shape[2] != x.shape[1]:
        raise ValueError("x must be [n, d] and pq [M, 2^nbits, d / M]")
    n, d, M = int(x.shape[0]), int(x.shape[1]), int(pq.shape[0])
    nlist = 0
    if centroids is not None:
        centroids = _f32(centroids)
        if centroids.dim() != 2 or centroids.shape[1] != d or assign is None:
            raise ValueError("centroids must be [nlist, d] and come with assign")
        assign = torch.as_tensor(assign).to(device=x.device, dtype=torch.int64).contiguous()
        if assign.shape != (n,):
            raise ValueError("assign must be [n]")
        nlist = int(centroids.shape[0])
    codes = torch.empty((n, (M * nbits + 7) // 8), dtype=torch.uint8, device=x.device)
    ctx = default_context()
    res = centroids is not None and n > 0  # (an empty batch has no assign array to point at)
    check(lib().vidc_ivf_pq_encode_bits_dev(ctx.h, n, ptr(x) if n else None, d, M, nbits, ptr(pq), nlist, ptr(centroids) if res else None,
                                            ptr(assign) if res else None, ptr(codes) if n else None))
    return codes


def encode_device(index, x, assign=None):
    """the codes IVFIndex._encode_dev gives for ("PQ", M) codes, from the kernel: raw, or of x - centroids[assign] when the index
    is by_residual"""
    if not index.M:
        raise ValueError("encode_device needs (\"PQ\", M) codes")
    if getattr(index, "packed", False):
        if index.by_residual:
            return pq_encode_bits_device(x, index.pq, index.nbits, index.centroids, assign)
        return pq_encode_bits_device(x, index.pq, index.nbits)
    if index.by_residual:
        return pq_encode_device(x, index.pq, index.centroids, assign)
    return pq_encode_device(x, index.pq)
