"""Additive-quantiser codes of an IVFIndex: ("RQ", M), the RQ<M>x8_Nfloat of include/vidc.h -- M stage indices of 8 bits and the
float32 norm of the stored vector, M + 4 bytes a row; codebooks [M, 256, d].

    lut = ivf_aq.lut_device(codebooks, xq)          # float32 [nq, M, 256] = <xq, codeword> (vidc_ivf_aq_lut_dev)
    D, labels = index.scan_device(xq, k)            # -> ivf_aq.scan_device (vidc_ivf_scan_aq_dev)

Training (k-means on the running residual) and encoding (greedy, stage by stage: no beam search) are torch plumbing around the
k-means and argmin calls the index already has; the scan and its table GEMM are the device's.  Range search, inner product, other
norm encodings and stage widths other than 8 bits are out of scope.
"""
import numpy as np

from ._lib import VidcError, check, default_context, lib, ptr

KSUB = 256


def _torch():
    import torch

    return torch


def train(index, xt):
    """xt [n, d] (already x - centroid where the index is by_residual) -> codebooks [M, 256, d]: stage m is the k-means of what
    the stages before it left"""
    from . import ivf, ivf_train

    torch = _torch()
    r, books = xt.clone(), []
    for m in range(index.M):
        cb = ivf_train.kmeans_device(r, KSUB, seed=7 + m) if index.train_device else ivf._kmeans(r, KSUB, seed=7 + m)
        books.append(cb)
        r = r - cb[ivf._assign(r, cb)]
    return torch.stack(books)


def encode(index, x, assign=None):
    """-> uint8 CUDA tensor [n, M + 4]: per stage the argmin over 256 codewords of the running residual, then the float32 norm of
    the reconstruction (centroid included where the index is by_residual)"""
    from . import ivf, ivf_encode

    torch = _torch()
    cb = index.pq
    base = index.centroids[assign] if index.by_residual else torch.zeros_like(x)
    r, y, idx = x - base, base.clone(), []
    for m in range(index.M):
        if index.pq_device and index.d <= ivf_encode.MAX_DSUB:
            j = ivf_encode.pq_encode_device(r, cb[m:m + 1])[:, 0].long()
        else:
            j = ivf._assign(r, cb[m])
        r, y = r - cb[m][j], y + cb[m][j]
        idx.append(j)
    norm = (y * y).sum(1).to(torch.float32).contiguous()
    return torch.cat([torch.stack(idx, 1).to(torch.uint8), norm.view(torch.uint8).reshape(-1, 4)], 1)


def decode(index, codes):
    """rows [n, M + 4] -> the sum of their M codewords, float32 [n, d] (without the centroid; the norm is not used)"""
    torch = _torch()
    out = torch.zeros((codes.shape[0], index.d), dtype=torch.float32, device=codes.device)
    for m in range(index.M):
        out = out + index.pq[m][codes[:, m].long()]
    return out


def lut_device(codebooks, xq):
    """codebooks [M, 256, d], xq [nq, d] -> float32 CUDA tensor [nq, M, 256], entry = <xq, codeword>.  Runs on torch's current
    stream."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: lut_device needs an MI355X (there is no CPU fallback)")
    cb, xq = (torch.as_tensor(np.asarray(a, np.float32) if not hasattr(a, "is_cuda") else a).cuda().to(torch.float32).contiguous()
              for a in (codebooks, xq))
    if cb.dim() != 3 or cb.shape[1] != KSUB or xq.dim() != 2 or xq.shape[1] != cb.shape[2]:
        raise ValueError("codebooks must be [M, 256, d] and xq [nq, d]")
    nq, M, d = int(xq.shape[0]), int(cb.shape[0]), int(cb.shape[2])
    lut = torch.empty((nq, M, KSUB), dtype=torch.float32, device=xq.device)
    check(lib().vidc_ivf_aq_lut_dev(default_context().h, d, M, ptr(cb), nq, ptr(xq) if nq else None, ptr(lut) if nq else None))
    return lut


def scan_device(index, xq, probes, k, off, codes):
    """the tail of IVFIndex.scan_device for ("RQ", M): checked CUDA tensors in, (D, labels) out"""
    torch = _torch()
    nq = int(xq.shape[0])
    D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
    labels = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
    cb = index.pq.to(torch.float32).contiguous()
    cent = index.centroids.to(torch.float32).contiguous() if index.by_residual else None
    from .ivf import NARROW_K

    call = lib().vidc_ivf_scan_aq_wide_dev if k > NARROW_K else lib().vidc_ivf_scan_aq_dev  # (wide: 1 <= k <= 2048)
    check(call(
        default_context().h, index.nlist, ptr(off), int(codes.shape[0]), ptr(codes) if codes.numel() else None, index.d, index.M, ptr(cb),
        ptr(cent) if index.by_residual else None, nq, ptr(xq) if nq else None, int(probes.shape[1]),
        ptr(probes) if probes.numel() else None, k, ptr(D) if D.numel() else None, ptr(labels) if labels.numel() else None, None))
    return D, labels
