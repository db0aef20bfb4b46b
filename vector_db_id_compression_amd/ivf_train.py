"""k-means training of an IVFIndex on the device (vidc_ivf_kmeans_step_dev): one Lloyd iteration per call, batched over independent
groups of columns, with a deterministic result -- the step IVFIndex.train does otherwise with torch.cdist, index_add_ and bincount.

    c_new, assign, counts = ivf_train.kmeans_step_device(x, c, groups=1)   # c [G, k, dsub] (or [k, d] for one group)
    centroids = ivf_train.kmeans_device(x, k, iters=10, seed=123)          # [k, d]; the initial rows of ivf._kmeans
    pq = ivf_train.pq_train_device(x, M, iters=10, ksub=256)               # [M, ksub, d / M]; all sub-quantisers advance together

IVFIndex.train_device = True makes train take its centroids and its codebooks from here.  An objective value, splitting of empty
clusters, k-means++ and inner product are out of scope.
"""
import numpy as np

from ._lib import VidcError, check, default_context, lib, ptr


def _torch():
    import torch

    return torch


def _f32(a):
    torch = _torch()
    if not (isinstance(a, torch.Tensor) and a.is_cuda):
        a = torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()
    return a.to(torch.float32).contiguous()


def kmeans_step_device(x, c, groups=1):
    """x [n, ld], c [G, k, dsub] with G * dsub <= ld (or [k, dsub] when groups == 1) -> (c_new like c, assign int32 [G, n],
    counts int32 [G, k]) as CUDA tensors; with a 2-D c, assign is [n] and counts [k].  Runs on torch's current stream."""
    torch = _torch()
    if not torch.cuda.is_available():
        raise VidcError("no HIP device: kmeans_step_device needs an MI355X (there is no CPU fallback)")
    x, c = _f32(x), _f32(c)
    flat = c.dim() == 2
    if flat:
        if groups != 1:
            raise ValueError("a 2-D c is one group")
        c = c[None]
    if x.dim() != 2 or c.dim() != 3 or c.shape[0] != groups:
        raise ValueError("x must be [n, ld] and c [groups, k, dsub]")
    n, ld = int(x.shape[0]), int(x.shape[1])
    G, k, dsub = (int(s) for s in c.shape)
    c_new = torch.empty_like(c)
    assign = torch.empty((G, n), dtype=torch.int32, device=x.device)
    counts = torch.empty((G, k), dtype=torch.int32, device=x.device)  # (the bytes of the call's uint32)
    ctx = default_context()
    check(lib().vidc_ivf_kmeans_step_dev(ctx.h, n, ptr(x) if n else None, ld, G, dsub, k, ptr(c), ptr(c_new), ptr(assign) if n else None,
                                         ptr(counts)))
    if flat:
        return c_new[0], assign[0], counts[0]
    return c_new, assign, counts


def _initial_rows(x, k, seed):
    """the rows ivf._kmeans starts from: the same randperm seed, the same padding rule for n < k"""
    torch = _torch()
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    c = x[torch.randperm(x.shape[0], generator=g)[:k].to(x.device)].clone()
    if c.shape[0] < k:
        reps = (k + c.shape[0] - 1) // c.shape[0]
        c = c.repeat(reps, 1)[:k] + 1e-3 * torch.arange(k, device=x.device, dtype=x.dtype)[:, None]
    return c


def kmeans_device(x, k, iters=10, seed=123):
    """x [n, d] -> centroids [k, d] after `iters` device iterations from ivf._kmeans's initial rows"""
    x = _f32(x)
    c = _initial_rows(x, k, seed)
    for _ in range(iters):
        c = kmeans_step_device(x, c)[0]
    return c


def pq_train_device(x, M, iters=10, ksub=256):
    """x [n, d], d a multiple of M -> codebooks [M, ksub, d / M]: sub-quantiser m starts from seed 7 + m, one step call per iteration
    advances all M"""
    torch = _torch()
    x = _f32(x)
    d = int(x.shape[1])
    if M < 1 or d % M:
        raise ValueError("d must be a multiple of M")
    dsub = d // M
    pq = torch.stack([_initial_rows(x[:, m * dsub:(m + 1) * dsub], ksub, 7 + m) for m in range(M)]).contiguous()
    for _ in range(iters):
        pq = kmeans_step_device(x, pq, groups=M)[0]
    return pq
