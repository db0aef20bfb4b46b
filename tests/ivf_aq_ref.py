"""The numpy statement of an additive-quantiser code (RQ<M>x8_Nfloat: include/vidc.h, csrc/ivf_aq_plan.h), in float64, and the
objects the CPU and GPU tests share.

A code row is M + 4 bytes: the stage indices c_0 .. c_{M-1}, then the little-endian float32 norm of the stored vector.  Codebooks are
[M, 256, d].  distance = max-by-compare(qn + n - 2 (cq + sum_m <xq, cb[m][c_m]>), +0), cq = <xq, centroid> (0 for raw codes).
"""
import functools

import numpy as np

import ivf_scan_ref as ir

FORMS = ((4, 1), (16, 8), (10, 3), (7, 5))  # (d, M): code_size % 4 = 1, 0, 3, 1


def pack(idx, norm):
    """idx integer [n, M], norm float [n] -> uint8 [n, M + 4]"""
    n4 = np.ascontiguousarray(norm, dtype="<f4").view(np.uint8).reshape(-1, 4)
    return np.concatenate([np.asarray(idx).astype(np.uint8), n4], 1)


def unpack(codes, M):
    """uint8 [n, M + 4] -> (idx int64 [n, M], norm float32 [n])"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return codes[:, :M].astype(np.int64), codes[:, M:M + 4].copy().view("<f4")[:, 0]


def decode(codes, cb):
    idx, _ = unpack(codes, cb.shape[0])
    return sum(cb[m][idx[:, m]].astype(np.float64) for m in range(cb.shape[0]))


def distances(codes, cb, xq, cent=None, magnitude=False):
    """float64 [nq, n]: the distance of every row for every query; cent: None, or the centroid of every ROW, [n, d].  magnitude:
    the same sum over absolute values, qn + |n| + 2 (sum |xq_i cent_i| + sum_m sum |xq_i cb_i|): what a rounding bound scales with"""
    idx, norm = unpack(codes, cb.shape[0])
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if magnitude else (lambda a: np.asarray(a, np.float64))
    x = f(xq)
    ip = sum((x @ f(cb[m]).T)[:, idx[:, m]] for m in range(cb.shape[0]))
    if cent is not None:
        ip = ip + x @ f(cent).T
    v = (x * x).sum(1)[:, None] + f(norm)[None, :] + (2 if magnitude else -2) * ip
    return np.where(v > 0, v, 0.0)


def model(offsets, dist, probes, k, dtype=np.float32):
    """ivf_scan_ref.model's selection over given distances [nq, ntotal] -> D [nq, k], labels, stats"""
    off = np.asarray(offsets).astype(np.int64)
    nq, nlist, ntotal = len(probes), off.size - 1, dist.shape[1]
    D, L = np.full((nq, k), np.inf, dtype=dtype), np.full((nq, k), -1, dtype=np.int64)
    stats = np.zeros((nq, 2), dtype=np.uint32)
    for q in range(nq):
        cand = []
        for l in ir.valid_lists(probes[q], nlist):
            b = min(int(off[l + 1]), ntotal)
            a = min(int(off[l]), b)
            stats[q] += np.array((1, b - a), dtype=np.uint32)
            cand += list(zip(dist[q, a:b].astype(dtype).tolist(), range(a, b)))
        for i, (dv, pos) in enumerate(sorted(cand)[:k]):
            l = int(np.searchsorted(off, pos, side="right")) - 1
            D[q, i], L[q, i] = dv, (l << 32) | (pos - int(off[l]))
    return D, L, stats


@functools.lru_cache(maxsize=None)
def obj(d, M, res, sizes=ir.EDGE_SIZES, R=ir.R_EDGES, seed=5):
    """random indices, integer codebooks [M, 256, d] and centroids; the stored norm is the exact |decoded (+ centroid)|^2.  Every
    intermediate (a table entry <= d R^2, their sum, the norm <= d ((M + 1) R)^2) is an integer below 2^24: float32 is exact."""
    assert 4 * d * ((M + 2) * R) ** 2 < 2 ** 24
    rng = np.random.default_rng(seed + 1000 * d + M)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ntotal = int(off[-1])
    cb = rng.integers(-R, R + 1, size=(M, 256, d)).astype(np.float32)
    cent = rng.integers(-R, R + 1, size=(len(sizes), d)).astype(np.float32)
    idx = rng.integers(0, 256, size=(ntotal, M))
    rowc = cent[np.repeat(np.arange(len(sizes)), sizes)]
    vecs = sum(cb[m][idx[:, m]] for m in range(M)) + (rowc if res else 0)
    codes = pack(idx, (vecs.astype(np.float64) ** 2).sum(1))
    return ir._freeze(dict(offsets=off, ntotal=ntotal, nlist=len(sizes), codes=codes, vecs=vecs.astype(np.float32), codebooks=cb, centroids=cent,
                           rowc=rowc if res else None, d=d, M=M, res=res))
