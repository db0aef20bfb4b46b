"""The numpy statement of one vidc_ivf_kmeans_step_dev call (include/vidc.h).  Assignment: the float64 argmin of the squared distance
with first-index ties.  Update: float32, members in ascending point order, sequential partial sums over chunks of 256 members, the
partials added in chunk order, one float32 division by the count; an empty cluster keeps c_in."""
import numpy as np

KM_CHUNK = 256


def distances(x, c):
    """x [n, ld], c [G, k, dsub] -> float64 squared distances [G, n, k] (exact on small integer grids)"""
    G, k, dsub = c.shape
    out = np.empty((G, len(x), k))
    for g in range(G):
        xg, cg = x[:, g * dsub:(g + 1) * dsub].astype(np.float64), c[g].astype(np.float64)
        out[g] = (xg ** 2).sum(1)[:, None] - 2.0 * (xg @ cg.T) + (cg ** 2).sum(1)[None]
    return out


def assign(x, c):
    return distances(x, c).argmin(2).astype(np.int32)


def chunk_sum(rows):
    """float32 [m, dsub] in member order -> the cluster sum of the chunk rule"""
    total = np.zeros(rows.shape[1], np.float32)
    for at in range(0, len(rows), KM_CHUNK):
        part = np.zeros(rows.shape[1], np.float32)
        for row in rows[at:at + KM_CHUNK]:
            part = part + row
        total = total + part
    return total


def update(x, c, a):
    """-> (c_out float32 [G, k, dsub], counts uint32 [G, k]) for the assignment a [G, n]"""
    G, k, dsub = c.shape
    out, counts = c.copy(), np.zeros((G, k), np.uint32)
    for g in range(G):
        xg = np.ascontiguousarray(x[:, g * dsub:(g + 1) * dsub], np.float32)
        order = np.argsort(a[g], kind="stable")
        bounds = np.searchsorted(a[g][order], np.arange(k + 1))
        for j in range(k):
            m = bounds[j + 1] - bounds[j]
            counts[g, j] = m
            if m:
                out[g, j] = chunk_sum(xg[order[bounds[j]:bounds[j + 1]]]) / np.float32(m)
    return out, counts


def step(x, c):
    a = assign(x, c)
    return update(x, c, a) + (a,)
