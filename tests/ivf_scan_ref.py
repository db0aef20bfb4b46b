"""The numpy model of the IVF list scan on the device (vidc_ivf_scan_dev, csrc/ivf_scan_ref.h) and the shapes the CPU and GPU tests share.

Per query: the candidates are all entries of the distinct valid lists its probe row names; the result is the first k in ascending
(distance, label) order, label = list_no << 32 | offset, padded with +inf / -1; stats = (lists scanned, codes scanned).

Test data are integer grids: coordinates (and PQ codebook entries) are integers in [-R, R] stored as float32 with d * (2R)^2 < 2^24, so
every squared distance is an exact float32 integer in any summation order and D, labels and stats are compared element for element.
"""
import functools

import numpy as np

R_EDGES = 3
EDGE_SIZES = (0, 1, 63, 64, 65, 129, 300, 7)  # list sizes around the 64-code trip, one above 256, an empty list in front
FLAT, PQ8 = 0, 1


def l2(vecs, q):
    return ((q[None, :].astype(np.float32) - vecs.astype(np.float32)) ** 2).sum(1, dtype=np.float32)


def valid_lists(row, nlist, lo=0, hi=None):
    """the lists a probe row names, first mention first, each once; with (lo, hi) the piece row[lo:hi] of a row that was
    de-duplicated as a whole"""
    seen, out = set(), []
    for j, p in enumerate(row):
        p = int(p)
        if 0 <= p < nlist and p not in seen:
            seen.add(p)
            if lo <= j < (len(row) if hi is None else hi):
                out.append(p)
    return out


def model(offsets, vecs, xq, probes, k, S=1):
    """-> D float32 [nq, k], labels int64 [nq, k], stats uint32 [nq, 2].  vecs: the decoded vectors float32 [ntotal, d] in the
    container's order.  S > 1: every piece of the probe row keeps its own k best and the pieces are merged -- the same result."""
    off = np.asarray(offsets).astype(np.int64)
    nlist, ntotal = off.size - 1, vecs.shape[0]
    xq = np.asarray(xq, dtype=np.float32)
    probes = np.asarray(probes, dtype=np.int64)
    nq, nprobe = probes.shape
    D = np.full((nq, k), np.inf, dtype=np.float32)
    L = np.full((nq, k), -1, dtype=np.int64)
    stats = np.zeros((nq, 2), dtype=np.uint32)
    for q in range(nq):
        best = []  # (distance, position) of the pieces' survivors
        for s in range(S):
            cand = []
            for l in valid_lists(probes[q], nlist, s * nprobe // S, (s + 1) * nprobe // S):
                b = min(int(off[l + 1]), ntotal)
                a = min(int(off[l]), b)
                stats[q] += np.array((1, b - a), dtype=np.uint32)
                if b > a:
                    dist = l2(vecs[a:b], xq[q])
                    cand += list(zip(dist.tolist(), range(a, b)))
            cand.sort()
            best += cand[:k]
        best.sort()
        for i, (dist, pos) in enumerate(best[:k]):
            l = int(np.searchsorted(off, pos, side="right")) - 1
            D[q, i] = dist
            L[q, i] = (l << 32) | (pos - int(off[l]))
    return D, L, stats


def brute_force(offsets, vecs, xq, probes, k):
    """the statement again as a double loop over (list, offset), written from include/vidc.h: no positions, no pieces"""
    off = [int(v) for v in offsets]
    nlist = len(off) - 1
    D = np.full((len(xq), k), np.inf, dtype=np.float32)
    L = np.full((len(xq), k), -1, dtype=np.int64)
    stats = np.zeros((len(xq), 2), dtype=np.uint32)
    for q in range(len(xq)):
        lists = sorted({int(p) for p in probes[q] if 0 <= int(p) < nlist})
        found = []
        for l in lists:
            for o in range(off[l + 1] - off[l]):
                v = vecs[off[l] + o]
                dist = np.float32(0)
                for i in range(v.size):
                    t = np.float32(xq[q][i]) - np.float32(v[i])
                    dist = np.float32(dist + t * t)
                found.append((float(dist), (l << 32) | o))
        found.sort()
        for i, (dist, label) in enumerate(found[:k]):
            D[q, i], L[q, i] = dist, label
        stats[q] = (len(lists), sum(off[l + 1] - off[l] for l in lists))
    return D, L, stats


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def obj(d, M=0, sizes=EDGE_SIZES, R=R_EDGES, seed=3):
    """lists of the given sizes over random grid vectors.  M == 0: FLAT (codes = the float32 bytes); else PQ8 with integer codebooks
    [M, 256, d / M] and random code bytes.  -> dict(offsets uint64, ntotal, nlist, codes uint8 [ntotal, code_size], vecs, codebooks)"""
    assert d * (2 * R) ** 2 < 2 ** 24
    rng = np.random.default_rng(seed + 1000 * d + M)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ntotal = int(off[-1])
    if M:
        dsub = d // M
        assert dsub * M == d
        cb = rng.integers(-R, R + 1, size=(M, 256, dsub)).astype(np.float32)
        codes = rng.integers(0, 256, size=(ntotal, M), dtype=np.uint8)
        vecs = np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1).astype(np.float32)
    else:
        cb = None
        vecs = rng.integers(-R, R + 1, size=(ntotal, d)).astype(np.float32)
        codes = np.ascontiguousarray(vecs).view(np.uint8).reshape(ntotal, 4 * d).copy()
    return _freeze(dict(offsets=off, ntotal=ntotal, nlist=len(sizes), codes=codes, vecs=vecs, codebooks=cb, d=d, M=M, R=R,
                        kind=PQ8 if M else FLAT))


@functools.lru_cache(maxsize=None)
def queries(d, nq, R=R_EDGES, seed=9):
    xq = np.random.default_rng(seed + d).integers(-R, R + 1, size=(nq, d)).astype(np.float32)
    xq.setflags(write=False)
    return xq


# the probe rows of the designed object (8 lists: EDGE_SIZES), 4 wide.  Against k = 64: list 2 holds fewer than k entries, list 3
# exactly k, list 4 k + 1.
EDGE_ROWS = np.array([
    [2, -1, -1, -1], [3, -1, -1, -1], [4, -1, -1, -1], [0, -1, -1, -1],  # one list: 63, 64, 65 and 0 entries
    [-1, 8, 2 ** 40, -1],                                                 # only invalid probes: -1, nlist, 2^40
    [5, 5, 6, -1], [6, 1, 6, 6],                                          # a list named two and three times
    [0, 1, 2, 3], [7, 6, 5, 4], [1, -1, 5, 2 ** 40], [3, 3, 3, 3], [8, 7, -5, 0],
], dtype=np.int64)
EDGE_ROWS.setflags(write=False)


@functools.lru_cache(maxsize=None)
def probe_rows(nq, nprobe, nlist=len(EDGE_SIZES), seed=21):
    """random rows over [-1, nlist]: -1 and nlist are invalid, and a row wider than the lists names lists again and again"""
    p = np.random.default_rng(seed + nprobe).integers(-1, nlist + 1, size=(nq, nprobe)).astype(np.int64)
    p.setflags(write=False)
    return p


# name: d, R, vectors, lists, nprobe, k, queries
SHAPES = {"distinct": (16, 30, 2000, 16, 4, 10, 64), "ties": (4, 2, 2000, 16, 4, 10, 64)}


@functools.lru_cache(maxsize=None)
def shape(name):
    """-> dict(x [n, d] in add order, assign [n], centroids [nlist, d], xq, and the FLAT lists built from them: offsets, vecs, codes,
    probes = distinct lists per query, nearest centroid first)"""
    d, R, n, nlist, nprobe, k, nq = SHAPES[name]
    assert d * (2 * R) ** 2 < 2 ** 24
    rng = np.random.default_rng(41)
    x = rng.integers(-R, R + 1, size=(n, d)).astype(np.float32)
    xq = rng.integers(-R, R + 1, size=(nq, d)).astype(np.float32)
    centroids = rng.integers(-R, R + 1, size=(nlist, d)).astype(np.float32)
    assign = np.array([int(np.argmin(l2(centroids, v))) for v in x])
    order = np.argsort(assign, kind="stable")
    off = np.searchsorted(assign[order], np.arange(nlist + 1)).astype(np.uint64)
    vecs = x[order]
    probes = np.stack([np.argsort(l2(centroids, v), kind="stable")[:nprobe] for v in xq]).astype(np.int64)
    codes = np.ascontiguousarray(vecs).view(np.uint8).reshape(n, 4 * d).copy()
    return _freeze(dict(x=x, xq=xq, centroids=centroids, assign=assign, offsets=off, vecs=vecs, codes=codes, probes=probes, ids=order,
                        d=d, R=R, nlist=nlist, nprobe=nprobe, k=k, nq=nq, ntotal=n, M=0, kind=FLAT, codebooks=None))


@functools.lru_cache(maxsize=None)
def expected(name, k=None):
    s = shape(name)
    out = model(s["offsets"], s["vecs"], s["xq"], s["probes"], k or s["k"])
    for a in out:
        a.setflags(write=False)
    return out


def tie_free(offsets, vecs, xq, probes, k):
    """per query: no two of its k + 1 best candidates share a distance (torch.topk and the kernel then agree on the labels)"""
    D = model(offsets, vecs, xq, probes, k + 1)[0]
    return np.array([np.unique(row[np.isfinite(row)]).size == np.isfinite(row).sum() for row in D])


def cases_text(cases):
    """cases: [(obj dict, xq, probes, k)] -> the text tests/ivf_scan_test.cpp reads, the model's answers included"""
    def floats(a):
        return " ".join("inf" if np.isinf(v) else repr(float(v)) for v in np.asarray(a, dtype=np.float32).reshape(-1))

    lines = [str(len(cases))]
    for o, xq, probes, k in cases:
        D, L, st = model(o["offsets"], o["vecs"], xq, probes, k)
        lines.append(f"{o['nlist']} {o['ntotal']} {o['kind']} {o['d']} {o['M']} {xq.shape[0]} {probes.shape[1]} {k}")
        lines.append(" ".join(map(str, np.asarray(o["offsets"]).tolist())))
        lines.append(" ".join(map(str, o["codes"].reshape(-1).tolist())))
        lines.append(floats(o["codebooks"]) if o["M"] else "")
        lines.append(floats(xq))
        lines.append(" ".join(map(str, probes.reshape(-1).tolist())))
        lines.append(floats(D))
        lines.append(" ".join(map(str, L.reshape(-1).tolist())))
        lines.append(" ".join(map(str, st.reshape(-1).tolist())))
    return "\n".join(lines) + "\n"


# the plan of csrc/ivf_scan_plan.h, restated (tests/ivf_scan_test.cpp `plan` prints the header's own figures)
def plan_lds(kind, k, nprobe, d, M):
    r16 = lambda b: (b + 15) // 16 * 16
    pools, row, q = 2 * k * 8 + 64 * 8 + 64 * 4, r16(nprobe * 4), r16(d * 4)
    return max(pools, q) + row + M * 256 * 4 if kind == PQ8 else pools + row + q


def plan_resident(num_cu, lds):
    return min(8192, max(num_cu, 1) * max(1, min(32, 160 * 1024 // lds)))


def plan_pieces(nq, nprobe, resident):
    S = 1
    while S < 16 and S * 2 <= nprobe and nq * S < resident:
        S *= 2
    return S


def plan_slot_items(items, nslots, s):
    return (items - 1 - s) // nslots + 1 if s < items else 0
