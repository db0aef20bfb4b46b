"""The numpy model of the residual-PQ IVF scan and range search on the device (vidc_ivf_scan_residual_dev,
vidc_ivf_range_count_residual_dev / vidc_ivf_range_fill_residual_dev, csrc/ivf_residual_ref.h) and the objects the CPU and GPU tests share.

A code of list l is the 8-bit PQ code of (vector - centroids[l]).  For a query xq, a valid list l and a code of that list:

    r           = xq - centroids[l]                                  one float32 subtraction per component
    entry(m, c) = sum_i (r[m * dsub + i] - codebooks[m][c][i])^2     components in order
    distance    = sum_m entry(m, code[m])                            in m order

and everything else is the scan's and the range search's (tests/ivf_scan_ref.py, tests/ivf_range_ref.py): `model` and `range_model`
call their models on vecs = decode(codes) + centroids[list].

Test data are integer grids: query, centroid and codebook coordinates are integers in [-R, R] stored as float32, so r lies in
[-2R, 2R] and r minus a codebook entry in [-3R, 3R]; with d * (3R)^2 < 2^24 (three terms now) every distance is an exact float32
integer in any summation order and in either form, (xq - c) - decode or xq - (decode + c): all comparisons are element for element.
"""
import functools

import numpy as np

import ivf_range_ref as rr
import ivf_scan_ref as ir

EDGE_ROWS = ir.EDGE_ROWS
FORMS = ((8, 2), (16, 4), (24, 3), (128, 16), (4, 4))  # (d, M)


def decode(codes, codebooks):
    M = codebooks.shape[0]
    return np.concatenate([codebooks[m][codes[:, m]] for m in range(M)], axis=1).astype(np.float32)


def list_of_rows(offsets, ntotal):
    """the list every row of the code array lies in (the label rule: the last l with offsets[l] <= position)"""
    off = np.asarray(offsets).astype(np.int64)
    return np.searchsorted(off, np.arange(ntotal), side="right") - 1


def stored(offsets, codes, codebooks, centroids):
    """what the codes stand for: decode(code) + centroids[list]"""
    return (decode(codes, codebooks) + centroids[list_of_rows(offsets, codes.shape[0])]).astype(np.float32)


def model(offsets, codes, codebooks, centroids, xq, probes, k, S=1):
    """-> D float32 [nq, k], labels int64 [nq, k], stats uint32 [nq, 2]"""
    return ir.model(offsets, stored(offsets, codes, codebooks, centroids), xq, probes, k, S)


def range_model(offsets, codes, codebooks, centroids, xq, probes, radius):
    """-> slot_lims uint64 [nq * nprobe + 1], D float32 [total], labels int64 [total]"""
    return rr.model(offsets, stored(offsets, codes, codebooks, centroids), xq, probes, radius)


def fill_model(offsets, codes, codebooks, centroids, xq, probes, radius, lims, capacity):
    return rr.fill_model(offsets, stored(offsets, codes, codebooks, centroids), xq, probes, radius, lims, capacity)


def candidates(offsets, codes, codebooks, centroids, xq, row):
    """The statement as a double loop over (probe entry, offset), written from include/vidc.h: no positions, no pieces, no decoded
    vectors.  -> [(distance float32, list, offset)] of one query in probe-row order, then offset order, and the lists scanned."""
    off = [int(v) for v in offsets]
    nlist, (M, _, dsub) = len(off) - 1, codebooks.shape
    out, lists = [], []
    for j, p in enumerate(row):
        p = int(p)
        if not (0 <= p < nlist) or any(int(e) == p for e in row[:j]):
            continue
        lists.append(p)
        if off[p + 1] == off[p]:
            continue
        r = (np.asarray(xq, np.float32) - centroids[p].astype(np.float32)).astype(np.float32)
        table = np.zeros((M, 256), np.float32)
        for m in range(M):
            for i in range(dsub):  # components in order, float32 at every step (all 256 entries at once)
                t = (r[m * dsub + i] - codebooks[m][:, i].astype(np.float32)).astype(np.float32)
                table[m] = (table[m] + t * t).astype(np.float32)
        for o in range(off[p + 1] - off[p]):
            dist = np.float32(0)
            for m in range(M):
                dist = np.float32(dist + table[m][codes[off[p] + o][m]])
            out.append((dist, p, o))
    return out, lists


def brute_force(offsets, codes, codebooks, centroids, xq, probes, k):
    off = [int(v) for v in offsets]
    D = np.full((len(xq), k), np.inf, dtype=np.float32)
    L = np.full((len(xq), k), -1, dtype=np.int64)
    stats = np.zeros((len(xq), 2), dtype=np.uint32)
    for q in range(len(xq)):
        cand, lists = candidates(offsets, codes, codebooks, centroids, xq[q], probes[q])
        found = sorted((float(dist), (l << 32) | o) for dist, l, o in cand)
        for i, (dist, label) in enumerate(found[:k]):
            D[q, i], L[q, i] = dist, label
        stats[q] = (len(lists), sum(off[l + 1] - off[l] for l in lists))
    return D, L, stats


def range_brute_force(offsets, codes, codebooks, centroids, xq, probes, radius):
    lims, D, L = [0], [], []
    rad = np.float32(radius)
    seen = 0
    for q in range(len(xq)):
        cand, _ = candidates(offsets, codes, codebooks, centroids, xq[q], probes[q])
        hits = {}
        for dist, l, o in cand:
            if dist < rad:
                hits.setdefault(l, []).append((dist, (l << 32) | o))
        for p in probes[q]:
            for dist, label in hits.pop(int(p), []):  # (popped: the first mention of a list owns its hits)
                D.append(dist)
                L.append(label)
                seen += 1
            lims.append(seen)
    return np.array(lims, np.uint64), np.array(D, np.float32), np.array(L, np.int64)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def obj(d, M):
    """ir.obj(d, M) (lists of EDGE_SIZES, random code bytes, grid codebooks) plus integer-grid centroids; vecs = what the codes stand
    for under by_residual"""
    o = dict(ir.obj(d, M))
    R, nlist = o["R"], o["nlist"]
    assert d * (3 * R) ** 2 < 2 ** 24
    o["centroids"] = np.random.default_rng(500 + d).integers(-R, R + 1, (nlist, d)).astype(np.float32)
    o["vecs"] = stored(o["offsets"], o["codes"], o["codebooks"], o["centroids"])
    return _freeze(o)


def queries(d, nq):
    return ir.queries(d, nq)


@functools.lru_cache(maxsize=None)
def radii(d, M):
    """three radii over the designed object and EDGE_ROWS: no hit, some (the median distance: a candidate's own, compared strictly),
    all"""
    o = obj(d, M)
    D = rr.model(o["offsets"], o["vecs"], queries(d, len(EDGE_ROWS)), EDGE_ROWS, np.inf)[1]
    return (0.0, float(np.sort(D)[D.size // 2]), float("inf"))


SHAPE_M = {"distinct": 4, "ties": 2}


@functools.lru_cache(maxsize=None)
def shape(name):
    """ir.shape(name) as a residual-PQ index: the residual of every vector against its list's centroid, encoded to the nearest entry
    (the first of equals) of grid codebooks [M, 256, d / M]"""
    s = dict(ir.shape(name))
    d, R, M = s["d"], s["R"], SHAPE_M[name]
    assert d * (3 * R) ** 2 < 2 ** 24
    dsub = d // M
    cb = np.random.default_rng(77).integers(-R, R + 1, size=(M, 256, dsub)).astype(np.float32)
    res = s["vecs"] - s["centroids"][s["assign"][s["ids"]]]
    codes = np.stack([((res[:, None, m * dsub:(m + 1) * dsub] - cb[m][None]) ** 2).sum(2).argmin(1) for m in range(M)], 1).astype(np.uint8)
    s.update(M=M, kind=ir.PQ8, codebooks=cb, codes=codes, flat_vecs=s["vecs"])
    s["vecs"] = stored(s["offsets"], codes, cb, s["centroids"])
    return _freeze(s)


@functools.lru_cache(maxsize=None)
def expected(name, k=None):
    s = shape(name)
    out = ir.model(s["offsets"], s["vecs"], s["xq"], s["probes"], k or s["k"])
    for a in out:
        a.setflags(write=False)
    return out


def cases_text(cases):
    """cases: [(obj dict, xq, probes, k, radius)] -> the text tests/ivf_residual_test.cpp reads, the model's answers included"""
    def floats(a):
        return " ".join("inf" if np.isinf(v) else repr(float(v)) for v in np.asarray(a, dtype=np.float32).reshape(-1))

    lines = [str(len(cases))]
    for o, xq, probes, k, radius in cases:
        D, L, st = ir.model(o["offsets"], o["vecs"], xq, probes, k)
        lims, rD, rL = rr.model(o["offsets"], o["vecs"], xq, probes, radius)
        lines.append(f"{o['nlist']} {o['ntotal']} {o['d']} {o['M']} {xq.shape[0]} {probes.shape[1]} {k} {float(radius)!r} {rD.size}")
        lines.append(" ".join(map(str, np.asarray(o["offsets"]).tolist())))
        lines.append(" ".join(map(str, o["codes"].reshape(-1).tolist())))
        lines.append(floats(o["codebooks"]))
        lines.append(floats(o["centroids"]))
        lines.append(floats(xq))
        lines.append(" ".join(map(str, probes.reshape(-1).tolist())))
        lines.append(floats(D))
        lines.append(" ".join(map(str, L.reshape(-1).tolist())))
        lines.append(" ".join(map(str, st.reshape(-1).tolist())))
        lines.append(" ".join(map(str, lims.tolist())))
        lines.append(floats(rD))
        lines.append(" ".join(map(str, rL.tolist())))
    return "\n".join(lines) + "\n"


# the plan of csrc/ivf_residual_plan.h, restated (tests/ivf_residual_test.cpp `plan` prints the header's own figures)
def plan_lds(k, nprobe, d, M):
    """the scan's LDS; k = 0: the range search's (no pools)"""
    r16 = lambda b: (b + 15) // 16 * 16
    pools = 2 * k * 8 + 64 * 8 + 64 * 4 if k else 0
    return pools + r16(nprobe * 4) + 2 * r16(d * 4) + 1024 * M


plan_resident, plan_pieces, plan_slot_items = ir.plan_resident, ir.plan_pieces, ir.plan_slot_items

# the one-CU batches (a context of one compute unit; scan lds 18560 -> 8 resident wavefronts, range lds 17472 -> 9): nq with S == 1
# whose wavefronts take three items or four (a ragged last trip), nq with S == 4 where some slots go round
ONE_CU = dict(d=128, M=16, nprobe=16, k=20, nq_whole=29, nq_cut=3)
