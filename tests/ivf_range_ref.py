"""The numpy model of the IVF range search on the device (vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev,
csrc/ivf_range_ref.h) and the radii and one-CU batches the CPU and GPU tests share.

Slot s = q * nprobe + j is entry j of query q's probe row.  Its candidates are the entries of the list it names, in ascending offset
order, if the entry is a valid list number and the first mention of that list in the row; every other slot has none.  A candidate
is a hit iff its float32 squared distance is strictly below the radius.  slot_lims is the exclusive prefix sum of the hits per slot;
the r-th hit of slot s lies at slot_lims[s] + r of D / labels, label = list_no << 32 | offset.

Data are the integer grids of tests/ivf_scan_ref.py: every distance is an exact float32 integer, so everything is compared element
for element, and radius = a distance +- 0.5 lies strictly between two distances.
"""
import functools

import numpy as np

import ivf_scan_ref as ir

POISON_D = np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0]
POISON_L = np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0]


def slot_lists(row, nlist):
    """per entry of a probe row: the list it scans, or -1 (invalid, or a list an earlier entry named)"""
    seen, out = set(), []
    for p in row:
        p = int(p)
        if 0 <= p < nlist and p not in seen:
            seen.add(p)
            out.append(p)
        else:
            out.append(-1)
    return out


def model(offsets, vecs, xq, probes, radius):
    """-> slot_lims uint64 [nq * nprobe + 1], D float32 [total], labels int64 [total]"""
    off = np.asarray(offsets).astype(np.int64)
    nlist, ntotal = off.size - 1, vecs.shape[0]
    xq = np.asarray(xq, dtype=np.float32)
    probes = np.asarray(probes, dtype=np.int64)
    nq, nprobe = probes.shape
    radius = np.float32(radius)
    counts = np.zeros(nq * nprobe, np.uint64)
    Ds, Ls = [], []
    for q in range(nq):
        for j, l in enumerate(slot_lists(probes[q], nlist)):
            if l < 0:
                continue
            b = min(int(off[l + 1]), ntotal)
            a = min(int(off[l]), b)
            if b <= a:
                continue
            dist = ir.l2(vecs[a:b], xq[q])
            with np.errstate(invalid="ignore"):
                hit = np.flatnonzero(dist < radius)  # (a NaN radius: no hit)
            counts[q * nprobe + j] = hit.size
            pos = a + hit
            lists = np.searchsorted(off, pos, side="right") - 1  # the label rule of the scan
            Ds.append(dist[hit])
            Ls.append((lists.astype(np.int64) << 32) | (pos - off[lists]))
    lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    D = np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32)
    L = np.concatenate(Ls).astype(np.int64) if Ls else np.zeros(0, np.int64)
    return lims, D, L


def brute_force(offsets, vecs, xq, probes, radius):
    """the statement again as loops over (query, probe entry, offset), written from include/vidc.h: python lists, no positions"""
    off = [int(v) for v in offsets]
    nlist = len(off) - 1
    lims, D, L = [0], [], []
    r = np.float32(radius)
    for q in range(len(xq)):
        for j, p in enumerate(probes[q]):
            p = int(p)
            first = 0 <= p < nlist and all(int(e) != p for e in probes[q][:j])
            if first:
                for o in range(off[p + 1] - off[p]):
                    v = vecs[off[p] + o]
                    dist = np.float32(0)
                    for i in range(v.size):
                        t = np.float32(xq[q][i]) - np.float32(v[i])
                        dist = np.float32(dist + t * t)
                    if dist < r:
                        D.append(dist)
                        L.append((p << 32) | o)
            lims.append(len(D))
    return np.array(lims, np.uint64), np.array(D, np.float32), np.array(L, np.int64)


def fill_model(offsets, vecs, xq, probes, radius, lims, capacity):
    """what a fill with the given slot limits and capacity leaves in poisoned arrays of `capacity` entries: the r-th hit of slot s at
    lims[s] + r if that is below lims[s + 1] and below the capacity (the slot limits of another radius, a short capacity)"""
    own, D, L = model(offsets, vecs, xq, probes, radius)
    outD = np.full(capacity, POISON_D, np.float32)
    outL = np.full(capacity, POISON_L, np.int64)
    lims = [int(v) for v in lims]
    for s in range(own.size - 1):
        a, b = int(own[s]), int(own[s + 1])
        for r in range(b - a):
            p = (lims[s] + r) % 2 ** 64
            if p < lims[s + 1] and p < capacity:
                outD[p], outL[p] = D[a + r], L[a + r]
    return outD, outL


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def equal_radius(d, M=0):
    """a radius that equals some candidate's distance over the designed object and rows: the median of the positive distances"""
    o, xq = ir.obj(d, M), ir.queries(d, len(ir.EDGE_ROWS))
    D = model(o["offsets"], o["vecs"], xq, ir.EDGE_ROWS, np.inf)[1]
    return float(np.sort(D[D > 0])[(D > 0).sum() // 2])


def radii(d, M=0):
    """the radii of the tests: a candidate's distance, that +- 0.5, 0, -1, +inf, NaN"""
    eq = equal_radius(d, M)
    return (eq, eq - 0.5, eq + 0.5, 0.0, -1.0, float("inf"), float("nan"))


# the one-CU batches (a context of one compute unit): (d, M, nprobe) -> nq with S == 1 whose wavefronts take three items or four (a
# ragged last trip), nq with S > 1.  The cut is the smallest S with nq * S >= the resident wavefronts, so a call with S > 1 has fewer
# than two items per wavefront: three and more are asserted at S == 1.
ONE_CU = {"flat": dict(d=4, M=0, nprobe=16, nq_whole=101, nq_cut=13),
          "pq": dict(d=128, M=16, nprobe=16, nq_whole=31, nq_cut=3)}


# the plan of csrc/ivf_range_plan.h, restated (tests/ivf_range_test.cpp `plan` prints the header's own figures)
def plan_lds(kind, nprobe, d, M):
    r16 = lambda b: (b + 15) // 16 * 16
    return r16(d * 4) + r16(nprobe * 4) + M * 256 * 4 if kind == ir.PQ8 else 256 + r16(nprobe * 4) + r16(d * 4)


def cases_text(cases):
    """cases: [(obj dict, xq, probes, radius)] -> the text tests/ivf_range_test.cpp reads, the model's answers included"""
    def floats(a):
        return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float32).reshape(-1))

    lines = [str(len(cases))]
    for o, xq, probes, radius in cases:
        lims, D, L = model(o["offsets"], o["vecs"], xq, probes, radius)
        lines.append(f"{o['nlist']} {o['ntotal']} {o['kind']} {o['d']} {o['M']} {xq.shape[0]} {probes.shape[1]} {float(radius)!r} {D.size}")
        lines.append(" ".join(map(str, np.asarray(o["offsets"]).tolist())))
        lines.append(" ".join(map(str, o["codes"].reshape(-1).tolist())))
        lines.append(floats(o["codebooks"]) if o["M"] else "")
        lines.append(floats(xq))
        lines.append(" ".join(map(str, probes.reshape(-1).tolist())))
        lines.append(" ".join(map(str, lims.tolist())))
        lines.append(floats(D))
        lines.append(" ".join(map(str, L.tolist())))
    return "\n".join(lines) + "\n"
