"""The numpy model of the one-launch graph search (vidc_*_search_dev, csrc/graph_search_ref.h): graph_search.search with the step cap,
the id >= N rule and the two counters added, and the shapes the CPU and GPU tests share.

Test data are integer grids: coordinates are integers in [-R, R] stored as float32, so every squared distance is an exact integer
below 2^24 in any summation order and D, I and stats can be compared element for element.  Ties are frequent and decided by node id.
"""
import functools

import numpy as np

# N, d, K, L, k, R, nq
SHAPES = {
    "n500": (500, 4, 16, 32, 10, 3, 40),
    "n300": (300, 8, 7, 8, 8, 2, 40),
    "n2000": (2000, 16, 64, 64, 10, 3, 40),
    "n700_k80": (700, 4, 80, 16, 5, 3, 20),
}


def model(rows, x, xq, k, L, entry=0, max_rounds=0):
    """-> D float32 [nq, k], I int64 [nq, k], stats uint32 [nq, 2] = (steps, distances computed, the entry's included).
    rows: int32 [N, K]; a row ends at its first negative entry; an id >= N is skipped; a repeated id counts once."""
    rows = np.asarray(rows, dtype=np.int32)
    x = np.asarray(x, dtype=np.float32)
    xq = np.asarray(xq, dtype=np.float32)
    N, nq = x.shape[0], xq.shape[0]
    D = np.full((nq, k), np.inf, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    stats = np.zeros((nq, 2), dtype=np.uint32)
    bound = min(max_rounds if max_rounds else N, N)
    for q in range(nq):
        visited = np.zeros(N, dtype=bool)
        visited[entry] = True
        pool = [(np.float32(((x[entry] - xq[q]) ** 2).sum(dtype=np.float32)), entry, False)]
        steps, dists = 0, 1
        while steps < bound:
            cand = [i for i, t in enumerate(pool) if not t[2]]
            if not cand:
                break
            i = cand[0]
            dist, node, _ = pool[i]
            pool[i] = (dist, node, True)
            steps += 1
            for v in rows[node]:
                v = int(v)
                if v < 0:
                    break
                if v >= N or visited[v]:
                    continue
                visited[v] = True
                dists += 1
                pool.append((np.float32(((x[v] - xq[q]) ** 2).sum(dtype=np.float32)), v, False))
            pool.sort(key=lambda t: (t[0], t[1]))
            pool = pool[:L]
        top = pool[:k]
        D[q, : len(top)] = [t[0] for t in top]
        I[q, : len(top)] = [t[1] for t in top]
        stats[q] = (steps, dists)
    return D, I, stats


def random_rows(rng, N, K):
    """uniform random lengths in 0..K, neighbours drawn without replacement, -1 padded"""
    rows = np.full((N, K), -1, dtype=np.int32)
    for i, n in enumerate(rng.integers(0, K + 1, size=N)):
        rows[i, :n] = rng.choice(N, size=int(n), replace=False)
    return rows


@functools.lru_cache(maxsize=None)
def shape(name):
    """-> dict(rows, x, xq, N, d, K, L, k, nq) of SHAPES[name]; entry 0 (its row is made non-empty: the search has to start)"""
    N, d, K, L, k, R, nq = SHAPES[name]
    rng = np.random.default_rng(5)
    rows = random_rows(rng, N, K)
    if rows[0, 0] < 0:
        rows[0, : K // 2] = rng.choice(np.arange(1, N), size=K // 2, replace=False)
    x = rng.integers(-R, R + 1, size=(N, d)).astype(np.float32)
    xq = rng.integers(-R, R + 1, size=(nq, d)).astype(np.float32)
    for a in (rows, x, xq):
        a.setflags(write=False)
    return dict(rows=rows, x=x, xq=xq, N=N, d=d, K=K, L=L, k=k, nq=nq, R=R)


@functools.lru_cache(maxsize=None)
def expected(name, k=None, L=None, max_rounds=0, nq=None):
    """the model's (D, I, stats) on a shape, computed once per parameter set and shared (read-only)"""
    s = shape(name)
    out = model(s["rows"], s["x"], s["xq"][: nq or s["nq"]], k or s["k"], L or s["L"], 0, max_rounds)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hostile(entry_row_empty=False, big_ids=True):
    """A small graph whose rows hold what a decoder may meet: row 1 repeats a neighbour, row 2 holds ids >= N (big_ids; raw rows only
    can carry them), row 3 is empty, and with entry_row_empty row 0 (the entry's) is empty too.  -> dict like shape()."""
    N, d, K, L, k, R, nq = 120, 4, 12, 8, 5, 2, 12
    rng = np.random.default_rng(11)
    rows = random_rows(rng, N, K)
    rows[0] = -1
    if not entry_row_empty:
        rows[0, :6] = [1, 2, 3, 4, 5, 6]
    rows[1] = -1
    rows[1, :7] = [9, 17, 9, 40, 17, 9, 41]
    rows[2] = -1
    rows[2, :5] = [50, N, 51, 2 ** 31 - 1, N + 7] if big_ids else [50, 52, 51, 53, 54]
    rows[3] = -1
    x = rng.integers(-R, R + 1, size=(N, d)).astype(np.float32)
    xq = rng.integers(-R, R + 1, size=(nq, d)).astype(np.float32)
    # the first queries sit on nodes 1, 2 and 3, so those rows are expanded early
    xq[:3] = x[1:4]
    for a in (rows, x, xq):
        a.setflags(write=False)
    return dict(rows=rows, x=x, xq=xq, N=N, d=d, K=K, L=L, k=k, nq=nq, R=R)


def expanded_nodes(rows, x, xq, L, entry=0):
    """the nodes every query expands, in order (what the hostile rows are checked with)"""
    out = []
    N = x.shape[0]
    for q in range(xq.shape[0]):
        visited, pool, order = {entry}, [(float(((x[entry] - xq[q]) ** 2).sum()), entry, False)], []
        while True:
            cand = [i for i, t in enumerate(pool) if not t[2]]
            if not cand:
                break
            dist, node, _ = pool[cand[0]]
            pool[cand[0]] = (dist, node, True)
            order.append(node)
            for v in rows[node]:
                v = int(v)
                if v < 0:
                    break
                if v >= N or v in visited:
                    continue
                visited.add(v)
                pool.append((float(((x[v] - xq[q]) ** 2).sum()), v, False))
            pool.sort(key=lambda t: (t[0], t[1]))
            pool = pool[:L]
        out.append(order)
    return out


def cases_text(cases):
    """cases: [(rows, x, xq, k, L, entry, max_rounds)] -> the text tests/graph_search_test.cpp reads (the model's answers included)"""
    lines = [str(len(cases))]
    for rows, x, xq, k, L, entry, max_rounds in cases:
        D, I, st = model(rows, x, xq, k, L, entry, max_rounds)
        N, K = rows.shape
        lines.append(f"{N} {K} {x.shape[1]} {xq.shape[0]} {k} {L} {entry} {max_rounds}")
        lines.append(" ".join(map(str, rows.reshape(-1).tolist())))
        lines.append(" ".join(repr(float(v)) for v in x.reshape(-1)))
        lines.append(" ".join(repr(float(v)) for v in xq.reshape(-1)))
        lines.append(" ".join("inf" if np.isinf(v) else repr(float(v)) for v in D.reshape(-1)))
        lines.append(" ".join(map(str, I.reshape(-1).tolist())))
        lines.append(" ".join(map(str, st.reshape(-1).tolist())))
    return "\n".join(lines) + "\n"


# the plan of csrc/graph_search_plan.h, restated (tests/graph_search_test.cpp `plan` prints the header's own figures)
def plan_slots(nq, num_cu):
    return max(1, min(nq, num_cu * 32, 1024))


def plan_slot_queries(nq, nslots, s):
    return (nq - 1 - s) // nslots + 1 if s < nq else 0
