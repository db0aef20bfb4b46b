"""What vidc_*_update_rows_dev does to a graph, as a plain numpy model.

A graph is `rows`: int32 [N_old, K], row v = the neighbours of node v, ended by the first -1 (tests/rows_ref.py).  A batch is
`nodes` (int64 [m]) and `batch` (int32 [m, K]).  The updated matrix R' has n_new >= N_old rows:

  row v = batch[i] for the LARGEST i with nodes[i] == v   (the last mention wins)
        = rows[v]                                         for v < N_old without a mention
        = the empty row (-1 in column 0)                  for a new node without a mention

A negative node is skipped and not counted; a node >= n_new is skipped and counted as invalid.  An old row is taken as its container
decodes it (`keep`: the identity here; the GPU tests pass what decode_rows answers, e.g. ascending rows for Elias-Fano), a batch row as
it was given.

It is an ordinary helper module: no torch, no oracle, nothing from the product package.
"""
import numpy as np


def slot_table(nodes, n_new):
    """-> (int64 [n_new]: 1 + the largest batch index that names v, 0 = none; the number of nodes >= n_new)"""
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    slot = np.zeros(n_new, dtype=np.int64)
    ok = (nodes >= 0) & (nodes < n_new)
    np.maximum.at(slot, nodes[ok], np.flatnonzero(ok) + 1)
    return slot, int(((nodes >= 0) & (nodes >= n_new)).sum())


def update_rows(rows, nodes, batch, n_new=None):
    """-> (R' int32 [n_new, K], invalid count, slot table)"""
    rows = np.asarray(rows, dtype=np.int32)
    n_old, K = rows.shape
    n_new = n_old if n_new is None else int(n_new)
    assert n_new >= n_old
    batch = np.asarray(batch, dtype=np.int32).reshape(-1, K)
    slot, invalid = slot_table(nodes, n_new)
    assert batch.shape[0] == np.asarray(nodes).size
    out = np.full((n_new, K), -1, dtype=np.int32)
    out[:n_old] = rows
    hit = np.flatnonzero(slot)
    out[hit] = batch[slot[hit] - 1]
    return out, invalid, slot


def update_rows_loop(rows, nodes, batch, n_new=None):
    """the same by the definition, one batch entry after the other -> (R', invalid count)"""
    rows = np.asarray(rows, dtype=np.int32)
    n_old, K = rows.shape
    n_new = n_old if n_new is None else int(n_new)
    out = [list(map(int, rows[v])) if v < n_old else [-1] * K for v in range(n_new)]
    invalid = 0
    for i, v in enumerate(np.asarray(nodes, dtype=np.int64).reshape(-1).tolist()):
        if v < 0:
            continue
        if v >= n_new:
            invalid += 1
            continue
        out[v] = [int(x) for x in np.asarray(batch, dtype=np.int32).reshape(-1, K)[i]]
    return np.array(out, dtype=np.int32).reshape(n_new, K), invalid


# ------------------------------------------------------------------------------------------------------------------- batches
BATCHES = ("random", "repeats_in_tile", "repeats_across_tiles", "negatives", "beyond", "every_node", "every_node_twice", "mixed")


def batch_nodes(name, m, n_new, seed=0):
    """int64 [m] node numbers of a named batch shape:
      random                 uniform valid nodes
      repeats_in_tile        groups of up to 64 consecutive entries name the same node
      repeats_across_tiles   entry i and entry i + 64 (and i + 128 ...) name the same node
      negatives              a third of the entries are -1 or another negative number
      beyond                 a third of the entries are >= n_new (n_new itself, n_new + 1, 2^40)
      every_node             a permutation of every node (m >= n_new: the rest random)
      every_node_twice       every node at least twice when m allows it
      mixed                  all of the above together"""
    rng = np.random.default_rng([seed, m, n_new, BATCHES.index(name)])
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    hi = max(n_new, 1)
    base = rng.integers(0, hi, m)
    if n_new == 0:
        base[:] = 0  # (every entry is then beyond the object)
    if name == "random":
        out = base
    elif name == "repeats_in_tile":
        out = np.repeat(rng.integers(0, hi, (m + 6) // 7), 7)[:m]
    elif name == "repeats_across_tiles":
        out = base[np.arange(m) % 64]
    elif name == "negatives":
        out = np.where(rng.random(m) < 0.34, rng.choice([-1, -2, -(1 << 40)], m), base)
    elif name == "beyond":
        out = np.where(rng.random(m) < 0.34, rng.choice([n_new, n_new + 1, 1 << 40], m), base)
    elif name in ("every_node", "every_node_twice"):
        reps = 2 if name == "every_node_twice" else 1
        every = np.concatenate([rng.permutation(n_new) for _ in range(reps)]) if n_new else np.zeros(0, np.int64)
        out = np.concatenate([every, base])[:m] if every.size < m else every[:m]
    elif name == "mixed":
        out = base[np.arange(m) % 64].copy()
        r = rng.random(m)
        out[r < 0.15] = -1
        out[(r >= 0.15) & (r < 0.3)] = n_new + 3
        out[(r >= 0.3) & (r < 0.5)] = out[0]
    else:
        raise ValueError(name)
    return np.asarray(out, dtype=np.int64)
