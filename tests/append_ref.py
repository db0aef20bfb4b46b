"""What an append must produce, stated without the library (numpy plus the CPU oracle for ROC's order).

A batch is n pairs (list_nos[i], add_ids[i]).  With old_l = list l of the old object in the object's own order, the merged input of
list l is  M_l = old_l ++ [add_ids[i] for every i with list_nos[i] == l, in ascending i]  (include/vidc.h, "append").  A negative list
number is skipped and not counted, one >= nlist is skipped and counted.  The appended object is the one the ordinary encoder builds
from the CSR form of M; this module gives that CSR, the label (list_no << 32 | offset) of every batch entry in the new object, and the
permutation over M that a re-ordering container reports.

It is an ordinary helper module: it never imports the product package.
"""
import numpy as np

KINDS = ("packed", "ef", "wt", "roc")


class Merged:
    """offsets / ids: the CSR of M.  old_n[l] = |old_l|.  valid[i]: pair i was placed.  rank[i]: its number among the batch entries
    of its list (-1 for a skipped pair).  invalid: pairs whose list number is >= nlist."""

    def __init__(self, offsets, ids, old_n, list_nos, valid, rank, invalid):
        self.offsets, self.ids, self.old_n = offsets, ids, old_n
        self.list_nos, self.valid, self.rank, self.invalid = list_nos, valid, rank, invalid
        self.nlist = offsets.size - 1


def merge(offsets, ids_in_object_order, list_nos, add_ids):
    """-> Merged.  offsets uint64[nlist + 1], ids_in_object_order: what decode_all of the old object returns."""
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    old = np.asarray(ids_in_object_order, dtype=np.uint64)
    ln = np.asarray(list_nos, dtype=np.int64).reshape(-1)
    add = np.asarray(add_ids, dtype=np.uint64).reshape(-1)
    assert ln.size == add.size and off[0] == 0 and off[-1] == old.size
    nlist = off.size - 1
    valid = (ln >= 0) & (ln < nlist)
    invalid = int(np.count_nonzero(ln >= nlist))
    idx = np.flatnonzero(valid)
    order = idx[np.argsort(ln[idx], kind="stable")]  # batch entries grouped by list, ascending i inside a list
    cnt = np.bincount(ln[idx], minlength=nlist).astype(np.int64)
    add_off = np.concatenate([[0], np.cumsum(cnt)])
    old_n = off[1:] - off[:-1]
    new_off = off + add_off
    out = np.empty(int(new_off[-1]), np.uint64)
    # old entries keep their offsets inside the list
    l_old = np.repeat(np.arange(nlist), old_n)
    out[np.arange(old.size) + add_off[l_old]] = old
    rank = np.full(ln.size, -1, np.int64)
    rank[order] = np.arange(order.size) - add_off[ln[order]]
    out[new_off[ln[order]] + old_n[ln[order]] + rank[order]] = add[order]
    return Merged(new_off.astype(np.uint64), out, old_n, ln, valid, rank, invalid)


def list_perm(kind, ids, oracle=None):
    """the permutation a container of `kind` reports for ONE list built from `ids`: perm[q] = input position of the entry at offset q"""
    ids = np.asarray(ids, dtype=np.uint64)
    if kind in ("packed", "wt"):
        return np.arange(ids.size, dtype=np.uint32)
    if kind == "ef":
        return np.argsort(ids, kind="stable").astype(np.uint32)  # std::sort of (id, position) pairs, custom_invlists_impl.cpp:336
    assert kind == "roc"
    if ids.size == 0:
        return np.zeros(0, np.uint32)
    return np.asarray(oracle.roc_encode(ids, oracle.list_precision(ids))["perm"], dtype=np.uint32)


def perm(kind, m, oracle=None):
    """uint32[ntotal_new]: the permutation over M, list by list (positions local to the list)"""
    off = m.offsets.astype(np.int64)
    parts = [list_perm(kind, m.ids[off[l]:off[l + 1]], oracle) for l in range(m.nlist)]
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def labels(kind, m, oracle=None):
    """int64[n]: list_no << 32 | offset of every batch entry in the new object, -1 for a skipped pair"""
    assert kind in KINDS
    lab = np.full(m.list_nos.size, -1, np.int64)
    v = np.flatnonzero(m.valid)
    at = m.old_n[m.list_nos[v]] + m.rank[v]  # position in M_l
    if kind in ("ef", "roc"):
        off = m.offsets.astype(np.int64)
        inv = {}
        for l in np.unique(m.list_nos[v]):
            p = list_perm(kind, m.ids[off[l]:off[l + 1]], oracle).astype(np.int64)
            q = np.empty(p.size, np.int64)
            q[p] = np.arange(p.size)
            inv[int(l)] = q
        at = np.array([inv[int(l)][int(a)] for l, a in zip(m.list_nos[v], at)], dtype=np.int64).reshape(-1)
    lab[v] = (m.list_nos[v] << 32) | at
    return lab
