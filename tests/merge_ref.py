"""What a merge must produce, stated without the library (numpy).

Two objects over the same nlist lists: a_l and b_l are list l of each in the object's own order (what decode_all returns, cut by the
offsets).  The merged input of list l is  M_l = a_l ++ [x + add_id for x in b_l]  (include/vidc.h, "merge").  The merged object is
the one the ordinary encoder builds from the CSR form of M; this module gives that CSR, the `src` array of the new object (for every
position of its decode_all order: p >= 0 = position p of a's decode_all order, ~p = position p of b's) for the three kinds of
container -- input order, stable ascending order, a given permutation over M --, the class of every ROC list (which source its
stream comes from) and the refusals a merge makes before any device work.

It is an ordinary helper module: it never imports the product package.
"""
import numpy as np

KEEP_A, KEEP_B, ENCODE = 0, 1, 2  # the ROC list classes (csrc/merge_plan.h)
OK, ERR_NULL, ERR_NLIST, ERR_DEVICE, ERR_NTOTAL = range(5)
ROC_MAX_LIST = 262144


class Merged:
    """offsets / ids: the CSR of M.  a_n[l] = |a_l|, b_n[l] = |b_l|, a_off / b_off: the sources' offsets (int64)."""

    def __init__(self, offsets, ids, a_off, b_off):
        self.offsets, self.ids, self.a_off, self.b_off = offsets, ids, a_off, b_off
        self.a_n, self.b_n = a_off[1:] - a_off[:-1], b_off[1:] - b_off[:-1]
        self.nlist = offsets.size - 1


def merge(a_offsets, a_ids, b_offsets, b_ids, add_id=0):
    """-> Merged.  a_ids / b_ids: what decode_all of each object returns (uint64); the shift wraps mod 2^64 as the device's does."""
    ao = np.asarray(a_offsets, dtype=np.uint64).astype(np.int64)
    bo = np.asarray(b_offsets, dtype=np.uint64).astype(np.int64)
    a = np.asarray(a_ids, dtype=np.uint64).reshape(-1)
    b = np.asarray(b_ids, dtype=np.uint64).reshape(-1)
    assert ao.size == bo.size and ao[0] == 0 and bo[0] == 0 and ao[-1] == a.size and bo[-1] == b.size
    nlist = ao.size - 1
    new_off = ao + bo
    out = np.empty(int(new_off[-1]), np.uint64)
    a_n, b_n = ao[1:] - ao[:-1], bo[1:] - bo[:-1]
    la, lb = np.repeat(np.arange(nlist), a_n), np.repeat(np.arange(nlist), b_n)
    out[np.arange(a.size) + bo[la]] = a                                    # a's entries keep their offsets inside the list
    with np.errstate(over="ignore"):
        out[np.arange(b.size) + ao[lb + 1]] = b + np.uint64(add_id)       # b's go behind them: new_off[l] + |a_l| = a_off[l + 1] + b_off[l]
    return Merged(new_off.astype(np.uint64), out, ao, bo)


def src_from_perm(m, perm):
    """int64[ntotal_new]: perm[q] (local to its list) = the position in M_l of the entry at offset q of the new list l"""
    off = m.offsets.astype(np.int64)
    l_new = np.repeat(np.arange(m.nlist), off[1:] - off[:-1])
    j = np.asarray(perm, dtype=np.int64)
    from_a = j < m.a_n[l_new]
    return np.where(from_a, m.a_off[l_new] + j, ~(m.b_off[l_new] + j - m.a_n[l_new]))


def identity_perm(m):
    off = m.offsets.astype(np.int64)
    l_new = np.repeat(np.arange(m.nlist), off[1:] - off[:-1])
    return (np.arange(int(off[-1])) - off[l_new]).astype(np.uint32)


def ascending_perm(m):
    """the stable ascending order of every M_l (Elias-Fano: std::sort of (id, position) pairs)"""
    off = m.offsets.astype(np.int64)
    parts = [np.argsort(m.ids[off[l]:off[l + 1]], kind="stable") for l in range(m.nlist)]
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def src(kind, m, perm=None):
    """`src` of the new object: kind "plain" (packed bits, wavelet tree: input order), "ascending" (Elias-Fano) or "perm" (ROC: the
    permutation the new object reports, given)"""
    if kind == "plain":
        return src_from_perm(m, identity_perm(m))
    if kind == "ascending":
        return src_from_perm(m, ascending_perm(m))
    assert kind == "perm" and perm is not None
    return src_from_perm(m, perm)


def roc_classes(m, add_id):
    """uint32[nlist]: KEEP_A where b_l is empty, KEEP_B where a_l is empty and nothing is shifted, ENCODE elsewhere"""
    cls = np.full(m.nlist, ENCODE, np.uint32)
    cls[(m.a_n == 0) & (m.b_n != 0) & (int(add_id) == 0)] = KEEP_B
    cls[m.b_n == 0] = KEEP_A
    return cls


def refusal(any_null, nlist_a, nlist_b, dev_ctx, dev_a, dev_b, ntotal_a, ntotal_b):
    """what a merge refuses before any device work, in the order it is reported"""
    if any_null:
        return ERR_NULL
    if nlist_a != nlist_b:
        return ERR_NLIST
    if dev_a != dev_ctx or dev_b != dev_ctx:
        return ERR_DEVICE
    if ntotal_a + ntotal_b >= 2 ** 32 - 1:
        return ERR_NTOTAL
    return OK


def shift_overflows(max_b, add_id, bits):
    """the largest id of b, shifted, leaves 64 bits or does not fit `bits` (64: every id fits; ROC: 31)"""
    s = int(max_b) + int(add_id)
    return s >= 2 ** 64 or (bits < 64 and s >> bits != 0)


def roc_domain_error(m, add_id, b_ids):
    """True when the ROC merge is outside its domain: a re-encoded list above ROC_MAX_LIST, or a shifted id of a re-encoded list
    >= 2^31"""
    enc = roc_classes(m, add_id) == ENCODE
    if np.any((m.a_n + m.b_n)[enc] > ROC_MAX_LIST):
        return True
    b = np.asarray(b_ids, dtype=np.uint64)
    for l in np.flatnonzero(enc):
        part = b[m.b_off[l]:m.b_off[l + 1]]
        if part.size and shift_overflows(int(part.max()), add_id, 31):
            return True
    return False
