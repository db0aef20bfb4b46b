"""What a subset must produce, stated without the library (numpy).

An object over nlist lists: old_l is list l in the object's own order (what decode_all returns, cut by the offsets), n = |old_l|,
T = ntotal.  A subset type and two arguments name the entries a new object over the same lists takes, order kept (include/vidc.h,
"subset"; ids and all arithmetic unsigned 64-bit, done here in Python integers):

    ID_RANGE (0)          a1 <= id < a2
    ID_MOD (1)            id % a1 == a2                                           needs a1 >= 1, a2 < a1
    ELEMENT_RANGE (2)     i1 <= i < i2, i1 = off[l+1]*a1 // T - off[l]*a1 // T, i2 the same with a2     needs a1 <= a2 <= T
    INVLIST_FRACTION (3)  n*a2 // a1 <= i < n*(a2+1) // a1                        needs 1 <= a1 < 2^32, a2 < a1
    INVLIST (4)           a1 <= l < a2

The new object is the one the ordinary encoder builds from the CSR form of S; this module gives the taken mask, that CSR, the class of
every ROC list (keep the stream / empty / re-encode), the refusals a subset makes before any device work, the kind of ID_MOD
arithmetic and the bytes a call reads back.

It is an ordinary helper module: it never imports the product package.
"""
import numpy as np

ID_RANGE, ID_MOD, ELEMENT_RANGE, INVLIST_FRACTION, INVLIST = range(5)
KEEP, EMPTY, PARTIAL = 0, 1, 2  # the ROC list classes (csrc/subset_plan.h)
OK, ERR_NULL, ERR_TYPE, ERR_ARGS = range(4)
MOD_MASK, MOD_U32, MOD_U64 = 0, 1, 2


def refusal(any_null, subset_type, a1, a2, T):
    """what a subset refuses before any device work, in the order it is reported"""
    if any_null:
        return ERR_NULL
    if subset_type not in (0, 1, 2, 3, 4):
        return ERR_TYPE
    ok = {ID_RANGE: True, ID_MOD: a1 >= 1 and a2 < a1, ELEMENT_RANGE: a1 <= a2 <= T,
          INVLIST_FRACTION: 1 <= a1 < 2 ** 32 and a2 < a1, INVLIST: True}[subset_type]
    return OK if ok else ERR_ARGS


def bounds(subset_type, a1, a2, offsets):
    """the positional types: int64[nlist] i1, i2 with i2 >= i1 (a list with i1 > i2 takes nothing: i2 = i1)"""
    off = [int(x) for x in np.asarray(offsets, dtype=np.uint64)]
    T = off[-1]
    i1, i2 = [], []
    for l in range(len(off) - 1):
        n = off[l + 1] - off[l]
        if subset_type == ELEMENT_RANGE:
            lo, hi = (off[l + 1] * a1 // T - off[l] * a1 // T, off[l + 1] * a2 // T - off[l] * a2 // T) if T else (0, 0)
        elif subset_type == INVLIST_FRACTION:
            lo, hi = n * a2 // a1, n * (a2 + 1) // a1
        else:
            assert subset_type == INVLIST
            lo, hi = (0, n) if a1 <= l < a2 else (0, 0)
        i1.append(lo)
        i2.append(max(lo, hi))
    return np.array(i1, np.int64), np.array(i2, np.int64)


def taken_mask(subset_type, a1, a2, offsets, ids):
    """uint8[T]: 1 where that position of the object's decode_all order is in the subset"""
    assert refusal(False, subset_type, a1, a2, int(np.asarray(offsets)[-1])) == OK
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    assert off[0] == 0 and off[-1] == ids.size
    if subset_type == ID_RANGE:
        return ((ids >= np.uint64(a1)) & (ids < np.uint64(a2))).astype(np.uint8)
    if subset_type == ID_MOD:
        if a1 < 2 ** 63:  # (numpy's uint64 remainder is exact)
            return (ids % np.uint64(a1) == np.uint64(a2)).astype(np.uint8)
        return np.array([int(x) % a1 == a2 for x in ids], np.uint8).reshape(-1)
    i1, i2 = bounds(subset_type, a1, a2, offsets)
    n = off[1:] - off[:-1]
    lst = np.repeat(np.arange(off.size - 1), n)
    pos = np.arange(ids.size) - off[lst]
    return ((pos >= i1[lst]) & (pos < i2[lst])).astype(np.uint8)


class Subset:
    """mask: the taken mask over the source; offsets / ids: the CSR of S; n_taken; classes: the ROC class of every list"""

    def __init__(self, mask, offsets, ids, classes):
        self.mask, self.offsets, self.ids, self.classes = mask, offsets, ids, classes
        self.n_taken = int(ids.size)
        self.nlist = offsets.size - 1


def subset(subset_type, a1, a2, offsets, ids):
    """-> Subset.  ids: what decode_all of the object returns (uint64)"""
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    mask = taken_mask(subset_type, a1, a2, offsets, ids)
    cum = np.concatenate([[0], np.cumsum(mask, dtype=np.int64)])
    new_off = cum[off]
    n, n_new = off[1:] - off[:-1], new_off[1:] - new_off[:-1]
    classes = np.where(n_new == n, KEEP, np.where(n_new == 0, EMPTY, PARTIAL)).astype(np.uint32)
    return Subset(mask, new_off.astype(np.uint64), ids[mask == 1], classes)


def roc_class(n, n_new):
    return KEEP if n_new == n else (EMPTY if n_new == 0 else PARTIAL)


def mod_kind(a1):
    """how id % a1 is computed: a power of two is a mask, a1 < 2^32 reduces the high half first, else the 64-bit remainder"""
    if a1 & (a1 - 1) == 0:
        return MOD_MASK
    return MOD_U32 if a1 < 2 ** 32 else MOD_U64


def readback_bytes(roc, subset_type, nlist, T, n_candidates, n_reencoded):
    """bytes a call copies device -> host (counts and list numbers, never an id): packed bits and Elias-Fano read the size of the
    subset; ROC reads the word total of the splice and, for the id types, the candidate count, the candidates' numbers, the count of
    re-encoded lists with the survivor total and 8 bytes per re-encoded list.  The positional types of ROC read nothing else: the host
    finds the partial lists on its mirror of the offsets."""
    if not roc:
        return 8 if T else 0
    if nlist == 0:
        return 0
    if subset_type in (ID_RANGE, ID_MOD) and T:
        return 8 + 8 + 4 * n_candidates + (16 + 8 * n_reencoded if n_candidates else 0)
    return 8
