"""What a remove must produce, stated without the library (numpy only).

A batch is n pairs (list_nos[i], rm_ids[i]).  Pairs mode (list_nos given): an entry of list l is removed iff some pair has that list
number and an id equal to the entry's id, all 64 bits; a negative list number is skipped and not counted, one >= nlist is skipped and
counted as invalid.  Any-list mode (list_nos None): an entry of any list is removed iff its id equals some rm_ids[i].  Every copy of a
matching id inside a list goes.  A valid pair that matches no entry is missing, each copy of a repeated pair like the first.  The
survivors keep their order: with old_l = list l in the object's own order, S_l = old_l without the removed entries (include/vidc.h,
"remove").  The new object is the one the ordinary encoder builds from the CSR form of S.

It is an ordinary helper module: it never imports the product package.
"""
import numpy as np


class Removed:
    """offsets / ids: the CSR of S.  mask[p] = 1 where position p of the old decode_all order was removed.  missing: valid pairs that
    matched no entry.  invalid: pairs whose list number is >= nlist."""

    def __init__(self, offsets, ids, mask, missing, invalid):
        self.offsets, self.ids, self.mask, self.missing, self.invalid = offsets, ids, mask, missing, invalid
        self.nlist = offsets.size - 1
        self.removed = int(mask.sum())


def remove(offsets, ids_in_object_order, list_nos, rm_ids):
    """-> Removed.  offsets uint64[nlist + 1], ids_in_object_order: what decode_all of the old object returns."""
    off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    old = np.asarray(ids_in_object_order, dtype=np.uint64).reshape(-1)
    rm = np.asarray(rm_ids, dtype=np.uint64).reshape(-1)
    assert off[0] == 0 and off[-1] == old.size
    nlist = off.size - 1
    sizes = off[1:] - off[:-1]
    l_of = np.repeat(np.arange(nlist, dtype=np.int64), sizes)
    if list_nos is None:
        invalid = 0
        mask = np.isin(old, rm)
        missing = int(np.count_nonzero(~np.isin(rm, old)))
    else:
        ln = np.asarray(list_nos, dtype=np.int64).reshape(-1)
        assert ln.size == rm.size
        valid = (ln >= 0) & (ln < nlist)
        invalid = int(np.count_nonzero(ln >= nlist))
        # (list, id) as one integer key: the id's rank among all ids in play stands for its 64 bits
        uniq, rank = np.unique(np.concatenate([old, rm[valid]]), return_inverse=True)
        rank = rank.reshape(-1).astype(np.int64)
        have = l_of * np.int64(uniq.size) + rank[:old.size]
        want = ln[valid] * np.int64(uniq.size) + rank[old.size:]
        mask = np.isin(have, want)
        missing = int(np.count_nonzero(~np.isin(want, have)))
    kills = np.bincount(l_of[mask], minlength=nlist).astype(np.int64) if old.size else np.zeros(nlist, np.int64)
    new_off = np.concatenate([[0], np.cumsum(sizes - kills)]).astype(np.uint64)
    return Removed(new_off, old[~mask], mask.astype(np.uint8), missing, invalid)
