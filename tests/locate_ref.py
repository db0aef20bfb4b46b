"""What vidc_*_locate_dev must answer, stated without the library (numpy only; written from the "locate" section of include/vidc.h).

    labels, missing, invalid = locate(offsets, ids_in_object_order, list_nos | None, ids, id_bits)

The object is given as what it decodes to: offsets[nlist + 1] and the ids of every list in the object's own order (decode_all).
labels[i] = list << 32 | offset of the first entry equal to ids[i] -- in list list_nos[i] (pairs mode) or in the first list that holds
one (list_nos None: any-list mode) --, or -1.  missing counts the valid pairs that got -1, invalid the list numbers >= nlist.
"""
import numpy as np


def _u64(x):
    """the 64 bits of every id (int64 and uint64 arrays carry the same bytes)"""
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view(np.uint64) if x.dtype in (np.int64, np.uint64) else x.astype(np.uint64)


def locate(offsets, obj_ids, list_nos, ids, id_bits=64):
    off = np.asarray(offsets).astype(np.int64)
    obj, ids = _u64(obj_ids), _u64(ids)
    nlist = off.size - 1
    assert off[0] == 0 and int(off[-1]) == obj.size
    # the first place of every id, per list and over all lists: walked backwards, so that the lowest position is what stays
    first_in_list, first_anywhere = {}, {}
    for l in range(nlist - 1, -1, -1):
        for o in range(int(off[l + 1] - off[l]) - 1, -1, -1):
            v = int(obj[off[l] + o])
            first_in_list[(l, v)] = first_anywhere[v] = (l << 32) | o
    labels = np.full(ids.size, -1, np.int64)
    missing = invalid = 0
    for i in range(ids.size):
        v = int(ids[i])
        if list_nos is None:
            table, key = first_anywhere, v
        else:
            l = int(list_nos[i])
            if l < 0:
                continue
            if l >= nlist:
                invalid += 1
                continue
            table, key = first_in_list, (l, v)
        fits = id_bits >= 64 or (v >> id_bits) == 0  # an id the object cannot hold matches nothing
        labels[i] = table.get(key, -1) if fits else -1
        missing += int(labels[i] < 0)
    return labels, missing, invalid
