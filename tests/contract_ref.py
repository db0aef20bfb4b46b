"""What a decode call must leave in memory, stated without the library.

Every decode entry point of include/vidc.h writes into a buffer its caller owns.  The contract has two halves: every element of the
promised region is defined after the call (rows: the ids, then -1 up to column K), and not one byte outside it changes.  This module
gives the tests both halves:

  expected_rows / expected_lists (RowRef / ListRef)   the promised contents, from nothing but the ids that went into the encoder:
                                                      pure numpy plus the CPU oracle (oracle/pyoracle.py)
  guarded / assert_guards_intact / assert_view_equals poisoned buffers with a guard band on either side of the region handed to
                                                      the call

It is an ordinary helper module: it never imports the product package.
"""
import numpy as np

#: bytes of guard on either side of a view: more than an allocator's rounding, many times the widest single store (16 bytes)
GUARD_BYTES = 4096
#: int32 poison: negative and not -1, so neither an id nor the row padding
POISON32 = int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0])
#: 64-bit poison: never an id (ids are < 2^63), never -1
POISON64 = 0xA5A5A5A5A5A5A5A5
POISON64_SIGNED = int(np.array([POISON64], np.uint64).view(np.int64)[0])


# ------------------------------------------------------------------------------------------------------------- rows
def _row_ids(row):
    """ids of one -1 terminated int32 row (altid_impl.cpp:61-68: the row ends at its first -1)"""
    row = np.asarray(row)
    neg = np.flatnonzero(row < 0)
    return row[: int(neg[0])] if neg.size else row


def _roc_order(ids, oracle):
    """the pinned reference codec's answer for one id set: decode(encode(sorted ids)), its power-of-two-maximum quirk included"""
    s = np.sort(np.asarray(ids, dtype=np.uint64))
    if s.size == 0:
        return s
    prec = oracle.list_precision(s)
    e = oracle.roc_encode(s, prec)
    return oracle.roc_decode(e["head"], e["words"], s.size, prec, e["mt_draws"])[0]


class RowRef:
    """The rows a graph object of `kind` ('compact' | 'ef' | 'roc') must give back for the int32 [N, K] rows it was built from.
    The per-row answer is computed once; `expected` serves any node list and any width from it."""

    def __init__(self, kind, rows, oracle=None):
        rows = np.asarray(rows, dtype=np.int32)
        assert rows.ndim == 2 and kind in ("compact", "ef", "roc")
        self.kind, self.N, self.K = kind, rows.shape[0], rows.shape[1]
        self.table = np.full(rows.shape, -1, np.int32)
        self.counts = np.zeros(self.N, np.uint32)
        for i in range(self.N):
            ids = _row_ids(rows[i])
            if kind == "ef":
                ids = np.sort(ids)  # altid_impl.cpp:76
            elif kind == "roc":
                ids = _roc_order(ids, oracle).astype(np.int64)
            self.table[i, : ids.size] = ids
            self.counts[i] = ids.size

    def expected(self, nodes, K_out):
        """-> (int32 [m, K_out], uint32 counts[m]); nodes None = every node in order.  A node outside [0, N) gives a row of -1
        and count 0 (include/vidc.h, "Nodes")."""
        assert K_out >= self.K
        nodes = np.arange(self.N, dtype=np.int64) if nodes is None else np.asarray(nodes).astype(np.int64).reshape(-1)
        ok = (nodes >= 0) & (nodes < self.N)
        out = np.full((nodes.size, K_out), -1, np.int32)
        cnt = np.zeros(nodes.size, np.uint32)
        out[ok, : self.K] = self.table[nodes[ok]]
        cnt[ok] = self.counts[nodes[ok]]
        return out, cnt


def expected_rows(kind, rows, nodes, K_out, oracle=None):
    """int32 [m, K_out] and counts[m] that decoding `nodes` of an object built from `rows` must leave behind:
    compact: the row's ids in input order; ef: ascending; roc: oracle.roc_decode(oracle.roc_encode(sorted ids)); then -1."""
    return RowRef(kind, rows, oracle).expected(nodes, K_out)


# ------------------------------------------------------------------------------------------------------------ lists
class ListRef:
    """The ids a list object of `kind` ('packed' | 'ef' | 'wt' | 'roc') must give back, list by list, for the CSR (offsets, ids) it
    was built from: packed input order, ef / wt ascending, roc the oracle's decode order."""

    def __init__(self, kind, offsets, ids, oracle=None):
        assert kind in ("packed", "ef", "wt", "roc")
        self.offsets = np.asarray(offsets, dtype=np.uint64)
        ids = np.asarray(ids, dtype=np.uint64)
        assert self.offsets[0] == 0 and int(self.offsets[-1]) == ids.size
        self.flat = ids.copy()
        off = self.offsets.astype(np.int64)
        for l in range(off.size - 1):
            a, b = int(off[l]), int(off[l + 1])
            if kind in ("ef", "wt"):
                self.flat[a:b] = np.sort(ids[a:b])
            elif kind == "roc":
                self.flat[a:b] = _roc_order(ids[a:b], oracle)

    def expected(self, list_nos):
        """-> (uint64[total], uint64 out_offsets[m + 1]); list_nos None = every list in order"""
        off = self.offsets.astype(np.int64)
        ln = np.arange(off.size - 1, dtype=np.int64) if list_nos is None else np.asarray(list_nos).astype(np.int64).reshape(-1)
        sizes = off[ln + 1] - off[ln]
        out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        parts = [self.flat[off[l]: off[l + 1]] for l in ln]
        flat = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        return flat.astype(np.uint64), out_off

    def item(self, list_no, offset):
        """get_ids(list_no)[offset]"""
        return int(self.flat[int(self.offsets[list_no]) + int(offset)])


def expected_lists(kind, offsets, ids, list_nos, oracle=None):
    """uint64[total] and out_offsets[m + 1] that decoding `list_nos` of an object built from (offsets, ids) must leave behind"""
    return ListRef(kind, offsets, ids, oracle).expected(list_nos)


# ----------------------------------------------------------------------------------------------------------- guards
def _poison_for(np_dtype):
    np_dtype = np.dtype(np_dtype)
    if np_dtype.itemsize == 4:
        return np.array([0xA5A5A5A5], np.uint32).view(np_dtype)[0]
    assert np_dtype.itemsize == 8
    return np.array([POISON64], np.uint64).view(np_dtype)[0]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _np_dtype_of(x):
    if _is_torch(x):
        return np.dtype(str(x.dtype).split(".")[-1])
    return x.dtype


def _addr(x):
    return x.data_ptr() if _is_torch(x) else x.ctypes.data


def to_numpy(x):
    return x.cpu().numpy() if _is_torch(x) else np.asarray(x)


def guarded(shape, dtype, device="cpu", pad_elems=None, misalign_elems=0):
    """-> (whole, view).  `whole` is a 1-D buffer filled with the poison pattern of `dtype` (int32 / uint32 / int64 / uint64);
    `view` (of `shape`, contiguous) starts pad_elems + misalign_elems elements into it and is followed by at least pad_elems more.
    pad_elems defaults to GUARD_BYTES worth and is rounded up so that the guard is a multiple of 16 bytes: with the base of the
    buffer 16-byte aligned, misalign_elems alone decides the view's alignment.  device 'cpu': numpy arrays; otherwise torch tensors
    on that device (uint64 is carried as int64 there: same bytes)."""
    np_dtype = np.dtype(dtype)
    isz = np_dtype.itemsize
    per16 = 16 // isz
    pad = -(-GUARD_BYTES // isz) if pad_elems is None else int(pad_elems)
    assert pad * isz >= GUARD_BYTES, "a guard is at least 4 KiB"
    pad = -(-pad // per16) * per16
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64))
    start = pad + int(misalign_elems)
    total = start + n + pad
    poison = _poison_for(np_dtype)
    if device == "cpu":
        raw = np.empty(total + per16, np_dtype)
        skew = ((-raw.ctypes.data) % 16) // isz  # first 16-byte aligned element
        whole = raw[skew: skew + total]
        whole[:] = poison
    else:
        import torch

        tdt = {4: torch.int32, 8: torch.int64}[isz]
        whole = torch.full((total,), int(np.array([poison]).view(np.int32 if isz == 4 else np.int64)[0]), dtype=tdt, device=device)
    assert _addr(whole) % 16 == 0
    view = whole[start: start + n].reshape(shape)
    assert _addr(view) - _addr(whole) == start * isz
    return whole, view


def _split(whole, view):
    """(numpy copy of whole, start, n) of a (whole, view) pair made by `guarded`"""
    isz = _np_dtype_of(whole).itemsize
    delta = _addr(view) - _addr(whole)
    n = int(view.numel()) if _is_torch(view) else int(view.size)
    assert delta % isz == 0
    start = delta // isz
    w = to_numpy(whole).reshape(-1)
    assert 0 <= start and start + n <= w.size
    return w, start, n


def assert_guards_intact(whole, view, what=""):
    """not one element of `whole` outside `view` differs from the poison it was filled with"""
    w, start, n = _split(whole, view)
    poison = _poison_for(w.dtype)
    for name, part, base in (("before", w[:start], -start), ("behind", w[start + n:], n)):
        bad = np.flatnonzero(part != poison)
        if bad.size:
            raise AssertionError(f"{what}: stray write {name} the output: {bad.size} element(s), first at element "
                                 f"{base + int(bad[0])} relative to the view's start (value {part[bad[0]]!r})")


def assert_untouched(whole, view, what=""):
    """the call wrote nothing at all: guards and payload still hold the poison"""
    w, _, _ = _split(whole, view)
    bad = np.flatnonzero(w != _poison_for(w.dtype))
    assert bad.size == 0, f"{what}: {bad.size} element(s) changed, first at {int(bad[0])}"


def assert_view_equals(view, expected, what=""):
    """the WHOLE view equals `expected` (same number of elements; compared as the bytes of expected's dtype)"""
    got = to_numpy(view).reshape(-1)
    exp = np.ascontiguousarray(expected).reshape(-1)
    assert got.size == exp.size, f"{what}: {got.size} elements, expected {exp.size}"
    got = got.view(exp.dtype) if got.dtype != exp.dtype else got
    bad = np.flatnonzero(got != exp)
    if bad.size:
        i = int(bad[0])
        unwritten = int((got[bad] == _poison_for(exp.dtype)).sum())
        raise AssertionError(f"{what}: {bad.size} of {exp.size} elements differ ({unwritten} of them still hold the poison, i.e. "
                             f"were never written); first at flat index {i}: got {got[i]!r}, expected {exp[i]!r}")
