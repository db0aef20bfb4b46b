"""Chains of add, remove and locate on one set of lists, stated without the library (numpy only), and the designed schedules the GPU
chains (tests/test_gpu_churn.py) run.

The model is a list of uint64 arrays, one per inverted list, in the order an input-order container keeps: the old entries, then the
batch entries of that list in batch order; a removal keeps the order of the survivors (include/vidc.h, "append" and "remove").

    m = Model(lists)
    m.add(list_nos, ids)                 negative list number: skipped, not counted          -> the lists that grew
    m.remove(list_nos | None, ids)       pairs mode / any-list mode, as tests/remove_ref.py   -> Counts(removed, missing, invalid, touched)
    m.find(list_nos | None, ids)         -> the list that holds every id (-1: absent); any-list mode: the first one

code(ids) is the payload every entry carries: the little-endian bytes of id * 0x9E3779B97F4A7C15 mod 2^64, as one int64.

schedule(scheme) builds the designed chain: the initial lists and twelve steps, each an add, a remove or a query-only step, with the
arrays a caller passes.  The schemes differ in the ids alone:
    sparse   ids 6 k + 3 below 2^20 (Elias-Fano, ROC: lists the reference codec round-trips)
    dense    ids 0 .. 15 997 and two of them twice, fresh ids 16 000, 16 001, ... in batch order (packed bits: the constructor takes ids
             below ntotal, an append ids below the number ever handed out)
    perm     ids 0 .. 15 999, fresh ids continue; the removals are left out (the wavelet tree holds a permutation)
What the schedule contains is asserted, without a GPU, by tests/test_churn_ref_cpu.py.

An ordinary helper module: no torch, no oracle, nothing from the product package.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
NLIST = 16
CODE_SIZE = 8
SCHEMES = ("sparse", "dense", "perm")

# the lists of the designed object, by what the schedule does to them
L_64, L_1024, L_WIDE, L_NARROW, L_STARTS_EMPTY, L_ONE, L_REFILL, L_2048, L_PREC, L_DUP_A, L_DUP_B = range(11)
INIT_SIZES = (63, 1023, 4090, 4090, 0, 1, 300, 2040, 500, 70, 200, 1100, 900, 800, 600, 223)  # 16 000 ids
SEAMS_UP = {L_64: 2, L_1024: 2, L_WIDE: 10, L_NARROW: 10, L_2048: 20}                             # 63 -> 65, ..., 2040 -> 2060
# steps of the schedule
S_FRESH, S_SEAMS_UP, S_REMOVE_500, S_SEAMS_DOWN, S_ADD_600, S_EVERY_LIST, S_PRECISION_DOWN, S_ONE_LIST, S_EMPTY, S_REMOVE_ANY, \
    S_ADD_800, S_LAST = range(12)


def code(ids):
    """int64 array: the payload of every id"""
    x = np.ascontiguousarray(ids).reshape(-1)
    x = x.view(np.uint64) if x.dtype in (np.int64, np.uint64) else x.astype(np.uint64)
    with np.errstate(over="ignore"):
        return (x * np.uint64(GOLDEN)).view(np.int64)


# ----------------------------------------------------------------------------------------------------------------------- model
class Counts:
    def __init__(self, removed, missing, invalid, touched):
        self.removed, self.missing, self.invalid, self.touched = removed, missing, invalid, touched


class Model:
    def __init__(self, lists):
        self.lists = [np.array(li, dtype=np.uint64).reshape(-1) for li in lists]
        self.nlist = len(self.lists)

    def copy(self):
        return Model(self.lists)

    def sizes(self):
        return np.array([li.size for li in self.lists], dtype=np.int64)

    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.sizes())]).astype(np.uint64)

    def ids(self):
        return np.concatenate(self.lists) if self.nlist else np.zeros(0, np.uint64)

    @property
    def ntotal(self):
        return int(self.sizes().sum())

    def add(self, list_nos, ids):
        ln = np.asarray(list_nos, dtype=np.int64).reshape(-1)
        ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        assert ln.size == ids.size and (ln < self.nlist).all()
        touched = sorted(set(ln[ln >= 0].tolist()))
        for l in touched:
            self.lists[l] = np.concatenate([self.lists[l], ids[ln == l]])  # (boolean selection keeps the batch order)
        return touched

    def remove(self, list_nos, ids):
        ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        removed = missing = invalid = 0
        touched = []
        if list_nos is None:
            present = np.zeros(ids.size, bool)
            for l in range(self.nlist):
                present |= np.isin(ids, self.lists[l])
            missing = int((~present).sum())
            want = [ids] * self.nlist
        else:
            ln = np.asarray(list_nos, dtype=np.int64).reshape(-1)
            assert ln.size == ids.size
            invalid = int((ln >= self.nlist).sum())
            want = [ids[ln == l] for l in range(self.nlist)]
            missing = sum(int((~np.isin(want[l], self.lists[l])).sum()) for l in range(self.nlist))
        for l in range(self.nlist):
            gone = np.isin(self.lists[l], want[l])
            if gone.any():
                removed += int(gone.sum())
                touched.append(l)
                self.lists[l] = self.lists[l][~gone]
        return Counts(removed, missing, invalid, touched)

    def find(self, list_nos, ids):
        """int64[n]: the list holding ids[i] -- list_nos[i] if it does (pairs mode), the first list that does (None) --, else -1"""
        ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
        out = np.full(ids.size, -1, np.int64)
        for l in range(self.nlist - 1, -1, -1):
            hit = np.isin(ids, self.lists[l])
            if list_nos is not None:
                hit &= np.asarray(list_nos, dtype=np.int64).reshape(-1) == l
            out[hit] = l
        return out


# -------------------------------------------------------------------------------------------------------------------- schedule
class Step:
    """kind: "add" / "remove" / "query".  list_nos: int64 array, or None (a remove in any-list mode).  ids: uint64 array.  expect:
    Counts of a remove.  touched: the lists the step changes.  sizes: the list sizes behind it."""

    def __init__(self, name, kind, list_nos=None, ids=None):
        self.name, self.kind, self.list_nos, self.ids = name, kind, list_nos, ids
        self.expect, self.touched, self.sizes = None, [], None


class _Ids:
    """hands out the ids of one scheme: every one once"""

    def __init__(self, scheme, rng):
        self.scheme = scheme
        if scheme == "sparse":
            small, rest = rng.permutation(5000), 5000 + rng.permutation(16000)
            self.small = small[:499]                                          # L_PREC: ids below 2^15 ...
            self.pool = rng.permutation(np.concatenate([small[499:], rest]))  # every other list: below 2^17
            self.wide = 50_000 + rng.choice(120_000, 4090, replace=False)     # L_WIDE: 19 - 20 bits
            self.next_k, self.next_wide_k, self.next_high_k = 21_000, 170_000, 45_000
        else:
            self.next = 16_000

    @staticmethod
    def spread(k):
        """k -> 6 k + 3: odd multiples of three, so no list's largest id is a power of two"""
        return (6 * np.asarray(k, dtype=np.uint64) + 3).astype(np.uint64)

    def initial(self, rng, dups):
        own = np.array(INIT_SIZES, dtype=np.int64)
        if dups:
            own[L_DUP_B] -= 2
        if self.scheme == "sparse":
            lists, at = [], 0
            for l, n in enumerate(own):
                if l == L_WIDE:
                    lists.append(self.spread(self.wide))
                elif l == L_PREC:
                    lists.append(self.spread(np.concatenate([self.small, [131_077]])))  # ... and one of 20 bits
                else:
                    lists.append(self.spread(self.pool[at:at + n]))
                    at += n
        else:  # ids in add order: ascending inside every list
            lst = np.repeat(np.arange(NLIST), own)
            rng.shuffle(lst)
            order = np.argsort(lst, kind="stable").astype(np.uint64)
            off = np.concatenate([[0], np.cumsum(own)])
            lists = [order[off[l]:off[l + 1]] for l in range(NLIST)]
        if dups:  # two ids of L_DUP_A stand in L_DUP_B as well
            a, b = lists[L_DUP_A], lists[L_DUP_B]
            lists[L_DUP_B] = np.concatenate([[a[10]], b[:149], [a[40]], b[149:]]).astype(np.uint64)
        return lists

    def fresh(self, list_nos, high=False):
        """the ids of a batch, in batch order (the id of a skipped pair is never looked at)"""
        ln = np.asarray(list_nos, dtype=np.int64)
        out = np.zeros(ln.size, np.uint64)
        for i, l in enumerate(ln):
            if self.scheme != "sparse":
                out[i] = self.next
                self.next += int(l >= 0)
            elif l == L_WIDE:
                out[i] = 6 * self.next_wide_k + 3
                self.next_wide_k += 1
            elif high:
                out[i] = 6 * self.next_high_k + 3
                self.next_high_k += 1
            else:
                out[i] = 6 * self.next_k + 3
                self.next_k += 1
        return out

    def absent(self, n, salt):
        """ids no list ever holds: 6 k + 4, or above everything the chain hands out"""
        j = np.arange(n, dtype=np.uint64) + np.uint64(1000 * salt)
        return (6 * j + 4).astype(np.uint64) if self.scheme == "sparse" else (np.uint64(20_000) + j).astype(np.uint64)


def _batch(rng, counts, negatives=0):
    ln = np.concatenate([np.full(n, l, np.int64) for l, n in counts.items()] + [-1 - np.arange(negatives, dtype=np.int64)])
    return ln[rng.permutation(ln.size)] if ln.size else ln


def _pairs(rng, pairs):
    ln = np.array([p[0] for p in pairs], dtype=np.int64)
    ids = np.array([p[1] for p in pairs], dtype=np.uint64)
    order = rng.permutation(ln.size)
    return ln[order], ids[order]


def schedule(scheme):
    """-> (initial lists, steps).  The steps carry their expected counts, touched lists and list sizes (Model applied in order)."""
    assert scheme in SCHEMES
    rng = np.random.default_rng([20261021, SCHEMES.index(scheme)])  # (fixed: the order inside a batch, nothing the design rests on)
    src = _Ids(scheme, rng)
    init = src.initial(rng, dups=scheme != "perm")
    m = Model(init)
    steps = []

    def add(name, counts, negatives=0, high=False):
        ln = _batch(rng, counts, negatives)
        st = Step(name, "add", ln, src.fresh(ln, high))
        st.touched = m.add(st.list_nos, st.ids)
        st.sizes = m.sizes()
        steps.append(st)

    def remove(name, ln, ids):
        if scheme == "perm":  # add-only: the removals fall away
            return
        st = Step(name, "remove", ln, ids)
        st.expect = m.remove(ln, ids)
        st.touched = st.expect.touched
        st.sizes = m.sizes()
        steps.append(st)

    def query(name):
        st = Step(name, "query")
        st.sizes = m.sizes()
        steps.append(st)

    L = m.lists
    query("fresh")
    add("seams_up", SEAMS_UP, negatives=3)
    # 500 leave by pair, the only id of L_ONE among them; around them every kind of pair that is skipped
    pairs = [(11, L[11][5 * i]) for i in range(200)] + [(12, L[12][6 * i]) for i in range(150)] + [(13, L[13][5 * i + 1]) for i in range(149)]
    pairs += [(L_ONE, L[L_ONE][0])]
    a1, a2 = src.absent(2, 1)
    pairs += [(-1, L[11][1]), (-7, a1), (11, a2), (12, L[11][3]), (11, L[11][0])]  # negative x 2, absent, wrong list, repeated
    remove("remove_500", *_pairs(rng, pairs))
    # the seams downwards, old and new entries alike; L_REFILL emptied; the first duplicate leaves both its lists
    gone = [L[L_64][[0, 64]], L[L_1024][[5, 1023]], L[L_WIDE][np.r_[5:4090:455, 4095]], L[L_NARROW][np.r_[5:4090:455, 4095]], L[L_2048][np.r_[0:2060:115, 2041, 2059]], L[L_REFILL],
            L[L_DUP_A][[10]], src.absent(1, 2)]
    gone = np.concatenate(gone).astype(np.uint64)
    remove("seams_down", None, gone[rng.permutation(gone.size)])
    add("add_600", {L_STARTS_EMPTY: 50, 14: 250, 15: 300})
    add("every_list", {l: 300 if l == L_REFILL else 3 + l for l in range(NLIST)})
    # the largest id of L_PREC leaves; the second duplicate leaves L_DUP_A alone
    top = L[L_PREC].max()
    dup2 = init[L_DUP_A][40]
    a1, a2 = src.absent(2, 3)
    pairs = [(L_PREC, top), (L_DUP_A, dup2)] + [(14, L[14][3 * i]) for i in range(100)]
    pairs += [(-2, L[14][1]), (14, a1), (-1, a2), (13, L[14][4]), (14, L[14][0]), (L_PREC, top)]
    remove("precision_down", *_pairs(rng, pairs))
    add("one_list", {L_PREC: 40}, high=True)
    add("empty", {})
    gone = np.concatenate([li[::20] for li in L] + [src.absent(5, 4), L[11][:1]]).astype(np.uint64)
    remove("remove_any", None, gone[rng.permutation(gone.size)])
    add("add_800", {l: 50 for l in range(NLIST)}, negatives=3)
    query("last")
    return init, steps


def never(scheme, n):
    """n ids no step of the schedule ever hands out"""
    j = np.arange(n, dtype=np.uint64)
    return (6 * (np.uint64(300_000) + j) + 4).astype(np.uint64) if scheme == "sparse" else (np.uint64(30_000) + j).astype(np.uint64)


def positions(li, ids):
    """the first position of every id in the list `li` (all of them are in it)"""
    li, ids = np.asarray(li, dtype=np.uint64), np.asarray(ids, dtype=np.uint64)
    order = np.argsort(li, kind="stable")
    at = order[np.searchsorted(li[order], ids, side="left")]
    assert np.array_equal(li[at], ids)
    return at.astype(np.int64)
