"""The member-row geometry of the ROC decoders in numpy, and id families that load a bucket's row to exactly its capacity or to one id
beyond it.  A plain restatement of csrc/roc_sizing.h and of b2_buckets_for (csrc/roc_dec_plan.h) with no GPU in it: the tool that
places ids on the edge (tests/test_gpu_roc_member_rows.py), checked against the headers by tests/test_roc_rows_ref_cpu.py.  It is
not the correctness reference of anything it helps to test: that stays oracle.pyoracle.Oracle.

Every bucket-row decoder finds the rank of a decoded id x in member rows: x >> (P - bits) picks one of 2^bits buckets, the bucket's
earlier members sit in a row of `cap` slots.  A list is handed back (VIDC_ST_RETRY) if and only if one of its buckets would take
member cap + 1; the general decoder spills that member into an overflow list instead."""
import numpy as np

# the limits of the planner that no sizing header holds, as literals
R2_MIN_LIST = 256        # csrc/roc.hip:89   constexpr uint64_t R2_MIN_LIST = 256
B2L_CAP = 64             # csrc/roc_u2.h:1708 #define VIDC_B2L_CAP 64u
B2L_MAX_LIST = 4096      # csrc/roc_u2.h:1709 #define VIDC_B2L_MAX_LIST 4096u
B2L_MID_LIST = 2048      # csrc/roc_u2.h:1710 #define VIDC_B2L_MID_LIST 2048u
B2L_LOAD = 30            # csrc/roc_u2.h:1711 #define VIDC_B2L_LOAD 30u

KINDS = ("lane64", "lane128", "lane256", "grp", "b2", "b2l32", "b2l64", "b2l128", "b2l256", "gen")


# ---- csrc/roc_sizing.h
def lane_cap(nb, n, align=16):
    """roc_lane_cap_nb<NB>(n, align): twice the mean + 16, a multiple of 4, padded to `align` slots above align 4"""
    cap = ((n // nb) * 2 + 16 + 3) & ~3
    return (cap + align - 1) & ~(align - 1) if align > 4 else cap


def grp_fbits(n):
    """roc_grp_dec_fbits"""
    return 0 if n <= 2048 else (2 if n <= 8192 else (3 if n <= 16384 else 4))


def grp_cap(n):
    """roc_grp_dec_cap"""
    return 32 if n <= 32768 else (64 if n <= 65536 else 96)


def gen_cap(n):
    """roc_dec_cap"""
    return 64 if n > 32768 else 16


def gen_fine_bits(n, P):
    """roc_dec_fine_bits: lg(n) - 3, at most 12 and at most P"""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    return min(max(lg - 3, 0), 12, P)


def geometry(kind, n, P, align=16):
    """-> (bucket bits, members a bucket's row holds) of the decoder `kind` for a list of n ids with precision P"""
    if kind in ("lane64", "lane128", "lane256"):
        nb = int(kind[4:])
        return nb.bit_length() - 1, lane_cap(nb, n, align)
    if kind == "grp":
        return 8 + grp_fbits(n), grp_cap(n)
    if kind == "b2":
        return 12, 64
    if kind in ("b2l32", "b2l64", "b2l128", "b2l256"):
        return int(kind[3:]).bit_length() - 1, B2L_CAP
    if kind == "gen":
        return gen_fine_bits(n, min(P, 32)), gen_cap(n)
    raise ValueError(kind)


def b2l_buckets(n, P, umax):
    """b2_buckets_for (csrc/roc_dec_plan.h): the bucket count of k_roc_decode_b2<32 .. 256> for a short list, or 0.  umax = 0: the
    maximum is unknown (imported streams), half of the buckets are assumed to be in use."""
    if n <= R2_MIN_LIST or n > B2L_MAX_LIST or P > 31:
        return 0
    for bk in (32, 64, 128, 256):
        bbits = bk.bit_length() - 1
        bsh = P - bbits if P > bbits else 0
        mx = umax if umax else ((1 << (P - 1)) if P else 1)
        eff = min(bk, (mx >> bsh) + 1)
        if n <= B2L_LOAD * eff:
            return bk
    return 0


# ---- loads
def loads(ids, P, bits):
    """members per bucket, 2^bits of them (P > bits)"""
    assert P > bits
    b = (np.asarray(ids, dtype=np.uint64) >> np.uint64(P - bits)).astype(np.int64)
    return np.bincount(b, minlength=1 << bits)


def handed_back(ids, P, bits, cap):
    """a load of exactly cap is not handed back"""
    return bool(loads(ids, P, bits).max() > cap)


# ---- families: n distinct ascending ids with maximum 2^P - 1 (the reference precision is P, the top bucket has a member)
def _bucket_loads(n, nb, cap, where=None):
    """Loads of the family.  One id -- the maximum -- is set aside for the top bucket first.  The buckets are then filled in order
    of priority until n ids are placed: bucket 0, the top bucket, buckets 1, 2, ... (`packed`: the last one reached takes the
    remainder); the bucket that goes one over comes first, and for "middle" (bucket 1) its neighbours 0 and 2 come next."""
    top = nb - 1
    order = {None: [0, top], "first": [0, top], "top": [top, 0], "middle": [1, 0, 2, top]}[where]
    target = {None: -1, "first": 0, "top": top, "middle": 1}[where]
    order = order + [b for b in range(1, top) if b not in order]
    ld = np.zeros(nb, np.int64)
    ld[top] = 1
    left = n - 1
    for b in order:
        take = min((cap + 1 if b == target else cap) - ld[b], left)
        ld[b] += take
        left -= take
        if left == 0:
            break
    if left or (where is not None and ld[target] != cap + 1):
        raise ValueError(f"n={n} does not fit {nb} buckets of {cap} members ({where})")
    return ld


def _draw(rng, ld, P, bits):
    w = 1 << (P - bits)
    if int(ld.max()) > w:
        raise ValueError(f"a bucket of {w} ids cannot hold {int(ld.max())} members")
    top = ld.size - 1
    parts = []
    for b in np.flatnonzero(ld):
        k = int(ld[b])
        if b == top:  # the maximum id and k - 1 others
            v = np.concatenate([rng.choice(w - 1, size=k - 1, replace=False), [w - 1]])
        else:
            v = rng.choice(w, size=k, replace=False)
        parts.append(np.sort(v).astype(np.uint64) + np.uint64(int(b) * w))
    return np.concatenate(parts)


def packed(rng, n, P, bits, cap):
    """ceil(n / cap) buckets filled to exactly cap, the last one with the remainder: bucket 0, the top bucket and a run of adjacent
    buckets from 1 upward; ids random inside a bucket"""
    return _draw(rng, _bucket_loads(n, 1 << bits, cap), P, bits)


def one_over(rng, n, P, bits, cap, where):
    """`packed` with one bucket at cap + 1: where = "first" (bucket 0), "top" or "middle" (bucket 1).  The neighbours 0 and 2 of the
    middle bucket are full where n allows it (middle_is_flanked): two full neighbours and the maximum take 3 * cap + 2 ids."""
    return _draw(rng, _bucket_loads(n, 1 << bits, cap, where), P, bits)


def over_bucket(where, bits):
    return {"first": 0, "top": (1 << bits) - 1, "middle": 1}[where]


def middle_is_flanked(n, cap):
    return n >= 3 * cap + 2


def single_bucket(rng, n, P, bits):
    """every id but the maximum in bucket 0 (general decoder: an overflow list of n - 1 - cap entries)"""
    w = 1 << (P - bits)
    if n - 1 > w or bits < 1:
        raise ValueError("bucket too narrow")
    return np.concatenate([np.sort(rng.choice(w, size=n - 1, replace=False)), [(1 << P) - 1]]).astype(np.uint64)


def same_bucket_pairs(order, P, bits, block=64):
    """pairs of steps inside one `block`-step decode block whose ids fall into the same bucket (order: ids in decoding order)"""
    b = (np.asarray(order, dtype=np.uint64) >> np.uint64(P - bits)).astype(np.int64)
    total = 0
    for s in range(0, b.size, block):
        c = np.bincount(b[s:s + block])
        total += int((c * (c - 1) // 2).sum())
    return total


# ---- the calls of tests/test_gpu_roc_member_rows.py (checked on the CPU by tests/test_roc_rows_ref_cpu.py)
LAYOUT = ("top", None, "middle", None, "first")  # one_over / packed in this order, then a uniformly random list


def layout_lists(rng, kind, n, P, align=16):
    """The six lists of one (geometry, n): one_over(top), packed, one_over(middle), packed, one_over(first), a random list -- a clean
    list's rows lie right behind an overflowing top row in the slot arena.  -> [(ids, where or "packed" or "random")]"""
    bits, cap = geometry(kind, n, P, align)
    out = []
    for where in LAYOUT:
        out.append((packed(rng, n, P, bits, cap), "packed") if where is None else (one_over(rng, n, P, bits, cap, where), where))
    body = np.sort(rng.choice((1 << P) - 1, size=n - 1, replace=False)).astype(np.uint64)
    out.append((np.concatenate([body, [(1 << P) - 1]]).astype(np.uint64), "random"))
    return out


def lane_kind(n, no_lane128=False):
    return "lane64" if n <= 1024 else ("lane128" if n <= 2048 and not no_lane128 else "lane256")


def _case(name, hooks, groups, expect_kind=True, **kw):
    """groups: [(kind, n, P, align)], each the six lists of layout_lists; expect_kind: the lists that go one over are handed back"""
    return dict(name=name, hooks=hooks, groups=groups, hands_back=expect_kind, **kw)


def gpu_cases():
    cases = []
    # lane bucket rows, 64 buckets: ragged sizes in one wavefront
    for P in (20, 31):
        for align in (16, 4):
            for loop in (0, 1):
                hooks = {"VIDC_FORCE_LANE": "1", "VIDC_NO_LANE_REG": "1", "VIDC_NO_LANE_PAIR": "1", "VIDC_LANE_ALIGN": str(align)}
                if loop:
                    hooks["VIDC_LANE_LOOP"] = "1"
                cases.append(_case(f"lane64-P{P}-align{align}" + ("-loop" if loop else ""), hooks,
                                   [("lane64", n, P, align) for n in (65, 513, 700, 1024)]))
    # 128 and 256 buckets
    for P, align, no128, loop in [(P, a, k, 0) for P in (20, 31) for a in (16, 4) for k in (0, 1)] + [(31, 16, 1, 1), (20, 4, 0, 1)]:
        hooks = {"VIDC_FORCE_LANE": "1", "VIDC_LANE_ALIGN": str(align)}
        if no128:
            hooks["VIDC_NO_LANE128"] = "1"
        if loop:
            hooks["VIDC_LANE_LOOP"] = "1"
        cases.append(_case(f"lane128+256-P{P}-align{align}" + ("-no128" if no128 else "") + ("-loop" if loop else ""), hooks,
                           [(lane_kind(n, bool(no128)), n, P, align) for n in (1025, 1500, 2048, 2049, 3000, 4096)]))
    # row-per-list
    for n, P in [(65, 24), (2048, 24), (2049, 24), (8192, 24), (8193, 24), (8193, 31), (16385, 24), (32769, 24)]:
        cases.append(_case(f"grp-n{n}-P{P}", {"VIDC_FORCE_GRP": "1"}, [("grp", n, P, 16)]))
    cases.append(_case("grp-n65537-P24", {"VIDC_FORCE_GRP": "1"}, [("grp", 65537, 24, 16)], beyond_reference=True))
    # k_roc_decode_b2, rows in memory
    for n in (4097, 9000):
        for P in (21, 24, 27, 28, 31):
            for mask in (0, 1):
                cases.append(_case(f"b2-n{n}-P{P}-mask{mask}", {"VIDC_B2_MASK": str(mask)}, [("b2", n, P, 16)]))
    # k_roc_decode_b2<32 .. 256>, rows in LDS; imported without maxima the planner assumes half of the buckets
    for bk in (32, 64, 128, 256):
        for P in (20, 31):
            n = {32: 960, 64: 1920, 128: 3840, 256: 4096}[bk]
            assert b2l_buckets(n, P, (1 << P) - 1) == bk
            cases.append(_case(f"b2l{bk}-n{n}-P{P}", {}, [(f"b2l{bk}", n, P, 16)]))
            n = B2L_LOAD * (bk // 2 + 1)
            assert b2l_buckets(n, P, 0) == bk and b2l_buckets(n + 1, P, 0) != bk
            cases.append(_case(f"b2l{bk}-imported-n{n}-P{P}", {}, [(f"b2l{bk}", n, P, 16)], imported=True))
    # general decoder: an overflow entry per list that goes one over, nothing handed back
    for n in (65, 4096, 4097, 32769):
        for P in (24, 31):
            cases.append(_case(f"gen-n{n}-P{P}", {"VIDC_FORCE_GENERAL": "1"}, [("gen", n, P, 16)], expect_kind=False))
    return cases


def case_lists(case, seed=None):
    """-> ([ids], [tag], [(kind, n, P, align)] per list) of a case, deterministic in its name"""
    rng = np.random.default_rng(seed if seed is not None else [ord(c) for c in case["name"]])
    lists, tags, geo = [], [], []
    for g in case["groups"]:
        for ids, tag in layout_lists(rng, *g):
            lists.append(ids)
            tags.append(tag)
            geo.append(g)
    return lists, tags, geo


def model_handed_back(lists, geo):
    """which lists the bucket-row decoder of their geometry hands back"""
    return [handed_back(li, g[2], *geometry(g[0], g[1], g[2], g[3])) for li, g in zip(lists, geo)]


def geometry_table():
    """(n, P, umax, align) of every list of every case, with the unknown maximum of imported streams, plus the class boundaries"""
    rows = set()
    for c in gpu_cases():
        for kind, n, P, align in c["groups"]:
            rows.add((n, P, (1 << P) - 1, align))
            rows.add((n, P, 0, align))
    for n in (64, 65, 256, 257, 300, 510, 511, 960, 961, 990, 991, 1024, 1025, 1920, 1921, 1950, 1951, 2048, 2049, 3840, 3841, 3870, 3871, 4096,
              4097, 8192, 8193, 16384, 16385, 32768, 32769, 65536, 65537, 98304):
        for P in (3, 8, 12, 13, 20, 24, 31, 32):
            for umax in (0, (1 << P) - 1, (1 << P) // 3):
                for align in (4, 16):
                    rows.add((n, P, umax, align))
    return sorted(rows)
