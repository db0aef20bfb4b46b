"""Lists that drive the ANS word stacks of the ROC kernels through their cold paths -- underflow (mt19937 draws) up to the edge of the
1024-word table, the decoders' own pushes at and beyond the depth their LDS stacks hold, streams that grow while they are decoded
-- and what the library must produce for every one of them, from the CPU oracle alone.  Plain Python with no GPU in it, in the manner
of tests/roc_rows_ref.py: tests/test_gpu_roc_stack.py runs the cases, tests/test_roc_stack_ref_cpu.py pins what they rest on.

The regime.  An encode step pops log2(n - i) bits and pushes P (the precision), so a list whose precision is far below log2(n) pops
from an empty stack early on: every such pop takes the next word of mt19937(1234) (codec.h:32-40).  The decoder pushes those bits
back, so the stream GROWS while it is decoded, by about as many words as the encoder drew; with the ids cut to P bits the decoder sees
a multiset, and the list is no longer lossless.  The library reproduces the reference up to 1024 draws per list and refuses the list
beyond (include/vidc.h: VIDC_ERR_OVERFLOW).  The regime is reached by an explicit precision_mode, by duplicate-heavy lists under the
natural precision, and by any imported (P, n).

Lists are SEARCHED: for a fixed (P, universe, seed) the ids are the first n of one permutation, a figure of the oracle (draws, pushed
depth, growth) is bisected on n and the neighbourhood scanned for the exact value.  A search that finds nothing raises SearchFailed.

Checked facts (tests/test_roc_stack_ref_cpu.py): every list's decode stack peaks below roc_dec_stack_cap(n, nwords) and every stream
stays below n * 37 / 32 + 8 words, so no case expects the arena-overflow status; every list that is not meant to be refused stays
within 1024 draws through its decode as well.

Pushed depth: exactly 8 and exactly 9 were found in every class asked for (lane register / pair / quad / bucket rows of 64, 128 and 256
buckets, row-per-list with F = 0, 2 and 3); no class had to settle for less.

What cannot be built: a stream that grows in k_roc_decode_u2<20> (P = 19, 20) or in k_roc_decode_b2 (P > 20).  A decode step pops P
bits and pushes log2(i + 1) < 18 (lists end at VIDC_ROC_MAX_LIST = 2^18 ids), so above P = 18 a stack never regrows and an encoder
never draws.  Those two decoders meet their draw path through truncated imports instead (truncated_cases): the stream of a natural
list with its bottom words cut off, which the decoder replaces by table words.  With a claimed mt_draws near the table's end the same
imports take the lane- and row-per-list decoders and the tiny strip to the 1024 / 1025 edge at a pushed depth of one or two -- a list
that draws that much is deeper than 8 there and reaches the edge in the retry pass, on the wave-per-list stack."""
import functools
import os
import re

import numpy as np

import roc_rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vector_db_id_compression_amd", "csrc")
RANS_L = 1 << 31


class SearchFailed(Exception):
    pass


# ---- the bounds, read from the headers
_WANTED = {
    "common.h": ("VIDC_MT_TABLE",),
    "roc.hip": ("TINY_MAX", "GEN_SMALL_MAX", "U_MIN_LIST", "R2_MIN_LIST"),
    "roc_lane.h": ("VIDC_LANE_MAX", "VIDC_LANE_MAX64", "VIDC_LANE_MAX128", "VIDC_LANE_REG_MAX", "VIDC_LANE_PAIR_MAX", "VIDC_LANE_QUAD_MAX",
                   "VIDC_DPST", "VIDC_TINY_STRIP"),
    "roc_grp.h": ("VIDC_GRP_MIN_LIST", "VIDC_GRP_MAX_LIST", "VIDC_GRP_LEV2_MAX", "VIDC_GRP_DPST"),
    "roc_enc_plan.h": ("ENC_L4_MAX", "ENC_C1_MAX", "ENC_C2_MAX"),
    "roc_dec_plan.h": ("DEC_G8K_MAX", "DEC_G16K_MAX", "DEC_GMID_MAX", "B2_MIN_LIST", "B2_MAX_LIST"),
    "../../include/vidc.h": ("VIDC_ROC_MAX_LIST",),
}


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


@functools.lru_cache(maxsize=None)
def limits():
    """name -> value of the class bounds and stack sizes, from `#define NAME expr` / `constexpr type NAME = expr` in csrc/"""
    out = {}
    for fname, names in _WANTED.items():
        path = os.path.normpath(os.path.join(CSRC, fname))
        with open(path) as f:
            text = _strip_comments(f.read())
        for name in names:
            m = re.search(r"#define\s+%s\s+([^\n]+)" % name, text) or re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
            if not m:
                raise KeyError(f"{name} not found in {path}")
            expr = re.sub(r"\b(\d+)(?:u|ull|ul)\b", r"\1", m.group(1).strip())
            out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))  # (digits, names read before, arithmetic)
    return out


def dec_stack_cap(n, nwords):
    """roc_dec_stack_cap (csrc/roc_sizing.h): the decoder's private stack scratch, in words"""
    return max(((n * 37) >> 5) + 8, nwords) + 64


def arena_words(n):
    """arena_words_for (csrc/roc.hip): the encoder's word arena of a list"""
    return n * 37 // 32 + 8


# ---- what the library must produce for one list
def natural_precision(oracle, ids):
    return oracle.list_precision(ids)


def model(oracle, ids, precision_mode=-1):
    """One list under precision_mode (-1: the reference's ceil(log2(max id)), >= 0: that precision) -> dict
         n, precision, head, words, nwords, mt_draws, perm      the stream (Oracle.roc_encode)
         enc_peak, enc_pop_run                                   the encoder's stack: peak, longest run of pops past fresh pushes
         order                                                   the oracle's decode of that stream, as the library lays it out
         end_head, end_nwords, end_draws                         the state after the decode
         growth = end_nwords - nwords, depth, peak               the decoder's stack (Oracle.roc_decode_stats)
         lossless                                                the decode is the list as a multiset
         refused                                                 the encoder draws more than VIDC_MT_TABLE words
         decode_refused                                          ... or the decode of the stream does
         clean                                                   head back at 2^31, the stack holds what the decoder drew"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    n = ids.size
    P = natural_precision(oracle, ids) if precision_mode < 0 else int(precision_mode)
    e = oracle.roc_encode(ids, P, stats=True)
    order, end_head, end_words, end_draws, ds = oracle.roc_decode_stats(e["head"], e["words"], n, P, e["mt_draws"])
    table = limits()["VIDC_MT_TABLE"]
    return dict(n=n, precision=P if n else 0, head=e["head"], words=e["words"], nwords=int(e["words"].size), mt_draws=e["mt_draws"],
                perm=e["perm"], enc_peak=e["stack"]["peak"], enc_pop_run=e["stack"]["pop_run"], order=order, end_head=end_head,
                end_nwords=int(end_words.size), end_draws=end_draws, growth=int(end_words.size) - int(e["words"].size),
                depth=ds["depth"], peak=ds["peak"], lossless=bool(np.array_equal(np.sort(order), np.sort(ids))),
                refused=e["mt_draws"] > table, decode_refused=end_draws > table,
                clean=end_head == RANS_L and int(end_words.size) == end_draws - e["mt_draws"])


def draws_of(oracle, ids, P):
    return oracle.roc_encode(ids, P)["mt_draws"]


# ---- id families
@functools.lru_cache(maxsize=None)
def _permutation(ubits, seed):
    return np.random.default_rng([ubits, seed]).permutation(1 << ubits).astype(np.uint64)


def prefix_ids(n, ubits, seed):
    """n distinct ascending ids below 2^ubits: the first n of one permutation per (ubits, seed), so that n -> ids is nested (beyond
    16 bits: a permutation of 2^16 in the top bits, random bits below)"""
    if n > (1 << min(ubits, 16)):
        raise ValueError("universe too small")
    if ubits <= 16:
        return np.sort(_permutation(ubits, seed)[:n])
    low = np.random.default_rng([ubits, seed, 1]).integers(0, 1 << (ubits - 16), 1 << 16).astype(np.uint64)
    return np.sort((_permutation(16, seed)[:n] << np.uint64(ubits - 16)) | low[:n])


@functools.lru_cache(maxsize=None)
def _values(vbits, seed, count=1 << 16):
    return np.random.default_rng([77, vbits, seed]).integers(0, 1 << vbits, count).astype(np.uint64)


def multiset_ids(n, vbits, seed):
    """n ascending ids with duplicates, drawn from [0, 2^vbits) and nested in n; one of them is the maximum 2^vbits - 1, so the
    reference precision is vbits (vbits >= 2; vbits = 1: maximum 1, precision 0)"""
    v = _values(vbits, seed)[:n].copy()
    v[0] = (1 << vbits) - 1
    return np.sort(v)


def beside(P=None, seed=7, n=100):
    """the healthy list that shares a call: n distinct ids; P given and 2^P >= 2n: ids below 2^P with the maximum 2^P - 1, so that
    the list is in the clean domain at that precision too; otherwise ids below 2^20 with the maximum 2^20 - 1 (natural precision 20)"""
    bits = P if (P is not None and (1 << P) >= 2 * n) else 20
    rng = np.random.default_rng([seed, bits])
    body = np.sort(rng.choice((1 << bits) - 1, size=n - 1, replace=False)).astype(np.uint64)
    return np.concatenate([body, [np.uint64((1 << bits) - 1)]])


# ---- search
def find_exact(figure, target, lo, hi, accept=None, window=48):
    """n in [lo, hi] with figure(n) == target (and accept(n)), or None.  figure grows with n apart from local noise: bisect for the
    first n with figure(n) >= target, then scan `window` values on either side, nearest first."""
    if figure(hi) < target or figure(lo) > target:
        return None
    a, b = lo, hi
    while a < b:
        mid = (a + b) // 2
        if figure(mid) >= target:
            b = mid
        else:
            a = mid + 1
    for d in range(window + 1):
        for n in ((a + d, a - d) if d else (a,)):
            if lo <= n <= hi and figure(n) == target and (accept is None or accept(n)):
                return n
    return None


def _memo(f):
    cache = {}

    def g(n):
        if n not in cache:
            cache[n] = f(n)
        return cache[n]
    return g


def find_draws(oracle, P, target, lo, hi, ubits, seeds=range(6), decodable=True):
    """distinct ids below 2^ubits, lo <= n <= hi, whose encode at precision P draws exactly `target` words; decodable: the decode of
    the stream stays within the table too"""
    table = limits()["VIDC_MT_TABLE"]
    for seed in seeds:
        fig = _memo(lambda n: draws_of(oracle, prefix_ids(n, ubits, seed), P))
        ok = (lambda n: model(oracle, prefix_ids(n, ubits, seed), P)["end_draws"] <= table) if decodable and target <= table else None
        n = find_exact(fig, target, lo, hi, ok)
        if n is not None:
            return prefix_ids(n, ubits, seed)
    raise SearchFailed(f"no list of {lo}..{hi} ids below 2^{ubits} draws exactly {target} words at P={P}")


# ---- cases: name -> dict(lists=[ids], precision_mode, tags=[str], ...); the expectations come from expect()
def _call(lists, precision_mode, tags, **kw):
    assert len(lists) == len(tags)
    return dict(lists=[np.ascontiguousarray(li, dtype=np.uint64) for li in lists], precision_mode=precision_mode, tags=list(tags), **kw)


def expect(oracle, call):
    """[model(list)] of a call"""
    return [model(oracle, li, call["precision_mode"]) for li in call["lists"]]


def concat(lists):
    off = np.concatenate([[0], np.cumsum([li.size for li in lists])]).astype(np.uint64)
    return off, (np.concatenate(lists) if lists else np.zeros(0, np.uint64))


# -- the table edge
def edge_classes(oracle):
    """class -> (P, ubits, lo, hi): where a list of the class crosses 1024 draws.  lane64 / C1: up to lane_max64 = ENC_C1_MAX ids
    (P = 0); C2 / G2: up to ENC_C2_MAX / VIDC_GRP_LEV2_MAX; r2: ids of 24 bits, which the universe-bitmap encoders do not take, so the
    position-bitmap chain encoder does (the others, ids below 2^13, go to k_roc_encode_u2 in the automatic mode, which hands a list
    whose ids do not fit P to the general encoder); G3: beyond VIDC_GRP_LEV2_MAX; C3: beyond ENC_C2_MAX.  P of the longer classes is
    the largest precision at which the class still crosses the edge below `hi`, so that n stays small."""
    L = limits()
    out = {"lane64": (0, 13, L["VIDC_LANE_MAX"] + 1, L["VIDC_LANE_MAX64"]),
           "C1": (0, 14, L["VIDC_LANE_MAX"] + 1, L["ENC_C1_MAX"]),
           "C2": (4, 13, L["ENC_C1_MAX"] + 1, min(L["VIDC_GRP_LEV2_MAX"], L["ENC_C2_MAX"])),
           "r2": (4, 24, L["U_MIN_LIST"], min(L["VIDC_GRP_LEV2_MAX"], L["ENC_C2_MAX"]))}
    table = L["VIDC_MT_TABLE"]
    for name, lo, hi in (("G3", L["VIDC_GRP_LEV2_MAX"] + 1, 12000), ("C3", L["ENC_C2_MAX"] + 1, 40000)):
        for P in range(15, -1, -1):
            if draws_of(oracle, prefix_ids(hi, 16, 0), P) > table + 8 and draws_of(oracle, prefix_ids(lo, 16, 0), P) < table - 8:
                out[name] = (P, 16, lo, hi)
                break
        else:
            raise SearchFailed(f"no precision puts the table edge between {lo} and {hi} ids")
    return out


EDGE_DRAWS = (1023, 1024, 1025)
DECODE_OVER = ("C2", "G3")  # classes with a list that encodes with 1024 draws and whose DECODE draws the 1025th word


@functools.lru_cache(maxsize=None)
def _edge_lists(oracle):
    return {(cls, d): (find_draws(oracle, P, d, lo, hi, ubits), P)
            for cls, (P, ubits, lo, hi) in edge_classes(oracle).items() for d in EDGE_DRAWS}


def edge_cases(oracle):
    """per class three calls at the class's precision: `ok` = the 1023- and the 1024-draw list and a healthy list; `over` = the
    1025-draw list alone; `over+` = healthy list, 1025-draw list, the 1024-draw list (the call must fail all the same);
    `decode-over` (classes DECODE_OVER) = a list that encodes with exactly 1024 draws and whose decode -- which at these
    precisions ends with one more pop from the empty stack -- needs the 1025th word: the encode succeeds, every decode is refused"""
    out = {}
    el = _edge_lists(oracle)
    for cls in edge_classes(oracle):
        (l23, P), (l24, _), (l25, _) = (el[(cls, d)] for d in EDGE_DRAWS)
        out[f"edge-{cls}-ok"] = _call([l23, beside(P), l24], P, ["draws1023", "beside", "draws1024"], cls=cls)
        out[f"edge-{cls}-over"] = _call([l25], P, ["draws1025"], cls=cls, fails=0)
        out[f"edge-{cls}-over+"] = _call([beside(P), l25, l24], P, ["beside", "draws1025", "draws1024"], cls=cls, fails=1)
    for cls in DECODE_OVER:
        P, ubits, lo, hi = edge_classes(oracle)[cls]
        table = limits()["VIDC_MT_TABLE"]
        fig = _memo(lambda n: draws_of(oracle, prefix_ids(n, ubits, 0), P))
        n = find_exact(fig, table, lo, hi, lambda n: model(oracle, prefix_ids(n, ubits, 0), P)["end_draws"] == table + 1)
        if n is None:
            raise SearchFailed(f"{cls}: no list encodes with {table} draws and draws once more in its decode")
        out[f"edge-{cls}-decode-over"] = _call([beside(P), prefix_ids(n, ubits, 0)], P, ["beside", "decode1025"], cls=cls, decode_fails=1)
    return out


# -- partial underflow in the short classes
def class_bounds():
    """both ends of every encoder and decoder class below the edge: (bound, bound + 1) of tiny_max, ENC_L4_MAX / lane_reg_max,
    lane_pair_max, lane_max (= lane_quad_max), lane_max128, and -- with a precision of their own -- gen_small_max (= lane_max64 =
    ENC_C1_MAX = U_MIN_LIST - 1), DEC_G8K_MAX (= VIDC_GRP_LEV2_MAX), DEC_G16K_MAX"""
    L = limits()
    short = sorted({L["TINY_MAX"], L["ENC_L4_MAX"], L["VIDC_LANE_REG_MAX"], L["R2_MIN_LIST"], L["VIDC_LANE_PAIR_MAX"], L["VIDC_LANE_MAX"],
                    L["VIDC_LANE_QUAD_MAX"], L["VIDC_LANE_MAX128"]})
    longer = sorted({L["GEN_SMALL_MAX"], L["VIDC_LANE_MAX64"], L["ENC_C1_MAX"], L["U_MIN_LIST"] - 1, L["DEC_G8K_MAX"], L["VIDC_GRP_LEV2_MAX"],
                     L["DEC_G16K_MAX"]})
    return short, longer


def partial_cases(oracle):
    """`partial-short-P0` / `-P3`: lists of 1, bound - 1, bound and bound + 1 ids for every short bound in one call (P = 0: every
    pop of the encoder is a draw, the stream is empty).  `partial-long-n<bound>`: bound and bound + 1 ids at the two lowest
    precisions that keep bound + 1 ids 40 draws or more below the edge."""
    short, longer = class_bounds()
    table = limits()["VIDC_MT_TABLE"]
    out = {}
    sizes = sorted({1} | {b + d for b in short for d in (-1, 0, 1)})
    for P in (0, 3):
        lists = [prefix_ids(n, 13, 20 + i) for i, n in enumerate(sizes)]
        out[f"partial-short-P{P}"] = _call(lists + [beside(P)], P, [f"n{n}" for n in sizes] + ["beside"])
    for b in longer:
        Ps = [P for P in range(0, 16) if draws_of(oracle, prefix_ids(b + 1, 15, 3), P) <= table - 40][:2]
        if len(Ps) < 2:
            raise SearchFailed(f"no precision keeps {b + 1} ids below the edge")
        for P in Ps:
            out[f"partial-long-n{b}-P{P}"] = _call([prefix_ids(b, 15, 3), beside(P), prefix_ids(b + 1, 15, 4)], P, [f"n{b}", "beside", f"n{b + 1}"])
    return out


# -- pushed depth
def depth_classes():
    """class -> (lo, hi, decoder kinds of tests/roc_rows_ref.py whose member rows the list must not overflow)"""
    L = limits()
    return {"reg": (L["TINY_MAX"] + 1, L["VIDC_LANE_REG_MAX"], ("lane64", "grp")),
            "pair": (L["VIDC_LANE_REG_MAX"] + 1, L["VIDC_LANE_PAIR_MAX"], ("lane64", "grp")),
            "quad": (L["VIDC_LANE_PAIR_MAX"] + 1, L["VIDC_LANE_QUAD_MAX"], ("lane64", "grp")),
            "rows128": (L["VIDC_LANE_MAX"] + 1, L["VIDC_LANE_MAX128"], ("lane128", "lane256", "grp")),
            "rows256": (L["VIDC_LANE_MAX128"] + 1, L["VIDC_LANE_MAX64"], ("lane256", "grp")),
            "grpF2": (L["VIDC_LANE_MAX64"] + 1, 8192, ("grp",)),
            "grpF3": (8193, 16384, ("grp",))}


def row_loads_max(values, P, bits):
    """the fullest member row when `values` (what a decoder sees) are spread over 2^bits buckets by their top bits"""
    sh = max(P - bits, 0)
    return int(np.bincount((np.asarray(values, dtype=np.uint64) >> np.uint64(sh)).astype(np.int64)).max())


def overflows_a_row(m, kinds, aligns=(4, 16)):
    """some bucket-row decoder of `kinds` would hand the list back for a full member row, whatever its pushed depth"""
    for kind in kinds:
        for align in aligns:
            bits, cap = rr.geometry(kind, m["n"], m["precision"], align)
            if row_loads_max(m["order"], m["precision"], bits) > cap:
                return True
    return False


DEPTHS = (8, 9)


@functools.lru_cache(maxsize=None)
def _depth_lists(oracle):
    """multisets under their natural precision (duplicates of ids below 2^P: the only way to a precision far below log2(n) without
    naming one) whose decode reaches a pushed depth of exactly 8 and exactly 9, that draw less than the table holds, and that
    overflow no member row of the decoders that can take them"""
    L = limits()
    assert L["VIDC_DPST"] == DEPTHS[0] and L["VIDC_GRP_DPST"] == DEPTHS[0]
    out = {}
    for cls, (lo, hi, kinds) in depth_classes().items():
        for depth in DEPTHS:
            found = None
            for vbits in range(15, 1, -1):
                for seed in range(4):
                    mk = (lambda n, vbits=vbits, seed=seed: multiset_ids(n, vbits, seed))
                    md = _memo(lambda n: model(oracle, mk(n), -1))
                    n = find_exact(lambda n: md(n)["depth"], depth, lo, hi,
                                   lambda n: not md(n)["refused"] and not md(n)["decode_refused"] and not overflows_a_row(md(n), kinds), window=24)
                    if n is not None:
                        found = mk(n)
                        break
                if found is not None:
                    break
            if found is None:
                raise SearchFailed(f"no multiset of {lo}..{hi} ids reaches a pushed depth of exactly {depth}")
            out[(cls, depth)] = found
    return out


def depth_cases(oracle):
    """`depth-lane`: the depth-8 and depth-9 lists of the five lane classes and a natural list of 100 ids in one call; `depth-grp`:
    the same for the row-per-list geometries (the lane lists again -- F = 0 up to 2048 ids, F = 2 beyond -- and the two longer
    classes).  precision_mode -1: every list has its own precision."""
    dl = _depth_lists(oracle)
    out = {}
    for name, classes in (("depth-lane", ("reg", "pair", "quad", "rows128", "rows256")),
                          ("depth-grp", ("reg", "quad", "rows128", "rows256", "grpF2", "grpF3"))):
        lists, tags = [], []
        for cls in classes:
            for d in DEPTHS:
                lists.append(dl[(cls, d)])
                tags.append(f"{cls}-depth{d}")
        k = len(lists) // 2
        out[name] = _call(lists[:k] + [beside()] + lists[k:], -1, tags[:k] + ["beside"] + tags[k:])
    return out


# -- regrowth in the wave-per-list decoders
REGROW_RESIDUES = (0, 1, 31, 32, 33)


def _find_growth(oracle, Ps, lo, hi, gmin, gmax, ubits=15, seed=5):
    """distinct ids below 2^ubits, lo <= n <= hi, whose stream at one of the precisions Ps grows by gmin .. gmax words while it is
    decoded, inside the table through the decode -> (ids, P)"""
    for P in Ps:
        md = _memo(lambda n: model(oracle, prefix_ids(n, ubits, seed), P))
        if md(hi)["growth"] < gmin or md(lo)["growth"] > gmax:
            continue
        a, b = lo, hi
        while a < b:
            mid = (a + b) // 2
            if md(mid)["growth"] >= gmin:
                b = mid
            else:
                a = mid + 1
        for n in range(a, min(a + 32, hi) + 1):
            m = md(n)
            if gmin <= m["growth"] <= gmax and not m["refused"] and not m["decode_refused"]:
                return prefix_ids(n, ubits, seed), P
    raise SearchFailed(f"no stream of {lo}..{hi} ids grows by {gmin}..{gmax} words at P in {Ps}")


@functools.lru_cache(maxsize=None)
def _regrow_lists(oracle):
    """(class, kind) -> (ids, P).  Classes: U18 = 4097 or more ids, which the automatic mode decodes in k_roc_decode_u2<18> (any
    P <= 18); gen = up to gen_small_max ids, the general decoder and, in a call of few lists, k_roc_decode_b2<32 .. 256> (precisions of
    7 and more: 2^P values spread over enough buckets).  Kinds: `spill` = 30 .. 49 words of growth -- the register ring of the
    wave-per-list stack holds 56 words before ws_spill32 writes 32 of them, so exactly one spill runs --, `deep` = several hundred."""
    L = limits()
    return {("U18", "spill"): _find_growth(oracle, (11, 10), L["U_MIN_LIST"], 9000, 30, 49),
            ("U18", "deep"): _find_growth(oracle, (9, 8), L["U_MIN_LIST"], 9000, 500, 900),
            ("gen", "spill"): _find_growth(oracle, (9, 8, 7), L["TINY_MAX"] + 1, L["GEN_SMALL_MAX"], 30, 49),
            ("gen", "deep"): _find_growth(oracle, (7, 8), L["TINY_MAX"] + 1, L["GEN_SMALL_MAX"], 200, 900)}


def regrow_cases(oracle):
    """one call per precision that the search settled on, each with a healthy list"""
    byP = {}
    for (cls, kind), (ids, P) in _regrow_lists(oracle).items():
        byP.setdefault(P, []).append((ids, f"{cls}-{kind}"))
    out = {}
    for P, items in sorted(byP.items()):
        out[f"regrow-P{P}"] = _call([i for i, _ in items] + [beside(P)], P, [t for _, t in items] + ["beside"])
    return out


def padded_cases(oracle):
    """name -> dict(n, precision, head, words, mt_draws, residue, growth): the streams of the regrowth lists on top of k words that no
    decode step reaches -- but the last: where the decode of the bare stream ends with a pop from the empty stack, this one takes the
    top pad word, and grows by one word less --, k chosen so that nwords = 0, 1, 31, 32, 33 (mod 64) -- where the stack starts decides which words the first
    spills and refills move.  The encoder cannot be made to produce these residues: the length of a stream in this regime is a
    function of P alone (about 0.045 * 2^P words: what the last steps push once log2(n - i) has fallen below P), 23 words at P = 9,
    46 at P = 10.  vidc_roc_import takes any stream; the oracle decodes the padded one like any other."""
    out = {}
    for (cls, kind), (ids, P) in _regrow_lists(oracle).items():
        m = model(oracle, ids, P)
        for r in REGROW_RESIDUES:
            k = (r - m["nwords"]) % 64
            if k == 0 and m["nwords"] == 0 and r == 0:
                k = 64
            pad = np.random.default_rng([P, r, ids.size]).integers(0, 1 << 32, k).astype(np.uint32)
            words = np.concatenate([pad, m["words"]])
            end_words = oracle.roc_decode(m["head"], words, ids.size, P, m["mt_draws"])[2]
            out[f"padded-{cls}-{kind}-mod64={r}"] = dict(n=ids.size, precision=P, head=m["head"], words=words, mt_draws=m["mt_draws"],
                                                         residue=r, growth=int(end_words.size) - int(words.size), base_growth=m["growth"])
    return out


# -- full precision
def full_precision_cases(oracle):
    """P = 32 (two 16-bit slices, the longest streams): the tiny strip -- 1, 63 and 64 ids; 64 ids take more words than the strip's
    window of VIDC_TINY_STRIP holds --, one list per general class"""
    L = limits()
    rng = np.random.default_rng(32)
    sizes = [1, L["TINY_MAX"] - 1, L["TINY_MAX"], 300, L["ENC_C1_MAX"] + 904, L["ENC_C2_MAX"] + 232]
    lists = [np.sort(rng.choice(1 << 31, size=n, replace=False)).astype(np.uint64) for n in sizes]
    return {"full-P32": _call(lists, 32, [f"n{n}" for n in sizes])}


def graph_rows(N=96, K=64, seed=5):
    """int32 [N, K] rows, -1 terminated, 0 .. K distinct unsorted neighbours below 2^20; rows 0 .. 2 hold 0, 1 and K edges"""
    rng = np.random.default_rng(seed)
    rows = np.full((N, K), -1, dtype=np.int32)
    for i in range(N):
        d = (0, 1, K)[i] if i < 3 else int(rng.integers(0, K + 1))
        rows[i, :d] = rng.choice(1 << 20, size=d, replace=False)
    return rows


# -- natural-precision multisets
def multiset_cases(oracle):
    """many duplicates of the ids 0 .. 3 (natural precision 2): one list that draws several hundred words, one that goes over
    the table (the call is refused)"""
    table = limits()["VIDC_MT_TABLE"]
    fig = _memo(lambda n: draws_of(oracle, multiset_ids(n, 2, 1), 2))
    n_over = find_exact(fig, table + 1, 1000, 8000)
    if n_over is None:
        raise SearchFailed("no multiset of the ids 0 .. 3 draws exactly 1025 words")
    n_under = n_over * 3 // 4
    return {"multiset-under": _call([multiset_ids(n_under, 2, 1), beside()], -1, ["multiset", "beside"]),
            "multiset-over": _call([beside(), multiset_ids(n_over, 2, 1)], -1, ["beside", "multiset-over"], fails=1)}


# -- imports with the bottom of the stream cut off
TRUNCATED = (("tiny", 64, 31), ("reg", 256, 24), ("pair", 512, 24), ("quad", 1024, 24), ("rows128", 2048, 24), ("rows256", 4096, 24),
             ("U18", 4097, 16), ("U20-P19", 4097, 19), ("U20-P20", 4097, 20), ("b2", 4097, 24), ("G16K", 9000, 28))


def truncated_cases(oracle, cut=20):
    """name -> dict(n, precision, head, words, mt_draws, end_draws, depth): the stream of a natural list (n distinct ids below 2^P,
    the maximum among them) with its `cut` bottom words removed, and a claimed mt_draws: the decoder runs into the empty stack `cut`
    words early and draws about `cut` words from there on.  Per class of TRUNCATED -- the tiny strip, the lane decoders, the three
    chain decoders, a general class -- one import whose decode ends at exactly 1024 draws and one at 1025 (how many words a decoder
    draws depends on their values: the claimed start is searched); the chain decoders, which no list makes draw, also from 0 with
    300 words cut.  (No class at P = 32: what a decoder makes of table words at that precision are ids of 2^31 and more, outside the
    library's id domain -- the register-rank decoders compare ids as signed numbers.)"""
    table = limits()["VIDC_MT_TABLE"]
    out = {}
    for cls, n, P in TRUNCATED:
        rng = np.random.default_rng([n, P])
        ids = np.sort(rng.choice((1 << min(P, 31)) - 1, size=n - 1, replace=False)).astype(np.uint64)
        ids = np.concatenate([ids, [np.uint64((1 << min(P, 31)) - 1)]])
        e = oracle.roc_encode(ids, P)
        if e["mt_draws"] != 0 or e["words"].size <= cut + 8:
            raise SearchFailed(f"{cls}: a natural list of {n} ids at P={P} has {e['words'].size} words")
        plans = [(cut, target, range(target - cut - 12, target - cut + 4)) for target in (table, table + 1)]
        if n > 4096 and e["words"].size > 320:
            plans.append((300, None, (0,)))
        for c, target, starts in plans:
            for s0 in starts:
                got = oracle.roc_decode_stats(e["head"], e["words"][c:], n, P, s0)
                if target is None or got[3] == target:
                    break
            else:
                raise SearchFailed(f"{cls}: no claimed mt_draws makes the decode end at exactly {target} draws")
            out[f"truncated-{cls}-{'from0' if target is None else 'end%d' % target}"] = dict(
                cls=cls, n=n, precision=P, head=e["head"], words=e["words"][c:].copy(), mt_draws=s0, end_draws=got[3], depth=got[4]["depth"])
    return out


# -- append onto a list at a fixed low precision
def append_case(oracle, P=4, start_draws=800):
    """-> dict(P, old=[list, a list of 8 ids that is lossless at P], add (ids for list 0; the first k_ok of them make the merged list draw exactly 1024 words, one
    more makes it draw 1025), k_ok, old_model, new_decode_refused (the merged list encodes, and its decode draws a 1025th word)).  The merged list is what the old object DECODES to (a multiset of P-bit values), then the batch
    ids in batch order (include/vidc.h, "append")."""
    table = limits()["VIDC_MT_TABLE"]
    old = find_draws(oracle, P, start_draws, 2000, 8000, 13)
    m = model(oracle, old, P)
    assert not m["decode_refused"]
    pool = _permutation(13, 99)
    fig = _memo(lambda k: draws_of(oracle, np.concatenate([m["order"], pool[:k]]), P))
    hi = 4000
    if fig(hi) <= table:
        raise SearchFailed("4000 appended ids do not reach the table's end")
    a, b = 0, hi
    while a < b:  # the first k with more than 1024 draws
        mid = (a + b) // 2
        if fig(mid) > table:
            b = mid
        else:
            a = mid + 1
    # (a is the first k beyond the table; draws step by at most one per id here, checked)
    if fig(a - 1) != table or fig(a) != table + 1:
        raise SearchFailed("no batch takes the merged list from exactly 1024 to 1025 draws")
    mk = model(oracle, np.concatenate([m["order"], pool[:a - 1]]), P)
    # (the list the batch does not touch keeps its stream, which is the from-scratch one only for a list that decodes to itself)
    small = np.array([1, 3, 4, 7, 9, 12, 14, 15], dtype=np.uint64)
    return dict(P=P, old=[old, small], add=pool[:a].copy(), k_ok=a - 1, old_model=m, new_decode_refused=mk["decode_refused"])


def all_calls(oracle):
    """every case that is one encode call: name -> call"""
    out = {}
    for f in (edge_cases, partial_cases, depth_cases, regrow_cases, full_precision_cases, multiset_cases):
        out.update(f(oracle))
    return out
