"""Numpy statement of the segmented ROC container (include/vidc.h, "segmented ROC lists").

A list of n ids over a universe of B bits is cut by VALUE RANGE into S = 2^k segments, k = 0 for n <= T and min(B, ceil_log2(ceil(n / T)))
otherwise: id x goes to segment x >> (B - k) and is stored as x & (2^(B - k) - 1).  The partition is stable (a segment keeps its ids in
the list's input order).  The inner object is an ordinary ROC object over the sum of S_l lists in (list, segment) order, encoded with
bit_width(max) per segment; because the segments of a list are consecutive, inner and outer CSR address the same positions.
"""
import numpy as np

MAX_SEGS = 1024      # VIDC_ROCSEG_MAX_SEGS
DEFAULT_IDS = 1024   # VIDC_ROCSEG_DEFAULT_IDS
CHUNK = 1024         # ids per wavefront of the multisplit (roc_seg_plan.h: SEG_CHUNK)


def bit_width(x):
    return int(x).bit_length()


def ceil_log2(x):
    return (int(x) - 1).bit_length()


def universe_bits(ids):
    """universe_bits = 0 of the C call: max(1, bit_width(largest id))"""
    ids = np.asarray(ids, dtype=np.uint64)
    return max(1, bit_width(ids.max())) if ids.size else 1


def seg_k(n, T, B):
    return 0 if n <= T else min(B, ceil_log2(-(-int(n) // T)))


def plan(offsets, T, B):
    """-> (k[nlist], shift[nlist], seg_first[nlist + 1]); ValueError where the C call answers VIDC_ERR_DOMAIN"""
    offsets = np.asarray(offsets, dtype=np.uint64)
    sizes = (offsets[1:] - offsets[:-1]).astype(np.int64)
    k = np.array([seg_k(n, T, B) for n in sizes], dtype=np.int64)
    if k.size and int(k.max()) > ceil_log2(MAX_SEGS):
        raise ValueError("a list needs more than MAX_SEGS segments")
    seg_first = np.concatenate([[0], np.cumsum(1 << k)]).astype(np.uint64)
    return k, (B - k).astype(np.uint8), seg_first


def split(offsets, ids, T, B):
    """The stable multisplit -> dict(k, shift, seg_first, inner_offsets, rebased, src_pos): rebased[inner_offsets[i] + j] is the j-th id
    of inner list i (input order kept), src_pos the position inside its outer list that it came from."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.uint64)
    if ids.size and int(ids.max()) >> B:
        raise ValueError("an id >= 2^B")
    k, shift, seg_first = plan(offsets, T, B)
    rebased = np.zeros(ids.size, np.uint64)
    src_pos = np.zeros(ids.size, np.uint32)
    inner_sizes = np.zeros(int(seg_first[-1]), np.int64)
    for l in range(offsets.size - 1):
        a, b = int(offsets[l]), int(offsets[l + 1])
        li = ids[a:b]
        sh = np.uint64(shift[l])
        key = (li >> sh).astype(np.int64) if k[l] else np.zeros(li.size, np.int64)
        order = np.argsort(key, kind="stable")
        rebased[a:b] = li[order] & np.uint64((1 << int(sh)) - 1)
        src_pos[a:b] = order
        inner_sizes[int(seg_first[l]): int(seg_first[l + 1])] = np.bincount(key, minlength=1 << int(k[l]))
    inner_offsets = np.concatenate([[0], np.cumsum(inner_sizes)]).astype(np.uint64)
    return dict(k=k, shift=shift, seg_first=seg_first, inner_offsets=inner_offsets, rebased=rebased, src_pos=src_pos, B=B, T=T,
                offsets=offsets)


def split_brute(offsets, ids, T, B):
    """the same by a loop over the ids, one at a time -> (inner lists of rebased ids, inner lists of source positions)"""
    inner, pos = [], []
    for l in range(len(offsets) - 1):
        n = int(offsets[l + 1] - offsets[l])
        k = seg_k(n, T, B)
        segs = [[] for _ in range(1 << k)]
        poss = [[] for _ in range(1 << k)]
        for p in range(n):
            x = int(ids[int(offsets[l]) + p])
            s = x >> (B - k) if k else 0
            segs[s].append(x & ((1 << (B - k)) - 1))
            poss[s].append(p)
        inner += segs
        pos += poss
    return inner, pos


def bases(model):
    """base of every inner list: segment number << shift of its outer list"""
    out = np.zeros(int(model["seg_first"][-1]), np.uint64)
    for l in range(model["k"].size):
        a, b = int(model["seg_first"][l]), int(model["seg_first"][l + 1])
        out[a:b] = np.arange(b - a, dtype=np.uint64) << np.uint64(model["shift"][l])
    return out


def segment(model, i):
    a, b = int(model["inner_offsets"][i]), int(model["inner_offsets"][i + 1])
    return model["rebased"][a:b]


def encode_segments(model, oracle):
    """Every inner list through the CPU oracle at bit_width(max) (VIDC_PREC_EXACT) -> list of dict(n, precision, head, words, order,
    perm, mt_draws) or None for an empty segment.  The stream of a list depends on its set of ids: the oracle gets them ascending, and
    `perm` is turned into positions of the segment's own (input) order."""
    out = []
    for i in range(int(model["seg_first"][-1])):
        seg = segment(model, i)
        if not seg.size:
            out.append(None)
            continue
        asc = np.argsort(seg, kind="stable")
        P = bit_width(seg.max())
        e = oracle.roc_encode(seg[asc], P)
        out.append(dict(n=seg.size, precision=P, head=e["head"], words=e["words"], order=e["order"], perm=asc[e["perm"]].astype(np.uint32),
                        mt_draws=e["mt_draws"]))
    return out


def decode_order(model, encs):
    """what decode_all returns: per list its segments in order, each in its own sampling order, base added"""
    base = bases(model)
    out = np.zeros(model["rebased"].size, np.uint64)
    for i, e in enumerate(encs):
        if e is not None:
            out[int(model["inner_offsets"][i]): int(model["inner_offsets"][i + 1])] = e["order"] + base[i]
    return out


def compose_perm(model, inner_perm):
    """perm[g] = src_pos[inner position of inner_perm[g]]: output position -> input position within the outer list"""
    io = model["inner_offsets"].astype(np.int64)
    sizes = io[1:] - io[:-1]
    start = np.repeat(io[:-1], sizes)
    return model["src_pos"][start + np.asarray(inner_perm, dtype=np.int64)]


def inner_perm(model, encs):
    out = np.zeros(model["rebased"].size, np.uint32)
    for i, e in enumerate(encs):
        if e is not None:
            out[int(model["inner_offsets"][i]): int(model["inner_offsets"][i + 1])] = e["perm"]
    return out


def inner_bytes(encs):
    """vidc_roc_compressed_bytes of the inner object: 8 + 4 * nwords per non-empty list"""
    return sum(8 + 4 * e["words"].size for e in encs if e is not None)


def compressed_bytes(model, encs):
    nseg = (1 << model["k"])
    return inner_bytes(encs) + 4 * int(nseg[nseg > 1].sum())


def expand_request(model, list_nos):
    """decode_lists: outer list numbers -> (inner list numbers, first inner entry of every request [m + 1])"""
    sf = model["seg_first"].astype(np.int64)
    inner, first = [], [0]
    for l in list_nos:
        inner += list(range(int(sf[l]), int(sf[l + 1])))
        first.append(len(inner))
    return np.array(inner, np.uint64), np.array(first, np.uint64)


def chunk_table(offsets, T, B):
    """the multisplit's chunks, (list, start) with start a multiple of CHUNK, and tbl_base[nlist + 1]: list l owns the count-table
    entries tbl_base[l] + s * nchunks_l + c"""
    k, _, _ = plan(offsets, T, B)
    chunks, tbl = [], [0]
    for l in range(len(offsets) - 1):
        n = int(offsets[l + 1] - offsets[l])
        nc = -(-n // CHUNK)
        chunks += [(l, c * CHUNK) for c in range(nc)]
        tbl.append(tbl[-1] + (nc << int(k[l])))
    return chunks, np.array(tbl, np.uint64)
