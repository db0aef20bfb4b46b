// roc_seg_plan.h -- host plan of the segmented ROC container (roc_seg.hip; include/vidc.h, "segmented ROC lists").  Host code only:
// builds with g++ (tests/roc_seg_plan_test.cpp) and holds no HIP type.
//
// A list of n ids over a universe of B bits is cut by value range into S = 2^k segments, k = 0 for n <= T, else
// min(B, ceil_log2(ceil(n / T))): id x sits in segment x >> (B - k) as x & (2^(B - k) - 1).  The inner object is an ordinary vidc_roc
// over the sum of S_l lists in (list, segment) order.  Here: k / shift / segment counts per list, the multisplit's chunk table and the
// layout of its count table, the chunks of the base fix-up, the expansion of a decode_lists request, and the checks of an imported map.
#pragma once
#include <cstdint>
#include <vector>

namespace vidc {
namespace rocseg {

constexpr uint32_t SEG_CHUNK = 1024;  // ids per wavefront of the multisplit and of the base fix-up
constexpr uint32_t MAX_SEGS = 1024;   // VIDC_ROCSEG_MAX_SEGS
constexpr uint32_t MIN_IDS = 16, MAX_IDS = 65536;

inline uint32_t bit_width(uint64_t x) {
    uint32_t b = 0;
    for (; x; x >>= 1) b++;
    return b;
}
inline uint32_t ceil_log2(uint64_t x) { return x <= 1 ? 0u : bit_width(x - 1); }
inline bool valid_seg_ids(uint32_t T) { return T >= MIN_IDS && T <= MAX_IDS && (T & (T - 1)) == 0; }
inline uint32_t seg_k(uint64_t n, uint32_t T, uint32_t B) {
    if (n <= T) return 0;
    const uint32_t k = ceil_log2((n + T - 1) / T);
    return k < B ? k : B;
}

// per outer list, as the kernels read it
struct ListSeg {
    uint64_t off;        // first position of the list (outer CSR = inner CSR)
    uint64_t tbl_base;   // its entries of the count table: tbl_base + s * nchunks + c
    uint32_t seg_first;  // its first inner list
    uint32_t n;
    uint32_t nchunks;    // ceil(n / SEG_CHUNK)
    uint8_t k, shift;
    uint16_t pad;
};
struct SplitChunk {
    uint32_t list;
    uint32_t start;  // multiple of SEG_CHUNK, < n of the list
};
// `count` decoded ids at position `start` of an output buffer get `base` ORed in (count <= SEG_CHUNK, base < 2^31)
struct FixChunk {
    uint64_t start;
    uint32_t count;
    uint32_t base;
};

struct SegPlan {
    uint32_t T = 0, B = 0;
    std::vector<ListSeg> lists;
    std::vector<uint64_t> seg_first;  // nlist + 1
    std::vector<uint8_t> shift;       // nlist
    std::vector<SplitChunk> chunks;
    uint64_t table_len = 0;  // entries of the count table
    uint64_t n_inner = 0;
    uint64_t meta_segs = 0;  // segments of the lists with S > 1: 4 bytes each in compressed_bytes
};

enum { PLAN_OK = 0, PLAN_TOO_MANY_SEGS = 1, PLAN_LIST_TOO_LONG = 2, PLAN_TABLE_TOO_LONG = 3 };

// offsets: nlist + 1 monotone entries from 0 (checked by the caller).  *bad_list names the list of a non-zero status.
inline int make_plan(const uint64_t *offsets, uint64_t nlist, uint32_t T, uint32_t B, SegPlan &p, uint64_t *bad_list) {
    p = SegPlan();
    p.T = T;
    p.B = B;
    p.lists.resize(nlist);
    p.seg_first.assign(nlist + 1, 0);
    p.shift.assign(nlist, (uint8_t)B);
    uint64_t nchunks_total = 0;
    for (uint64_t l = 0; l < nlist; l++) {
        const uint64_t n = offsets[l + 1] - offsets[l];
        if (n >= 0xffffffffull) { *bad_list = l; return PLAN_LIST_TOO_LONG; }
        const uint32_t k = seg_k(n, T, B);
        if ((1ull << k) > MAX_SEGS) { *bad_list = l; return PLAN_TOO_MANY_SEGS; }
        ListSeg &s = p.lists[l];
        s.off = offsets[l];
        s.tbl_base = p.table_len;
        s.seg_first = (uint32_t)p.seg_first[l];
        s.n = (uint32_t)n;
        s.nchunks = (uint32_t)((n + SEG_CHUNK - 1) / SEG_CHUNK);
        s.k = (uint8_t)k;
        s.shift = (uint8_t)(B - k);
        s.pad = 0;
        p.shift[l] = s.shift;
        p.seg_first[l + 1] = p.seg_first[l] + (1ull << k);
        p.table_len += (uint64_t)s.nchunks << k;
        if (k) p.meta_segs += 1ull << k;
        nchunks_total += s.nchunks;
        // (the scan takes a 32-bit length; inner list numbers sit in the upper half of a non-negative label)
        if (p.table_len >= 0xffffffffull || p.seg_first[l + 1] >= 0x7fffffffull) { *bad_list = l; return PLAN_TABLE_TOO_LONG; }
    }
    p.n_inner = p.seg_first[nlist];
    p.chunks.reserve(nchunks_total);
    for (uint64_t l = 0; l < nlist; l++)
        for (uint32_t c = 0; c < p.lists[l].nchunks; c++) p.chunks.push_back(SplitChunk{(uint32_t)l, c * SEG_CHUNK});
    return PLAN_OK;
}

inline void push_fix_chunks(std::vector<FixChunk> &out, uint64_t start, uint64_t count, uint32_t base) {
    if (!base) return;
    for (uint64_t c = 0; c < count; c += SEG_CHUNK) {
        const uint64_t left = count - c;
        out.push_back(FixChunk{start + c, (uint32_t)(left < SEG_CHUNK ? left : SEG_CHUNK), base});
    }
}

// decode_all: inner_offsets[n_inner + 1] of the inner object
inline std::vector<FixChunk> fix_chunks_all(const std::vector<uint64_t> &seg_first, const std::vector<uint8_t> &shift,
                                            const std::vector<uint64_t> &inner_offsets) {
    std::vector<FixChunk> out;
    for (size_t l = 0; l + 1 < seg_first.size(); l++)
        for (uint64_t i = seg_first[l] + 1; i < seg_first[l + 1]; i++)
            push_fix_chunks(out, inner_offsets[i], inner_offsets[i + 1] - inner_offsets[i], (uint32_t)((i - seg_first[l]) << shift[l]));
    return out;
}

// decode_lists: the request's outer list numbers (each < nlist: checked by the caller) -> the inner list numbers, request by request
inline std::vector<uint64_t> expand_request(const std::vector<uint64_t> &seg_first, uint64_t m, const uint64_t *list_nos) {
    std::vector<uint64_t> inner;
    for (uint64_t j = 0; j < m; j++)
        for (uint64_t i = seg_first[list_nos[j]]; i < seg_first[list_nos[j] + 1]; i++) inner.push_back(i);
    return inner;
}
// ... and behind the inner decode_lists (inner_out[m' + 1] = its packing): out_offsets[m + 1] and the fix-up chunks
inline std::vector<FixChunk> collapse_request(const std::vector<uint64_t> &seg_first, const std::vector<uint8_t> &shift, uint64_t m,
                                              const uint64_t *list_nos, const std::vector<uint64_t> &inner_out, uint64_t *out_offsets) {
    std::vector<FixChunk> out;
    uint64_t at = 0;
    out_offsets[0] = 0;
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t l = list_nos[j], S = seg_first[l + 1] - seg_first[l];
        for (uint64_t s = 1; s < S; s++)
            push_fix_chunks(out, inner_out[at + s], inner_out[at + s + 1] - inner_out[at + s], (uint32_t)(s << shift[l]));
        at += S;
        out_offsets[j + 1] = inner_out[at];
    }
    return out;
}

// An imported map (vidc_rocseg_wrap): seg_first monotone from 0 to the inner object's list count, every segment count a power of two
// <= MAX_SEGS that equals 2^(B - shift), every inner precision <= its list's shift.  -> 0, or 1 + the first bad list (nlist + 1: the
// ends of seg_first).
inline uint64_t check_map(uint64_t nlist, const uint64_t *seg_first, const uint8_t *shift, uint32_t B, uint64_t inner_nlist,
                          const uint32_t *inner_precisions) {
    if (seg_first[0] != 0 || seg_first[nlist] != inner_nlist) return nlist + 1;
    for (uint64_t l = 0; l < nlist; l++) {
        if (seg_first[l + 1] <= seg_first[l] || seg_first[l + 1] > inner_nlist) return l + 1;
        const uint64_t S = seg_first[l + 1] - seg_first[l];
        if (S > MAX_SEGS || (S & (S - 1)) != 0 || shift[l] > B || S != (1ull << (B - shift[l]))) return l + 1;
        for (uint64_t i = seg_first[l]; i < seg_first[l + 1]; i++)
            if (inner_precisions[i] > shift[l]) return l + 1;
    }
    return 0;
}

}  // namespace rocseg
}  // namespace vidc
