// ivf_residual_plan.h -- what the host decides for vidc_ivf_scan_residual_dev and vidc_ivf_range_{count,fill}_residual_dev before any
// device work: the argument checks, the LDS of one wavefront, the resident wavefront slots, the cut S of a probe row, the scratch of
// the cut, the load width W of a code and the load width of the codebooks.  Host only, no HIP runtime: ivf_residual.hip includes it
// and tests/ivf_residual_test.cpp builds it with g++.  The count and the fill of one search make the same plan from the same
// arguments.
//
// The cut is the scan's rule (ivs::pieces).  Tables here belong to (query, list), not to an item: cutting a row into S pieces costs
// no extra table builds, where every piece of a raw-PQ scan rebuilds its query's table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_range_plan.h"
#include "ivf_residual_ref.h"
#include "ivf_scan_plan.h"

namespace vidc {
namespace ivx {

// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work): the scan's refusals for PQ8, and the centroids
struct Args {
    uint64_t nlist;
    const void *offsets;
    uint64_t ntotal;
    const void *codes;
    uint32_t d, M;
    const void *codebooks, *centroids;
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
};
inline const char *check_scan(const Args &a, uint32_t k, const void *D, const void *labels) {
    const ivs::Args s = {a.nlist, a.offsets, a.ntotal, a.codes, ivs::PQ8, a.d, a.M, a.codebooks, a.nq, a.xq, a.nprobe, a.probes, k, D, labels};
    if (const char *msg = ivs::check_args(s)) return msg;
    if (a.nq && !a.centroids) return "NULL centroids";
    return nullptr;
}
inline ivr::Args range_args(const Args &a, const void *slot_lims) {
    const ivr::Args r = {a.nlist, a.offsets, a.ntotal, a.codes, ivs::PQ8, a.d, a.M, a.codebooks, a.nq, a.xq, a.nprobe, a.probes, slot_lims};
    return r;
}
inline const char *check_count(const Args &a, const void *slot_lims) {
    if (const char *msg = ivr::check_count(range_args(a, slot_lims))) return msg;
    if (a.nq && !a.centroids) return "NULL centroids";
    return nullptr;
}
inline const char *check_fill(const Args &a, const void *slot_lims, uint64_t capacity, const void *D, const void *labels) {
    if (const char *msg = ivr::check_fill(range_args(a, slot_lims), capacity, D, labels)) return msg;
    if (a.nq && !a.centroids) return "NULL centroids";
    return nullptr;
}

// dynamic LDS of a wavefront, every part a multiple of 16 bytes: the pool block of the scan (two pools of k keys, the survivors' keys
// and the raw scan's 64 trip floats, which the PQ trip leaves unused: the block keeps the raw scan's size; the range search has
// none), the probe row, the query vector, the residual, the M x 256 table of the list being scanned.
// The query vector is read in front of every list, so unlike the raw-PQ scan's it shares no bytes with the pools.
inline size_t pool_bytes(uint32_t k) { return (size_t)2 * k * 8 + (size_t)ivs::TRIP * 8 + (size_t)ivs::TRIP * 4; }
inline size_t row_bytes(uint32_t nprobe) { return ivs::round16((size_t)nprobe * 4); }
inline size_t vec_bytes(uint32_t d) { return ivs::round16((size_t)d * 4); }
inline size_t table_bytes(uint32_t M) { return (size_t)M * 256 * 4; }
inline size_t scan_lds_bytes(uint32_t k, uint32_t nprobe, uint32_t d, uint32_t M) {
    return pool_bytes(k) + row_bytes(nprobe) + 2 * vec_bytes(d) + table_bytes(M);
}
inline size_t range_lds_bytes(uint32_t nprobe, uint32_t d, uint32_t M) { return row_bytes(nprobe) + 2 * vec_bytes(d) + table_bytes(M); }
// (scan, d = 128, M = 16, k = 20, nprobe = 16: 1088 + 64 + 512 + 512 + 16384 = 18560 bytes, eight wavefronts per compute unit where
// the raw-PQ scan has nine; at the limits 4864 + 4096 + 8192 + 8192 + 65536 = 90880 bytes, one.  range, the same shape: 17472, nine)

// the table build reads the codebooks 16 bytes at a load where every row of a sub-quantiser starts on a 16-byte boundary
inline bool codebook_vec4(uint32_t d, uint32_t M, uintptr_t codebooks) { return M && (d / M) % 4 == 0 && codebooks % 16 == 0; }

struct Plan {
    size_t lds, merge_lds;  // (range: merge_lds = 0)
    uint32_t resident, S, nslots, W;
    bool vec4;
    uint64_t items, scratch;  // scan: the runs of a cut call; range: the nq * nprobe hit counts
};
inline Plan finish_plan(Plan p, uint32_t num_cu, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uintptr_t codes, uintptr_t codebooks) {
    p.resident = ivs::resident_slots(num_cu, p.lds);
    p.S = ivs::pieces(nq, nprobe, p.resident);
    p.items = nq * p.S;
    p.nslots = ivs::slots(p.items, p.resident);
    p.W = ivs::code_load_bytes(M, codes);
    p.vec4 = codebook_vec4(d, M, codebooks);
    return p;
}
inline Plan scan_plan(uint32_t num_cu, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uint32_t k, uintptr_t codes,
                      uintptr_t codebooks) {
    Plan p = {};
    p.lds = scan_lds_bytes(k, nprobe, d, M);
    p = finish_plan(p, num_cu, d, M, nq, nprobe, codes, codebooks);
    p.scratch = ivs::scratch_bytes(nq, p.S, k);
    p.merge_lds = ivs::merge_lds_bytes(p.S, k);
    return p;
}
inline Plan range_plan(uint32_t num_cu, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uintptr_t codes, uintptr_t codebooks) {
    Plan p = {};
    p.lds = range_lds_bytes(nprobe, d, M);
    p = finish_plan(p, num_cu, d, M, nq, nprobe, codes, codebooks);
    p.scratch = ivr::count_bytes(nq, nprobe);
    return p;
}

}  // namespace ivx
}  // namespace vidc
