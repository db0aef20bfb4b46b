// ivf_pqbits_plan.h -- what the host decides for vidc_ivf_scan_pqbits_dev before any device work, and the serial statement of a packed
// PQ code: the layout (code_size, the field of a sub-quantiser), the table entry over ksub = 2^nbits codewords, the argument checks,
// the LDS of one wavefront, the resident wavefront slots, the cut S and its scratch.  Host only, no HIP runtime: ivf_pqbits.hip
// includes it and tests/ivf_pqbits_plan_test.cpp builds it with g++.
//
// The layout (include/vidc.h): a code row is one little-endian bit string of code_size = ceil(M * nbits / 8) bytes, sub-quantiser m
// in the bits [m * nbits, (m + 1) * nbits), bit i of the row = bit i % 8 of byte i / 8, pad bits 0.  At nbits == 8 that is M bytes.
//
// Everything else -- probe rule, duplicate rule, clamp of a list range, key, insert by rank, the cut, the merge -- is the 8-bit
// scan's (ivf_scan_ref.h, ivf_scan_plan.h, ivf_residual_plan.h) and is called from there, not restated.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_residual_plan.h"
#include "ivf_scan_plan.h"
#include "ivf_scan_ref.h"

namespace vidc {
namespace ipb {

constexpr uint32_t MAX_NBITS = 12;              // bits of a sub-quantiser: 1 .. 12 (4096 codewords)
constexpr uint32_t BUILD4_KSUB = 256;           // from here on the table build keeps four entries of a lane in flight
constexpr size_t LDS_LIMIT = ivs::LDS_PER_CU;   // a wavefront's table, pools, row, vectors and code span have to fit one compute unit

VIDC_HD inline uint32_t ksub_of(uint32_t nbits) { return 1u << nbits; }
VIDC_HD inline uint64_t code_size(uint32_t M, uint32_t nbits) { return ((uint64_t)M * nbits + 7u) / 8u; }
// field m of a code row, a bit at a time from the layout statement (the kernels read it through a 64-bit window)
VIDC_HD inline uint32_t field_of(const uint8_t *row, uint32_t m, uint32_t nbits) {
    uint32_t f = 0;
    for (uint32_t b = 0; b < nbits; b++) {
        const uint32_t i = m * nbits + b;
        f |= (uint32_t)((row[i >> 3] >> (i & 7u)) & 1u) << b;
    }
    return f;
}
// entry (m, c) of a table: ivs::pq_entry's arithmetic in its order, over ksub codewords a sub-quantiser
VIDC_HD inline float entry(const float *v, const float *codebooks, uint32_t dsub, uint32_t ksub, uint32_t m, uint32_t c) {
    return ivs::l2_serial(v + (uint64_t)m * dsub, codebooks + ((uint64_t)m * ksub + c) * dsub, dsub);
}

// dynamic LDS of a scan wavefront, every part a multiple of 16 bytes: the residual scan's pool block, probe row and query vector
// (ivx::pool_bytes, row_bytes, vec_bytes), the residual (only with centroids), the staged code span of a trip, the M x ksub table.
// The span: 64 codes and what an aligned 16-byte load adds in front of and behind them, and the word behind a lane's 64-bit window.
inline size_t stage_bytes(uint32_t M, uint32_t nbits) { return ivs::round16((size_t)ivs::TRIP * code_size(M, nbits) + 32); }
inline size_t table_bytes(uint32_t M, uint32_t nbits) { return (size_t)M * ksub_of(nbits) * 4; }
inline size_t lds_bytes(uint32_t k, uint32_t nprobe, uint32_t d, uint32_t M, uint32_t nbits, bool residual) {
    return ivx::pool_bytes(k) + ivx::row_bytes(nprobe) + (residual ? 2 : 1) * ivx::vec_bytes(d) + stage_bytes(M, nbits) + table_bytes(M, nbits);
}
// (PQ8x10 residual, d = 128, k = 20, nprobe = 16: 1088 + 64 + 1024 + 672 + 32768 = 35616 bytes, four wavefronts per compute unit;
// the largest table that passes is 2^15 entries, M x nbits = 32 x 10 or 8 x 12: 131072 bytes of table, one wavefront)

struct Args {
    uint64_t nlist;
    const void *offsets;
    uint64_t ntotal;
    const void *codes;
    uint32_t d, M, nbits;
    const void *codebooks, *centroids;  // centroids NULL: raw PQ
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
    uint32_t k;
    const void *D, *labels;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work): the 8-bit scan's refusals, the bits, the LDS limit
inline const char *check_scan(const Args &a) {
    const ivs::Args s = {a.nlist, a.offsets, a.ntotal, a.codes, ivs::PQ8, a.d, a.M, a.codebooks, a.nq, a.xq, a.nprobe, a.probes, a.k, a.D, a.labels};
    if (const char *msg = ivs::check_args(s)) return msg;
    if (a.nbits < 1 || a.nbits > MAX_NBITS) return "1 <= nbits <= 12";
    if (lds_bytes(a.k, a.nprobe, a.d, a.M, a.nbits, a.centroids != nullptr) > LDS_LIMIT)
        return "the M x 2^nbits table, pools, probe row, vectors and code span of a wavefront exceed the LDS limit of 163840 bytes (160 KB)";
    return nullptr;
}

struct Plan {
    size_t lds, merge_lds;
    uint32_t resident, S, nslots;
    bool vec4;
    uint64_t items, scratch;
};
// resident slots from the real LDS size (ivs::resident_slots), the cut and its scratch by the scan's rules.  A residual table belongs
// to (query, list), a raw one to the item: the cut costs the raw scan one more table build per piece, as it does at 8 bits.
inline Plan scan_plan(uint32_t num_cu, uint32_t d, uint32_t M, uint32_t nbits, bool residual, uint64_t nq, uint32_t nprobe, uint32_t k,
                      uintptr_t codebooks) {
    Plan p = {};
    p.lds = lds_bytes(k, nprobe, d, M, nbits, residual);
    p.resident = ivs::resident_slots(num_cu, p.lds);
    p.S = ivs::pieces(nq, nprobe, p.resident);
    p.items = nq * p.S;
    p.nslots = ivs::slots(p.items, p.resident);
    p.vec4 = ivx::codebook_vec4(d, M, codebooks);
    p.scratch = ivs::scratch_bytes(nq, p.S, k);
    p.merge_lds = ivs::merge_lds_bytes(p.S, k);
    return p;
}

}  // namespace ipb
}  // namespace vidc
