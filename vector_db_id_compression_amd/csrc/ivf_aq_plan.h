// ivf_aq_plan.h -- what the host decides for vidc_ivf_aq_lut_dev and vidc_ivf_scan_aq_dev before any device work, and the serial
// statement of an additive-quantiser code (RQ<M>x8_Nfloat): the layout, the distance of a row, the argument checks, the LDS of one
// scan wavefront, the query chunk that bounds the table scratch, the tiles of the table GEMM.  Host only, no HIP runtime:
// ivf_aq.hip includes it and tests/ivf_aq_plan_test.cpp builds it with g++.
//
// The layout (include/vidc.h): a code row is code_size = M + 4 bytes, the stage indices c_0 .. c_{M-1} (one byte each) and behind
// them the little-endian float32 norm of the stored vector.  Codebooks are float32 [M, 256, d]: every codeword spans all d
// components.
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
namespace iaq {

constexpr uint32_t KSUB = 256;                       // codewords of a stage (8 bits)
constexpr uint32_t NORM_BYTES = 4;                   // the float32 behind the indices
constexpr uint64_t LUT_SCRATCH = 64ull << 20;        // bytes of context scratch the tables of one chunk may take
// the table GEMM: a workgroup of four wavefronts takes a tile of TQ queries x TN table entries, KC components a pass
constexpr uint32_t LUT_THREADS = 256, TQ = 64, TN = 128, KC = 32, LDW = KC + 4;

VIDC_HD inline uint64_t code_size(uint32_t M) { return (uint64_t)M + NORM_BYTES; }
// the stored norm of a row, a byte at a time from the layout statement (the kernel reads it through two aligned LDS words)
VIDC_HD inline float norm_of(const uint8_t *row, uint32_t M) {
    uint32_t u = 0;
    for (uint32_t b = 0; b < 4; b++) u |= (uint32_t)row[M + b] << (8u * b);
    return ivs::bits_f32(u);
}
// the distance of a row from the query's table (M x 256, entry (m, j) = <xq, codebooks[m][j]>), cq = <xq, centroid> (0 where the
// codes are of the raw vector) and qn = |xq|^2.  The compare, not an fmax: a negative value, -0 and a NaN all become +0, so the
// bits of a distance order like its value
VIDC_HD inline float clamp_dist(float v) { return v > 0.f ? v : 0.f; }
// the two steps k_ivf_scan_aq calls too (it takes the norm through a window of two LDS words instead of norm_of's bytes)
VIDC_HD inline float table_sum(const uint8_t *row, uint32_t M, const float *table) {
    float t = 0.f;
    for (uint32_t m = 0; m < M; m++) t += table[m * KSUB + row[m]];
    return t;
}
VIDC_HD inline float finish(float t, float n, float cq, float qn, bool residual) {
    return clamp_dist(__builtin_fmaf(-2.f, residual ? cq + t : t, qn + n));
}
VIDC_HD inline float distance(const uint8_t *row, uint32_t M, const float *table, float cq, float qn, bool residual) {
    return finish(table_sum(row, M, table), norm_of(row, M), cq, qn, residual);
}

// dynamic LDS of a scan wavefront, every part a multiple of 16 bytes: the residual scan's pool block, probe row and query vector
// (ivx::pool_bytes, row_bytes, vec_bytes), the staged code span of a trip, the M x 256 table.  The span: 64 rows and what an aligned
// 16-byte load adds in front of and behind them, and the word behind a lane's norm window.
inline size_t stage_bytes(uint32_t M) { return ivs::round16((size_t)ivs::TRIP * code_size(M) + 32); }
inline size_t table_bytes(uint32_t M) { return (size_t)M * KSUB * 4; }
inline size_t lds_bytes(uint32_t k, uint32_t nprobe, uint32_t d, uint32_t M) {
    return ivx::pool_bytes(k) + ivx::row_bytes(nprobe) + ivx::vec_bytes(d) + stage_bytes(M) + table_bytes(M);
}
// (RQ8, d = 128, k = 20, nprobe = 16: 1088 + 64 + 512 + 800 + 8192 = 10656 bytes, fifteen wavefronts a compute unit; at the limits
// M = 64, d = 2048, k = 256, nprobe = 1024: 4864 + 4096 + 8192 + 4384 + 65536 = 87072 bytes, one)
// the table GEMM's LDS: TQ query rows and TN codeword rows of KC components, rows LDW floats apart
constexpr size_t lut_lds_bytes() { return (size_t)(TQ + TN) * LDW * 4; }

// the queries of one chunk: what LUT_SCRATCH holds of M x 256 float tables, rounded down to 16, at least 16
inline uint64_t chunk_queries(uint32_t M) {
    const uint64_t c = (LUT_SCRATCH / ((uint64_t)1024 * (M ? M : 1))) & ~(uint64_t)15;
    return c < 16 ? 16 : c;
}
inline uint64_t chunks(uint64_t nq, uint32_t M) { return (nq + chunk_queries(M) - 1) / chunk_queries(M); }
inline uint64_t lut_bytes(uint64_t nq, uint32_t M) { return nq * (uint64_t)M * KSUB * 4; }
// tiles of the table GEMM over nq queries: item = query tile * column tiles + column tile
inline uint64_t lut_col_tiles(uint32_t M) { return (uint64_t)M * KSUB / TN; }
inline uint64_t lut_tiles(uint64_t nq, uint32_t M) { return (nq + TQ - 1) / TQ * lut_col_tiles(M); }
inline uint32_t lut_grid(uint32_t num_cu, uint64_t tiles) {
    const uint64_t cap = (uint64_t)(num_cu ? num_cu : 1) * 4;
    return (uint32_t)(tiles < cap ? (tiles ? tiles : 1) : cap);
}

struct LutArgs {
    uint32_t d, M;
    const void *codebooks;
    uint64_t nq;
    const void *xq, *lut;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work)
inline const char *check_lut(const LutArgs &a) {
    if (!a.codebooks || (a.nq && (!a.xq || !a.lut))) return "NULL codebook, query or table array";
    if (a.d < 1 || a.d > ivs::MAX_D) return "1 <= d <= 2048";
    if (a.M < 1 || a.M > ivs::MAX_M) return "1 <= M <= 64";
    if (a.nq >= (1ull << 32)) return "nq must be below 2^32";
    return nullptr;
}

struct Args {
    uint64_t nlist;
    const void *offsets;
    uint64_t ntotal;
    const void *codes;
    uint32_t d, M;
    const void *codebooks, *centroids;  // centroids NULL: codes of the raw vector
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
    uint32_t k;
    const void *D, *labels;
};
// the scan's refusals (k, nprobe, d, ntotal, nlist, NULL arrays), M and the codebooks; no d % M condition: a codeword has d components
inline const char *check_scan(const Args &a) {
    const ivs::Args s = {a.nlist, a.offsets, a.ntotal, a.codes, ivs::FLAT, a.d, a.M, a.codebooks, a.nq, a.xq, a.nprobe, a.probes, a.k, a.D, a.labels};
    if (const char *msg = ivs::check_args(s)) return msg;
    if (a.M < 1 || a.M > ivs::MAX_M) return "1 <= M <= 64";
    if (!a.codebooks) return "NULL codebooks";
    if (a.nq >= (1ull << 32)) return "nq must be below 2^32";
    return nullptr;
}

struct Plan {
    size_t lds, merge_lds;
    uint32_t resident, S, nslots;
    uint64_t items, scratch;
};
// the scan of one chunk of nq queries: resident slots from the real LDS size, the cut and its scratch by the scan's rules.  A table
// belongs to the query, not to the piece: the cut costs a copy of 1024 M bytes per piece, no build
inline Plan scan_plan(uint32_t num_cu, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uint32_t k) {
    Plan p = {};
    p.lds = lds_bytes(k, nprobe, d, M);
    p.resident = ivs::resident_slots(num_cu, p.lds);
    p.S = ivs::pieces(nq, nprobe, p.resident);
    p.items = nq * p.S;
    p.nslots = ivs::slots(p.items, p.resident);
    p.scratch = ivs::scratch_bytes(nq, p.S, k);
    p.merge_lds = ivs::merge_lds_bytes(p.S, k);
    return p;
}

}  // namespace iaq
}  // namespace vidc
