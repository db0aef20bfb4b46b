// ivf_pq_encode_plan.h -- what the host decides for vidc_ivf_pq_encode_dev before any device work: the argument checks, the LDS of a
// workgroup, the resident workgroups, the cut S of the vector range, the piece bounds and whether loads may be 16 bytes wide.  Host
// only, no HIP runtime: ivf_pq_encode.hip includes it and tests/ivf_pq_encode_plan_test.cpp builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_scan_plan.h"

namespace vidc {
namespace ipe {

constexpr uint32_t THREADS = 256;      // four wavefronts
constexpr uint32_t MT = 2;             // 16-row blocks of a wavefront: 16 x MT accumulator quads = 128 registers
constexpr uint32_t TV = 4 * 16 * MT;   // vectors of a tile
constexpr uint32_t KSUB = 256;         // codewords of a sub-quantiser (8 bits)
constexpr uint32_t MAX_DSUB = 128;     // the codebook of one sub-quantiser has to fit LDS
constexpr uint32_t MAX_WG_PER_CU = 2;  // 256 registers a lane (__launch_bounds__(256, 2)): two wavefronts per SIMD

struct Args {
    uint64_t n;
    const void *x;
    uint32_t d, M;
    const void *pq;
    uint64_t nlist;
    const void *centroids, *assign, *codes;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work)
inline const char *check_args(const Args &a) {
    if (a.n && (!a.x || !a.pq || !a.codes)) return "NULL vector, codebook or code array";
    if (a.centroids && !a.assign) return "centroids without d_assign";
    if (a.centroids && (a.nlist < 1 || a.nlist >= (1ull << 31))) return "1 <= nlist < 2^31";
    if (a.d < 1 || a.d > ivs::MAX_D) return "1 <= d <= 2048";
    if (a.M < 1 || a.d % a.M) return "M >= 1 and d a multiple of M";
    if (a.d / a.M > MAX_DSUB) return "d / M <= 128 (the codebook of a sub-quantiser is held in LDS)";
    if (a.n >= (1ull << 32)) return "n must be below 2^32";
    return nullptr;
}

// floats of a staged codeword: round_up(dsub, 4) + 4, the pad columns zero.  Rows are 16-byte aligned; where dsub rounds to a
// multiple of 8 the stride is an odd number of 16-byte groups, so the 16 rows of a fragment read fall into 16 distinct bank groups
VIDC_HD inline uint32_t row_floats(uint32_t dsub) { return ((dsub + 3u) & ~3u) + 4u; }
// dynamic LDS of a workgroup: the codebook [256][row_floats], behind it the norms [256]
inline size_t lds_bytes(uint32_t dsub) { return (size_t)KSUB * row_floats(dsub) * 4 + (size_t)KSUB * 4; }
// (dsub = 4: 9216 bytes; 8: 13312; 32: 37888; 64: 70656, two workgroups a compute unit up to here; 128: 136192, one)
inline uint32_t resident_workgroups(uint32_t num_cu, size_t lds) {
    const uint32_t per = ivs::slots_per_cu(lds);
    return (num_cu ? num_cu : 1) * (per > MAX_WG_PER_CU ? MAX_WG_PER_CU : per);
}
inline uint64_t tiles(uint64_t n) { return (n + TV - 1) / TV; }
// the cut: the smallest S with M * S >= the resident workgroups; a piece holds at least one tile
inline uint32_t pieces(uint32_t M, uint64_t ntiles, uint32_t resident) {
    uint64_t S = ((uint64_t)resident + M - 1) / M;
    if (S > ntiles) S = ntiles;
    return (uint32_t)(S ? S : 1);
}
// piece s of S takes the tiles [piece_tile(s), piece_tile(s + 1)) of the vector range
VIDC_HD inline uint64_t piece_tile(uint64_t ntiles, uint32_t S, uint32_t s) { return (uint64_t)s * ntiles / S; }  // (the kernel's too)
// 16-byte loads: every sub-vector of every array starts on a 16-byte boundary
inline bool vector_loads(uint32_t d, uint32_t dsub, uintptr_t x, uintptr_t pq, uintptr_t centroids) {
    return d % 4 == 0 && dsub % 4 == 0 && ((x | pq | centroids) & 15u) == 0;
}

struct Plan {
    uint32_t dsub, S, resident, grid;
    size_t lds;
    uint64_t ntiles, items;
    bool vec;
};
inline Plan make_plan(uint32_t num_cu, uint64_t n, uint32_t d, uint32_t M, uintptr_t x, uintptr_t pq, uintptr_t centroids) {
    Plan p;
    p.dsub = d / M;
    p.lds = lds_bytes(p.dsub);
    p.resident = resident_workgroups(num_cu, p.lds);
    p.ntiles = tiles(n);
    p.S = pieces(M, p.ntiles, p.resident);
    p.items = (uint64_t)M * p.S;
    p.grid = (uint32_t)(p.items < p.resident ? p.items : p.resident);
    p.vec = vector_loads(d, p.dsub, x, pq, centroids);
    return p;
}

}  // namespace ipe
}  // namespace vidc
