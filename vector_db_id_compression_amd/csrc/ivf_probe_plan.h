// ivf_probe_plan.h -- what the host decides for vidc_ivf_probe_dev before any device work: the argument checks, the tile sizes, the
// LDS of a workgroup, the resident workgroups, the cut S of the centroid range, the piece bounds, the scratch of the cut and whether
// the staging loads may be 16 bytes wide.  Host only, no HIP runtime: ivf_probe.hip includes it and tests/ivf_probe_plan_test.cpp
// builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_scan_plan.h"

namespace vidc {
namespace ivp {

constexpr uint32_t THREADS = 256;      // four wavefronts
constexpr uint32_t TC = 128;           // centroids of a tile: 32 columns per wavefront
constexpr uint32_t KC = 32;            // components of a staged chunk
constexpr uint32_t LDW = KC + 4;       // floats of a staged row: 16-byte aligned, 16 rows fall into 16 distinct bank groups
constexpr uint32_t DTW = TC + 4;       // floats of a row of the distance tile
constexpr uint32_t MAX_NPROBE = ivs::MAX_K;  // the pool limit
constexpr uint32_t MAX_S = 256;        // pieces of the centroid range
constexpr uint32_t MAX_WG_PER_CU = 8;  // 32 wavefronts of a compute unit / 4

struct Args {
    uint64_t nlist;
    const void *centroids;
    uint32_t d;
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work)
inline const char *check_args(const Args &a) {
    if (a.nq && (!a.centroids || !a.xq || !a.probes)) return "NULL centroid, query or probe array";
    if (a.nprobe < 1 || a.nprobe > MAX_NPROBE) return "1 <= nprobe <= 256";
    if (a.d < 1 || a.d > ivs::MAX_D) return "1 <= d <= 2048";
    if (a.nlist < 1 || a.nlist >= (1ull << 31)) return "1 <= nlist < 2^31";
    if (a.nq >= (1ull << 32)) return "nq must be below 2^32";
    return nullptr;
}

// queries of a tile: 32 while the pools of 32 queries are no larger than the staging buffers, 16 above
inline uint32_t tile_queries(uint32_t nprobe) { return nprobe <= 64 ? 32u : 16u; }

// dynamic LDS of a workgroup, in this order: the pools [TQ][2][nprobe] keys, the survivors' keys [4][64], the two staging buffers
// [2][TQ + TC][LDW] floats, the distance tile [TQ][DTW], the norms [TC + TQ]
inline size_t pool_bytes(uint32_t TQ, uint32_t nprobe) { return (size_t)2 * TQ * nprobe * 8; }
inline size_t lds_bytes(uint32_t TQ, uint32_t nprobe) {
    return pool_bytes(TQ, nprobe) + (size_t)4 * 64 * 8 + (size_t)2 * (TQ + TC) * LDW * 4 + (size_t)TQ * DTW * 4 + (size_t)(TC + TQ) * 4;
}
// (nprobe = 16: 73856 bytes, two workgroups per compute unit; 64: 98432, one; 256, TQ = 16: 118080, one)
inline size_t merge_lds_bytes(uint32_t nprobe) { return (size_t)2 * nprobe * 8 + (size_t)64 * 8; }

inline uint32_t resident_workgroups(uint32_t num_cu, size_t lds) {
    const uint32_t per = ivs::slots_per_cu(lds);
    return (num_cu ? num_cu : 1) * (per > MAX_WG_PER_CU ? MAX_WG_PER_CU : per);
}
inline uint64_t tiles(uint64_t n, uint32_t T) { return (n + T - 1) / T; }
// the cut: the smallest power of two S <= 256 with query tiles * S >= the resident workgroups; a piece holds at least one tile
inline uint32_t pieces(uint64_t qtiles, uint64_t ntiles, uint32_t resident) {
    uint32_t S = 1;
    while (S < MAX_S && (uint64_t)S * 2 <= ntiles && qtiles * S < resident) S *= 2;
    return S;
}
// piece s of S takes the centroid tiles [piece_tile(s), piece_tile(s + 1)), the centroids [piece_begin(s), piece_begin(s + 1))
VIDC_HD inline uint64_t piece_tile(uint64_t ntiles, uint32_t S, uint32_t s) { return (uint64_t)s * ntiles / S; }  // (the kernel's too)
inline uint64_t piece_begin(uint64_t nlist, uint32_t S, uint32_t s) {
    const uint64_t b = piece_tile(tiles(nlist, TC), S, s) * TC;
    return b < nlist ? b : nlist;
}
// context scratch of a cut call: the pieces' sorted keys [nq, S, nprobe]
inline uint64_t scratch_bytes(uint64_t nq, uint32_t S, uint32_t nprobe) { return S > 1 ? nq * S * nprobe * 8 : 0; }
// 16-byte staging loads: every row of both arrays starts on a 16-byte boundary
inline bool vector_loads(uint32_t d, uintptr_t centroids, uintptr_t xq) { return d % 4 == 0 && ((centroids | xq) & 15u) == 0; }

struct Plan {
    uint32_t TQ, S, resident, grid;
    size_t lds, merge_lds;
    uint64_t qtiles, ntiles, items, scratch;
    bool vec;
};
inline Plan make_plan(uint32_t num_cu, uint64_t nlist, uint32_t d, uint64_t nq, uint32_t nprobe, uintptr_t centroids, uintptr_t xq) {
    Plan p;
    p.TQ = tile_queries(nprobe);
    p.lds = lds_bytes(p.TQ, nprobe);
    p.merge_lds = merge_lds_bytes(nprobe);
    p.resident = resident_workgroups(num_cu, p.lds);
    p.qtiles = tiles(nq, p.TQ);
    p.ntiles = tiles(nlist, TC);
    p.S = pieces(p.qtiles, p.ntiles, p.resident);
    p.items = p.qtiles * p.S;
    p.grid = (uint32_t)(p.items < p.resident ? (p.items ? p.items : 1) : p.resident);
    p.scratch = scratch_bytes(nq, p.S, nprobe);
    p.vec = vector_loads(d, centroids, xq);
    return p;
}

}  // namespace ivp
}  // namespace vidc
