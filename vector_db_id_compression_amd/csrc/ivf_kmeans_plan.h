// ivf_kmeans_plan.h -- what the host decides for vidc_ivf_kmeans_step_dev before any device work: the argument checks, whether the
// centroids of a group are held whole in LDS or streamed, the LDS of a workgroup, the resident workgroups, the cut S of the point
// range, the load width, the groups of one update batch, the lanes of a chunk in k_kmeans_partial and the scratch.  Host only, no HIP
// runtime: ivf_kmeans.hip includes it and tests/ivf_kmeans_plan_test.cpp builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_scan_plan.h"

namespace vidc {
namespace ikm {

constexpr uint32_t THREADS = 256;             // four wavefronts
constexpr uint32_t MT = 2;                    // 16-row blocks of a wavefront
constexpr uint32_t TV = 4 * 16 * MT;          // points of a block
constexpr uint32_t TC = 128;                  // centroids of a tile: 8 MFMA column blocks
constexpr uint32_t KC = 32;                   // components of a staged chunk
constexpr uint32_t LDW = KC + 4;              // floats of a staged row: 16-byte aligned, 16 rows fall into 16 distinct bank groups
constexpr uint32_t KM_CHUNK = 256;            // members of one partial sum (part of the result: include/vidc.h)
constexpr uint32_t MAX_DSUB = 2048;
constexpr uint64_t MAX_CLUSTERS = 1ull << 24; // G * k: a sort key
constexpr size_t WHOLE_LDS_MAX = 64u * 1024u; // centroids of a group up to here are held whole (the default cap of a launch)
constexpr uint32_t MAX_WG_PER_CU = 2;         // __launch_bounds__(256, 2)
constexpr uint64_t BATCH_PAIRS = 1ull << 26;  // (group, point) pairs of one update batch, while a group fits: 1 GiB of sort buffers

struct Args {
    uint64_t n;
    const void *x;
    uint32_t ld, G, dsub, k;
    const void *c_in, *c_out;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work)
inline const char *check_args(const Args &a) {
    if (a.n && (!a.x || !a.c_in || !a.c_out)) return "NULL point or centroid array";
    if (a.G < 1 || a.k < 1) return "G >= 1 and k >= 1";
    if (a.dsub < 1 || a.dsub > MAX_DSUB) return "1 <= dsub <= 2048";
    if ((uint64_t)a.G * a.dsub > a.ld) return "G * dsub <= ld";
    if ((uint64_t)a.G * a.k > MAX_CLUSTERS) return "G * k <= 2^24";
    if (a.n >= (1ull << 32)) return "n must be below 2^32";
    if (a.c_out && a.c_out == a.c_in) return "d_c_out must not alias d_c_in";
    return nullptr;
}

VIDC_HD inline uint32_t round4(uint32_t v) { return (v + 3u) & ~3u; }
// floats of a held centroid: round_up(dsub, 4) + 4, the pad columns zero (the encoder's row)
VIDC_HD inline uint32_t row_floats(uint32_t dsub) { return round4(dsub) + 4u; }
inline size_t whole_bytes(uint32_t dsub, uint32_t k) { return (size_t)k * row_floats(dsub) * 4; }
inline bool held_whole(uint32_t dsub, uint32_t k) { return whole_bytes(dsub, k) <= WHOLE_LDS_MAX; }
constexpr size_t STREAM_LDS = (size_t)2 * TC * LDW * 4;  // two staging buffers: 36864 bytes
inline size_t lds_bytes(uint32_t dsub, uint32_t k) { return held_whole(dsub, k) ? whole_bytes(dsub, k) : STREAM_LDS; }
// (k = 256: dsub = 8 -> 12288 held, 32 -> 36864 held, 60 -> 65536 held, 61 -> streamed; k = 1024, dsub = 128 -> streamed)

inline uint32_t resident_workgroups(uint32_t num_cu, size_t lds) {
    const uint32_t per = ivs::slots_per_cu(lds);
    return (num_cu ? num_cu : 1) * (per > MAX_WG_PER_CU ? MAX_WG_PER_CU : per);
}
inline uint64_t tiles(uint64_t n) { return (n + TV - 1) / TV; }
// the cut: the smallest S with G * S >= the resident workgroups; a piece holds at least one block of points
inline uint32_t pieces(uint32_t G, uint64_t ntiles, uint32_t resident) {
    uint64_t S = ((uint64_t)resident + G - 1) / G;
    if (S > ntiles) S = ntiles;
    return (uint32_t)(S ? S : 1);
}
VIDC_HD inline uint64_t piece_tile(uint64_t ntiles, uint32_t S, uint32_t s) { return (uint64_t)s * ntiles / S; }  // (the kernel's too)
// 16-byte loads of points: every group's columns of every row start on a 16-byte boundary; of centroids: every row does
inline bool vector_points(uint32_t ld, uint32_t dsub, uintptr_t x) { return ld % 4 == 0 && dsub % 4 == 0 && (x & 15u) == 0; }
inline bool vector_loads(uint32_t ld, uint32_t dsub, uintptr_t x, uintptr_t c) { return vector_points(ld, dsub, x) && (c & 15u) == 0; }

// the update runs over batches of whole groups: the most groups whose (group, point) pairs stay within BATCH_PAIRS, at least one
inline uint32_t batch_groups(uint64_t n, uint32_t G) {
    const uint64_t gb = n ? BATCH_PAIRS / n : G;
    return (uint32_t)(gb < 1 ? 1 : (gb > G ? G : gb));
}
inline uint32_t key_bits(uint64_t clusters) {  // keys are 0 .. clusters - 1
    uint32_t b = 0;
    while (b < 32u && ((clusters - 1) >> b)) b++;
    return b;
}
// chunks of a batch cannot exceed this: every cluster adds at most one ragged chunk
inline uint64_t chunk_bound(uint64_t pairs, uint64_t clusters) { return pairs / KM_CHUNK + clusters; }

// k_kmeans_partial: a lane owns V consecutive components (4 with 16-byte loads, else 1), a row has `slots` of them; up to 32 slots
// a wavefront serves 64 / bit_ceil(slots) chunks side by side, beyond it one chunk in ceil(slots / 64) passes
struct Lanes {
    uint32_t V, slots, W, side, passes;
};
inline Lanes partial_lanes(uint32_t dsub, bool vec) {
    Lanes l;
    l.V = vec ? 4u : 1u;
    l.slots = (dsub + l.V - 1) / l.V;
    l.W = 64;
    if (l.slots <= 32) {
        l.W = 1;
        while (l.W < l.slots) l.W *= 2;
    }
    l.side = 64u / l.W;
    l.passes = (l.slots + l.W - 1) / l.W;
    return l;
}

// context scratch of a call, bytes: the norms [G, k]; the assignment [G, n] where the caller passes none; per batch of gb groups with
// P = gb * n pairs and L = gb * k clusters: the keys and pair numbers with their double buffers (16 P) and the digit histograms of the
// sort (12 * 256 * ceil(P / 1024) + 8), the bounds, chunk counts and chunk offsets (16 (L + 1)), the chunk table (8 (P / 256 + L + 1))
// and the partials (4 dsub (P / 256 + L))
inline uint64_t scratch_bytes(uint64_t n, uint32_t G, uint32_t dsub, uint32_t k, bool own_assign) {
    const uint64_t gb = batch_groups(n, G), P = gb * n, L = gb * k, cb = chunk_bound(P, L), st = (P + 1023) / 1024;
    return (uint64_t)G * k * 4 + (own_assign ? (uint64_t)G * n * 4 : 0) + 16 * P + 12 * 256 * st + 8 + 16 * (L + 1) + 8 * (cb + 1) + 4 * dsub * cb;
}

struct Plan {
    bool whole, vec;
    size_t lds;
    uint32_t S, resident, grid, gb;
    uint64_t ntiles, items;
    Lanes lanes;
};
inline Plan make_plan(uint32_t num_cu, uint64_t n, uint32_t ld, uint32_t G, uint32_t dsub, uint32_t k, uintptr_t x, uintptr_t c) {
    Plan p;
    p.whole = held_whole(dsub, k);
    p.lds = lds_bytes(dsub, k);
    p.resident = resident_workgroups(num_cu, p.lds);
    p.ntiles = tiles(n);
    p.S = pieces(G, p.ntiles, p.resident);
    p.items = (uint64_t)G * p.S;
    p.grid = (uint32_t)(p.items < p.resident ? p.items : p.resident);
    p.vec = vector_loads(ld, dsub, x, c);
    p.gb = batch_groups(n, G);
    p.lanes = partial_lanes(dsub, vector_points(ld, dsub, x));
    return p;
}

}  // namespace ikm
}  // namespace vidc
