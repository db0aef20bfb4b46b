// graph_search_plan.h -- what the host decides for vidc_*_search_dev before any device work: the argument checks, the number of
// resident wavefront slots, the scratch of their visited sets, the LDS of one wavefront and the lane grouping of the distance loop.
// Host only, no HIP runtime: graph_search.hip includes it and tests/graph_search_test.cpp builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "graph_search_ref.h"

namespace vidc {
namespace gs {

constexpr uint32_t MAX_SLOTS = 1024;      // resident wavefronts (= visited sets) of one call
constexpr uint32_t SLOTS_PER_CU = 32;     // what req_grid gives a CU

// The tail every entry point shares.  -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work).
struct Args {
    uint64_t N;
    const void *x;
    uint32_t d;
    uint64_t nq;
    const void *xq;
    uint32_t k, L, entry, max_rounds;
    const void *D, *I;
};
inline const char *check_args(const Args &a) {
    if (a.nq >= 0xffffffffull) return "a batch holds fewer than 2^32 - 1 queries";
    if (a.nq && (!a.x || !a.xq || !a.D || !a.I)) return "NULL vector, query, distance or id array";
    if (a.N >= (1ull << 31)) return "N must be below 2^31";
    if (a.k < 1 || a.k > a.L || a.L > MAX_L) return "1 <= k <= L <= 256";
    if (a.d < 1 || a.d > MAX_D) return "1 <= d <= 2048";
    if ((uint64_t)a.entry >= a.N) return "the entry node must be below N";
    return nullptr;
}

// one wavefront (= one workgroup) per slot; a slot takes queries slot, slot + slots, ...
inline uint32_t slots(uint64_t nq, uint32_t num_cu) {
    uint64_t s = (uint64_t)num_cu * SLOTS_PER_CU;
    if (s > MAX_SLOTS) s = MAX_SLOTS;
    if (s > nq) s = nq;
    return (uint32_t)(s ? s : 1);
}
// queries of slot s (the trips of its grid-stride loop)
inline uint64_t slot_queries(uint64_t nq, uint32_t nslots, uint32_t s) { return s < nq ? (nq - 1 - s) / nslots + 1 : 0; }

// visited sets: N bits per slot, in 64-bit words (a lane clears one word per store)
inline uint64_t vis_words64(uint64_t N) { return (N + 63) / 64; }
inline uint64_t scratch_bytes(uint32_t nslots, uint64_t N) { return (uint64_t)nslots * vis_words64(N) * 8; }
// bound stated in include/vidc.h: MAX_SLOTS * ceil(N / 64) * 8 bytes (128 MB at N = 10^6)

// distance loop: G lanes per neighbour, each V components at a time (V = 4: 16-byte loads, when d is a multiple of 4 and both arrays
// are 16-byte aligned).  G = the power of two that covers the vector once, at most 16: a wavefront then has 64 / G neighbours in flight.
struct Group {
    uint32_t G, V;
};
inline Group group(uint32_t d, bool aligned16) {
    Group g;
    g.V = (aligned16 && d % 4 == 0) ? 4u : 1u;
    const uint32_t pieces = (d + g.V - 1) / g.V;
    g.G = 1;
    while (g.G < pieces && g.G < 16) g.G *= 2;
    return g;
}

// dynamic LDS of one wavefront: two pools of L keys (the merge writes the other one), the candidates' keys, their nodes and
// distances, the query vector
inline size_t lds_bytes(uint32_t L, uint32_t d) { return ((size_t)2 * L + TRIP) * 8 + (size_t)TRIP * 8 + (((size_t)d * 4 + 15) & ~(size_t)15); }
// (at most 2 * 256 * 8 + 512 + 512 + 8192 = 13312 bytes: twelve wavefronts per CU even at the limits; L = 64, d = 16: 2112 bytes)

}  // namespace gs
}  // namespace vidc
