// graph_search.hip -- best-first search over graph rows as ONE launch (vidc_{rows,compact,ef}_search_dev, include/vidc.h): a wavefront
// per query decodes the rows it expands inside the kernel; the pool, the frontier and the visited set never leave the device.
//
// The rules of a step (key, claim, insert by rank, truncation, loop bound) are csrc/graph_search_ref.h, which this kernel calls and
// tests/graph_search_test.cpp runs serially; what the host decides (checks, slots, scratch, LDS, lane grouping) is
// csrc/graph_search_plan.h.  graph_search.search (Python) is the statement of the result.
//
// One workgroup = one wavefront = one SLOT.  Slot s owns visited set s (N bits of context scratch) and takes queries s, s + slots, ...
//   * visited: cleared by the wavefront in front of EVERY query (8 bytes per lane and store), so neither the previous query of the
//     slot nor what the scratch block held before the call shows through.  A neighbour is claimed with one atomic OR on its 32-bit
//     word: the lane that flips the bit owns the candidate, so a neighbour that a row holds twice counts once whichever lane wins.
//   * rows: lane j takes field j of the expanded node's row, 64 fields a trip.  Raw rows end at the first negative entry, compact
//     rows at the sentinel N (two dwords around the field, as k_compact_rows_decode_wide); an Elias-Fano row is its n <= 64 ids:
//     lane j selects set bit j in the record's <= 4 high words and adds its low field (ef_rank_ref.h), read in place from the arena.
//     A field >= N is dropped before it is used as an index (gs::id_usable).
//   * distances: the query vector sits in LDS; G lanes share one neighbour (plan: gs::group -- d = 16 floats with 16-byte loads is
//     G = 4, 16 neighbours of 64 B each in flight), partial sums meet in a G-lane butterfly.  Which lanes sum which components
//     depends on (d, G) only, so a (query, node) distance has the same bits whatever container or row position it came from.
//   * pool: two arrays of L keys in LDS; the claimed candidates are ranked among themselves by lane reads, against the pool by
//     binary search, and every element is stored at its place in the other array (gs::place_kept).  No private arrays.
//   * termination: the step loop runs to gs::step_bound(N, max_rounds); every loop that holds a cross-lane operation has a
//     wavefront-uniform trip count (P, C, K, G are uniform).  Nothing spins and no wavefront waits for another.
#include "common.h"
#include "ef_plan.h"
#include "ef_rank_ref.h"
#include "graph_search_plan.h"
#include "graph_search_ref.h"
#include "graph_search_views.h"
#include "host_call.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

enum { GS_RAW = 0, GS_COMPACT = 1, GS_EF = 2 };

struct GsRows {
    const void *data;    // raw: int32 [N, K]; compact: the row bytes; Elias-Fano: the arena
    const uint2 *meta;   // Elias-Fano: {universe, n | l << 8} per row
    uint64_t N;
    uint32_t K, bits, stride, LW, HW;
};

// field j0 + lane of the row of `node` -> the id (>= 0) or -1 for "no candidate"; ended: the row ends inside this trip (uniform)
template <int KIND>
__device__ __forceinline__ int64_t gs_field(const GsRows &r, uint32_t node, uint32_t j0, uint32_t lane, bool &ended) {
    const uint32_t j = j0 + lane;
    if (KIND == GS_RAW) {
        const int32_t e = j < r.K ? ((const int32_t *)r.data)[(uint64_t)node * r.K + j] : 0;
        const uint64_t endm = __ballot(j < r.K && e < 0);
        ended = endm != 0;
        const uint32_t n = endm ? ff1(endm) : 64u;
        return (j < r.K && lane < n) ? (int64_t)e : -1;
    } else if (KIND == GS_COMPACT) {
        uint64_t v = ~0ull;
        if (j < r.K) {
            const uint32_t pos = j * r.bits;
            const uintptr_t a = (uintptr_t)((const uint8_t *)r.data + (uint64_t)node * r.stride + (pos >> 3));
            const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)(a & 3u) * 8u + (pos & 7u);
            v = ((((uint64_t)w[1] << 32) | w[0]) >> sh) & ((1ull << r.bits) - 1ull);
        }
        const uint64_t endm = __ballot(j < r.K && v == r.N);
        ended = endm != 0;
        const uint32_t n = endm ? ff1(endm) : 64u;
        return (j < r.K && lane < n) ? (int64_t)v : -1;
    } else {
        ended = true;  // (K <= 64: one trip)
        const uint2 mt = r.meta[node];
        uint32_t n = mt.y & 0xffu;
        n = n < 64u ? n : 64u;
        const uint32_t l = (mt.y >> 8) & 0x1fu;
        const uint64_t *rec = (const uint64_t *)r.data + (uint64_t)node * (r.LW + r.HW);
        uint64_t hw = n ? ef_high_words(n, mt.x, l) : 0;
        hw = hw < r.HW ? hw : r.HW;
        hw = hw < 4u ? hw : 4u;
        int64_t out = -1;
        if (j0 == 0 && lane < n) {
            uint32_t need = lane, pos = 0;
            bool hit = false;
            for (uint32_t w = 0; w < (uint32_t)hw; w++) {  // select1(lane) in the row's own high words
                const uint64_t word = rec[r.LW + w];
                const uint32_t c = efr::popc(word);
                if (!hit && need < c) {
                    pos = w * 64u + efr::select_in_word(word, need);
                    hit = true;
                }
                need -= hit ? 0u : c;
            }
            if (hit) out = (int64_t)(((uint64_t)(pos - lane) << l) | efr::low_field(rec, r.LW, (uint64_t)lane * l, l));
        }
        return out;
    }
}

template <int KIND, int V>
__global__ void __launch_bounds__(64) k_graph_search(GsRows rows, const float *__restrict__ x, uint32_t d, uint64_t nq, const float *__restrict__ xq,
                                                     uint32_t k, uint32_t L, uint32_t entry, uint32_t max_rounds, uint32_t G, uint32_t logG,
                                                     uint64_t *__restrict__ vis_all, uint64_t vis_words, float *__restrict__ D,
                                                     int64_t *__restrict__ I, uint32_t *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of gs::lds_bytes
    uint64_t *pool = lds, *other = lds + L, *ckey = lds + 2u * L;
    uint32_t *cnode = (uint32_t *)(ckey + gs::TRIP);
    float *cdist = (float *)(cnode + gs::TRIP);
    float *qv = (float *)(cdist + gs::TRIP);
    const uint32_t lane = lane_id();
    const uint64_t N = rows.N;
    const uint32_t bound = gs::step_bound(N, max_rounds);
    const uint32_t per = 64u >> logG, g = lane & (G - 1u);
    uint64_t *vis = vis_all + (uint64_t)blockIdx.x * vis_words;
    uint32_t *vis32 = (uint32_t *)vis;

    // distances of cnode[0 .. C) -> cdist (C <= 64, uniform)
    auto distances = [&](uint32_t C) {
        for (uint32_t p0 = 0; p0 < C; p0 += per) {
            const uint32_t idx = p0 + (lane >> logG);
            float s = 0.f;
            if (idx < C) {
                const float *row = x + (uint64_t)cnode[idx] * d;
                if (V == 4) {
                    for (uint32_t i = g * 4u; i < d; i += G * 4u) {
                        const float4 a = *(const float4 *)(row + i), b = *(const float4 *)(qv + i);
                        const float t0 = a.x - b.x, t1 = a.y - b.y, t2 = a.z - b.z, t3 = a.w - b.w;
                        s += t0 * t0;
                        s += t1 * t1;
                        s += t2 * t2;
                        s += t3 * t3;
                    }
                } else {
                    for (uint32_t i = g; i < d; i += G) {
                        const float t = row[i] - qv[i];
                        s += t * t;
                    }
                }
            }
            for (uint32_t o = G >> 1; o; o >>= 1) s += __shfl_xor(s, (int)o, 64);
            if (idx < C && g == 0) cdist[idx] = s;
        }
        __syncthreads();
    };

    for (uint64_t qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        for (uint64_t w = lane; w < vis_words; w += 64) vis[w] = 0ull;
        for (uint32_t i = lane; i < d; i += 64) qv[i] = xq[qi * d + i];
        if (lane == 0) cnode[0] = entry;
        __threadfence();
        __syncthreads();  // (the clear is in memory before the first claim)
        if (lane == 0) (void)atomicOr(&vis32[gs::vis_word(entry)], gs::vis_bit(entry));  // (entry < N: inside the slot)
        distances(1);
        if (lane == 0) pool[0] = gs::key_make(cdist[0], entry);
        __syncthreads();
        uint32_t P = 1, steps = 0, dists = 1;

        for (uint32_t step = 0; step < bound; step++) {
            // the first unexpanded entry
            uint32_t e = P;
            for (uint32_t t = 0; t < P; t += 64) {
                const uint32_t i = t + lane;
                const uint64_t b = __ballot(i < P && !gs::key_expanded(pool[i]));
                if (b) {
                    e = t + ff1(b);
                    break;
                }
            }
            if (e == P) break;
            const uint64_t ke = pool[e];
            __syncthreads();
            if (lane == 0) pool[e] = gs::key_expand(ke);
            const uint32_t node = gs::key_node(ke);
            steps++;
            __syncthreads();

            bool ended = false;
            for (uint32_t j0 = 0; j0 < rows.K && !ended; j0 += gs::TRIP) {
                const int64_t f = gs_field<KIND>(rows, node, j0, lane, ended);
                bool own = false;
                if (f >= 0 && gs::id_usable((uint64_t)f, N)) {
                    const uint32_t v = (uint32_t)f, bit = gs::vis_bit(v);
                    own = gs::claim_won(atomicOr(&vis32[gs::vis_word(v)], bit), bit);
                }
                const uint64_t ownm = __ballot(own);
                const uint32_t C = popc64(ownm);
                if (C == 0) continue;
                if (own) cnode[mbcnt(ownm)] = (uint32_t)f;
                dists += C;
                __syncthreads();
                distances(C);

                // insert by rank: lane c < C holds candidate c
                const uint64_t myk = lane < C ? gs::key_make(cdist[lane], cnode[lane]) : ~0ull;
                const uint32_t mlo = (uint32_t)myk, mhi = (uint32_t)(myk >> 32);
                uint32_t below = 0;
                for (uint32_t c = 0; c < C; c++) below += gs::key_less(rl64(mlo, mhi, c), myk) ? 1u : 0u;
                uint32_t pb = 0;
                if (lane < C) {
                    ckey[below] = myk;  // the candidates in ascending order
                    pb = gs::lower_bound(pool, P, myk);
                }
                __syncthreads();
                for (uint32_t t = 0; t < P; t += 64) {
                    const uint32_t i = t + lane;
                    if (i < P) {
                        const uint64_t pk = pool[i];
                        const uint32_t place = i + gs::lower_bound(ckey, C, pk);
                        if (gs::place_kept(place, L)) other[place] = pk;
                    }
                }
                if (lane < C && gs::place_kept(pb + below, L)) other[pb + below] = myk;
                P = gs::merged_size(P, C, L);
                uint64_t *t = pool;
                pool = other;
                other = t;
                __syncthreads();
            }
        }

        for (uint32_t i = lane; i < k; i += 64) {
            const uint64_t ki = i < P ? pool[i] : 0ull;
            D[qi * k + i] = i < P ? gs::key_dist(ki) : __builtin_inff();
            I[qi * k + i] = i < P ? (int64_t)gs::key_node(ki) : -1;
        }
        if (stats && lane == 0) {
            stats[qi * 2] = steps;
            stats[qi * 2 + 1] = dists;
        }
        __syncthreads();  // (the next query rewrites the pool and the query vector)
    }
}

template <int KIND>
int gs_launch(vidc_ctx *ctx, const char *what, const GsRows &rows, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq, uint32_t k,
              uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I, uint32_t *d_stats) {
    VIDC_HIP(hipSetDevice(ctx->device));
    const uint32_t nslots = std::min<uint32_t>(gs::slots(nq, (uint32_t)ctx->num_cu), req_grid(ctx, nq, 1).x);
    const uint64_t words = gs::vis_words64(rows.N);
    Scratch s_vis;
    VIDC_TRY(s_vis.get(ctx, (size_t)gs::scratch_bytes(nslots, rows.N)));
    StreamGuard guard(ctx);  // (an early return waits before the visited sets go back to the cache)
    const gs::Group grp = gs::group(d, (((uintptr_t)d_x | (uintptr_t)d_xq) & 15u) == 0);
    uint32_t logG = 0;
    while ((1u << logG) < grp.G) logG++;
    const size_t dyn = gs::lds_bytes(L, d);
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    if (grp.V == 4)
        hipLaunchKernelGGL((k_graph_search<KIND, 4>), dim3(nslots), dim3(64), dyn, ctx->stream, rows, d_x, d, nq, d_xq, k, L, entry, max_rounds,
                           grp.G, logG, s_vis.as<uint64_t>(), words, d_D, d_I, d_stats);
    else
        hipLaunchKernelGGL((k_graph_search<KIND, 1>), dim3(nslots), dim3(64), dyn, ctx->stream, rows, d_x, d, nq, d_xq, k, L, entry, max_rounds,
                           grp.G, logG, s_vis.as<uint64_t>(), words, d_D, d_I, d_stats);
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());  // the call's one wait: the visited sets go back to the context's cache
    guard.disarm();
    (void)what;
    return VIDC_OK;
}

// the shared tail of the three entry points, checked before any device work
int gs_check(const char *what, const vidc_ctx *ctx, const void *obj, uint64_t N, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq,
             uint32_t k, uint32_t L, uint32_t entry, uint32_t max_rounds, const float *d_D, const int64_t *d_I) {
    if (!ctx || !obj) {
        set_error("%s search: NULL context or rows", what);
        return VIDC_ERR_INVALID;
    }
    const gs::Args a = {N, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I};
    if (const char *msg = gs::check_args(a)) {
        set_error("%s search: %s", what, msg);
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}

}  // namespace

extern "C" {

int vidc_rows_search_dev(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, const float *d_x, uint32_t d, uint64_t nq,
                         const float *d_xq, uint32_t k, uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I,
                         uint32_t *d_stats) {
    // (the rows of an empty graph may be NULL; entry < N refuses N == 0 anyway)
    VIDC_TRY(gs_check("rows", ctx, (nq && !d_rows) ? nullptr : (const void *)ctx, N, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I));
    if (K == 0) { set_error("rows search: K = 0"); return VIDC_ERR_INVALID; }
    if (!nq) return VIDC_OK;
    const GsRows rows = {d_rows, nullptr, N, K, 0, 0, 0, 0};
    return gs_launch<GS_RAW>(ctx, "rows", rows, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I, d_stats);
}

int vidc_compact_search_dev(vidc_ctx *ctx, const vidc_compact *c, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq, uint32_t k,
                            uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I, uint32_t *d_stats) {
    CompactRowsView v = {};
    if (c) compact_rows_view(c, &v);
    VIDC_TRY(gs_check("compact", ctx, c, v.N, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I));
    if (v.K == 0 || v.K > 4096 || v.bits == 0 || v.bits > 32) {
        set_error("compact search: K=%u / %u bits unsupported (1..4096, 1..32)", v.K, v.bits);
        return VIDC_ERR_UNSUPPORTED;
    }
    if (!nq) return VIDC_OK;
    const GsRows rows = {v.data, nullptr, v.N, v.K, v.bits, v.stride, 0, 0};
    return gs_launch<GS_COMPACT>(ctx, "compact", rows, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I, d_stats);
}

int vidc_ef_search_dev(vidc_ctx *ctx, const vidc_ef *e, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq, uint32_t k, uint32_t L,
                       uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I, uint32_t *d_stats) {
    EfRowsView v = {};
    if (e) ef_rows_view(e, &v);
    if (ctx && e && !v.rows && v.K == 0) {  // (vidc_ef_encode_rows stamps its K on the CSR object it builds for wide rows)
        set_error("elias-fano search: the object holds lists, not graph rows");
        return VIDC_ERR_UNSUPPORTED;
    }
    if (ctx && e && !v.arena) {
        set_error("elias-fano search: rows of more than 64 edges (K=%u) have no arena to search in", v.K);
        return VIDC_ERR_UNSUPPORTED;
    }
    VIDC_TRY(gs_check("elias-fano", ctx, e, v.N, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I));
    if (!nq) return VIDC_OK;
    const GsRows rows = {v.arena_words, v.meta, v.N, v.K < 64u ? (v.K ? v.K : 1u) : 64u, 0, 0, v.LW, v.HW};
    return gs_launch<GS_EF>(ctx, "elias-fano", rows, d_x, d, nq, d_xq, k, L, entry, max_rounds, d_D, d_I, d_stats);
}

}  // extern "C"
