// ivf_residual.hip -- the IVF scan and range search over residual PQ codes on the device (vidc_ivf_scan_residual_dev,
// vidc_ivf_range_count_residual_dev / vidc_ivf_range_fill_residual_dev, include/vidc.h): a code of list l is the 8-bit PQ code of
// (vector - centroids[l]), the kind of index faiss.index_factory(d, "IVF<n>,PQ<M>") builds (by_residual).
//
// The rules are csrc/ivf_residual_ref.h (and through it ivf_scan_ref.h / ivf_range_ref.h), which these kernels call and
// tests/ivf_residual_test.cpp runs serially; what the host decides is csrc/ivf_residual_plan.h; tests/ivf_residual_ref.py is the
// statement of the result.  The organisation is k_ivf_scan's and k_ivf_range's (ivf_scan.hip, ivf_range.hip): one workgroup = one
// wavefront = one slot, slots take items (query, piece) in a grid-stride loop, the probe row is de-duplicated as a whole before the
// cut, a trip takes 64 codes, survivors are inserted by rank, a cut call is merged by k_ivf_merge (ivf_merge.h), the range search
// counts, scans the counts on the device and fills.  What is new sits in front of each probed list:
//   * the query vector stays in LDS for the whole item (it shares no bytes with the pools);
//   * for a valid list whose clamped range is not empty the wavefront writes r = q - centroids[l] to LDS and builds the list's
//     M x 256 table from it (residual_table, csrc/ivf_dist.h: the one function scan, count and fill call); an empty list builds nothing;
//   * the trips run through ivf_trip_distance<PQ8, W>, unchanged.
// A centroid row is read only for a list number the probe rule accepted.  Every loop that holds a barrier or a cross-lane operation
// has a wavefront-uniform trip count.  Nothing spins and no wavefront waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_dist.h"
#include "ivf_merge.h"
#include "ivf_residual_plan.h"
#include "ivf_residual_ref.h"
#include "requests.h"
#include "scan.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

struct IvRes {
    uint64_t nlist;
    const uint64_t *off;
    uint64_t ntotal;
    const uint8_t *codes;
    uint32_t d, M;
    const float *cb, *cent;
    uint64_t nq;
    const float *xq;
    uint32_t nprobe;
    const int64_t *probes;
    uint32_t S, vec4;  // vec4: 16-byte codebook loads (ivx::codebook_vec4)
    uint32_t pool_bytes, row_bytes, vec_bytes;  // LDS: the pools (scan), the probe row, q, r; the table lies behind them
    // scan
    uint32_t k;
    uint64_t *runs;       // S > 1: [nq, S, k]
    uint32_t *run_stats;  //        [nq, S, 2]
    uint32_t *stats;
    // range
    float radius;
    uint32_t *counts;      // count: [nq * nprobe]
    const uint64_t *lims;  // fill:  [nq * nprobe + 1]
    uint64_t capacity;
    float *D;
    int64_t *labels;
};

// the head of an item, shared: the query vector and the probe row go to LDS, the row is mapped to list numbers (-1: no list) and
// de-duplicated in place over the WHOLE row (k_ivf_scan's passes).  Ends behind a barrier.
__device__ __forceinline__ void load_item(const IvRes &a, uint64_t q, uint32_t lane, float *qv, int32_t *row) {
    const uint32_t d = a.d, nprobe = a.nprobe;
    for (uint32_t i = lane; i < d; i += 64) qv[i] = a.xq[q * d + i];
    for (uint32_t j = lane; j < nprobe; j += 64) row[j] = ivs::probe_list(a.probes[q * nprobe + j], a.nlist);
    __syncthreads();
    for (uint32_t j0 = 0; j0 < nprobe; j0 += 64) {
        const uint32_t j = j0 + lane, end = j0 + 64u < nprobe ? j0 + 64u : nprobe;
        const int32_t mine = j < nprobe ? row[j] : -1;
        bool dup = false;
        for (uint32_t i = 0; i < end; i++) dup = dup || (i < j && row[i] == mine);
        __syncthreads();
        if (dup && mine >= 0) row[j] = -1;
        __syncthreads();
    }
}

template <int W>
__global__ void __launch_bounds__(64) k_ivf_scan_residual(IvRes a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivx::scan_lds_bytes
    const uint32_t k = a.k, d = a.d, nprobe = a.nprobe, lane = lane_id();
    uint64_t *pool = lds, *other = lds + k, *ckey = lds + 2u * k;
    int32_t *row = (int32_t *)((uint8_t *)lds + a.pool_bytes);
    float *qv = (float *)((uint8_t *)row + a.row_bytes);
    float *rv = (float *)((uint8_t *)qv + a.vec_bytes);
    float *table = (float *)((uint8_t *)rv + a.vec_bytes);
    const uint64_t items = a.nq * a.S;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        load_item(a, q, lane, qv, row);
        for (uint32_t i = lane; i < k; i += 64) pool[i] = ivs::EMPTY;
        __syncthreads();

        uint32_t nlists = 0, ncodes = 0;
        const uint32_t jb = ivs::piece_begin(nprobe, a.S, s), je = ivs::piece_begin(nprobe, a.S, s + 1u);
        for (uint32_t j = jb; j < je; j++) {
            const int32_t l = (int32_t)rfl((uint32_t)row[j]);
            if (l < 0) continue;
            const ivs::Range r = ivs::list_range(a.off[l], a.off[(uint64_t)l + 1], a.ntotal);
            const uint32_t ra = rfl((uint32_t)r.a), rb = rfl((uint32_t)r.b);  // (a <= b <= ntotal < 2^32)
            nlists++;
            ncodes += rb - ra;
            if (ra < rb) residual_table(qv, a.cent + (uint64_t)l * d, a.cb, d, a.M, a.vec4 != 0, lane, rv, table);  // (wavefront-uniform)
            for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                const float dist = ivf_trip_distance<ivs::PQ8, W>(a.codes, p0, n, lane, d, a.M, qv, table, nullptr, 1u, 0u);
                const uint64_t key = lane < n ? ivs::key_make(dist, (uint32_t)(p0 + lane)) : ivs::EMPTY;
                const bool keep = lane < n && !ivs::key_dropped(key, pool[k - 1u]);
                const uint64_t keepm = __ballot(keep);
                const uint32_t C = popc64(keepm);
                if (C == 0) continue;

                // insert by rank (k_ivf_scan): the survivors among themselves, against the pool, everything into the other array
                const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
                uint32_t below = 0;
                for (uint64_t m = keepm; m; m &= m - 1ull) below += ivs::key_less(rl64(klo, khi, ff1(m)), key) ? 1u : 0u;
                uint32_t pb = 0;
                if (keep) {
                    ckey[below] = key;  // the survivors in ascending order
                    pb = ivs::lower_bound(pool, k, key);
                }
                __syncthreads();
                for (uint32_t t = 0; t < k; t += 64) {
                    const uint32_t i = t + lane;
                    if (i < k) {
                        const uint64_t pk = pool[i];
                        const uint32_t place = i + ivs::lower_bound(ckey, C, pk);
                        if (ivs::place_kept(place, k)) other[place] = pk;
                    }
                }
                if (keep && ivs::place_kept(pb + below, k)) other[pb + below] = key;
                uint64_t *t = pool;
                pool = other;
                other = t;
                __syncthreads();
            }
        }

        if (a.S == 1) {
            for (uint32_t i = lane; i < k; i += 64) {
                const uint64_t ki = pool[i];
                a.D[q * k + i] = ki == ivs::EMPTY ? __builtin_inff() : ivs::key_dist(ki);
                a.labels[q * k + i] = ki == ivs::EMPTY ? -1 : ivs::key_label(a.off, a.nlist, ki);
            }
            if (a.stats && lane == 0) {
                a.stats[q * 2] = nlists;
                a.stats[q * 2 + 1] = ncodes;
            }
        } else {
            for (uint32_t i = lane; i < k; i += 64) a.runs[item * k + i] = pool[i];
            if (lane == 0) {
                a.run_stats[item * 2] = nlists;
                a.run_stats[item * 2 + 1] = ncodes;
            }
        }
        __syncthreads();  // (the next item rewrites the pool, the row and the query vector)
    }
}

template <int W, bool FILL>
__global__ void __launch_bounds__(64) k_ivf_range_residual(IvRes a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivx::range_lds_bytes (no pools)
    const uint32_t d = a.d, nprobe = a.nprobe, lane = lane_id();
    int32_t *row = (int32_t *)lds;
    float *qv = (float *)((uint8_t *)row + a.row_bytes);
    float *rv = (float *)((uint8_t *)qv + a.vec_bytes);
    float *table = (float *)((uint8_t *)rv + a.vec_bytes);
    const uint64_t items = a.nq * a.S;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        load_item(a, q, lane, qv, row);

        const uint32_t jb = ivs::piece_begin(nprobe, a.S, s), je = ivs::piece_begin(nprobe, a.S, s + 1u);
        for (uint32_t j = jb; j < je; j++) {
            const uint64_t slot = ivr::slot_of(q, nprobe, j);
            const int32_t l = (int32_t)rfl((uint32_t)row[j]);
            uint32_t running = 0;  // the slot's hits so far (wavefront-uniform)
            if (l >= 0) {
                const ivs::Range r = ivs::list_range(a.off[l], a.off[(uint64_t)l + 1], a.ntotal);
                const uint32_t ra = rfl((uint32_t)r.a), rb = rfl((uint32_t)r.b);  // (a <= b <= ntotal < 2^32)
                uint64_t base = 0, slot_end = 0;
                if (FILL) {
                    base = rfl64(a.lims[slot]);
                    slot_end = rfl64(a.lims[slot + 1]);
                }
                if (ra < rb) residual_table(qv, a.cent + (uint64_t)l * d, a.cb, d, a.M, a.vec4 != 0, lane, rv, table);  // (wavefront-uniform)
                for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                    const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                    const float dist = ivf_trip_distance<ivs::PQ8, W>(a.codes, p0, n, lane, d, a.M, qv, table, nullptr, 1u, 0u);
                    const bool hit = lane < n && ivr::is_hit(dist, a.radius);
                    const uint64_t hits = __ballot(hit);
                    if (FILL && hit) {
                        const uint64_t place = ivr::hit_place(base, running, mbcnt(hits));
                        if (ivr::place_written(place, slot_end, a.capacity)) {
                            a.D[place] = dist;
                            a.labels[place] = ivs::key_label(a.off, a.nlist, ivs::key_make(dist, (uint32_t)(p0 + lane)));
                        }
                    }
                    running += popc64(hits);
                }
            }
            if (!FILL && lane == 0) a.counts[slot] = running;
        }
        __syncthreads();  // (the next item rewrites the row, the query vector and the table)
    }
}

typedef void (*ResKernel)(IvRes);
ResKernel scan_kernel(uint32_t W) {
    switch (W) {
        case 16: return k_ivf_scan_residual<16>;
        case 8: return k_ivf_scan_residual<8>;
        case 4: return k_ivf_scan_residual<4>;
        case 2: return k_ivf_scan_residual<2>;
        default: return k_ivf_scan_residual<1>;
    }
}
template <bool FILL>
ResKernel range_kernel(uint32_t W) {
    switch (W) {
        case 16: return k_ivf_range_residual<16, FILL>;
        case 8: return k_ivf_range_residual<8, FILL>;
        case 4: return k_ivf_range_residual<4, FILL>;
        case 2: return k_ivf_range_residual<2, FILL>;
        default: return k_ivf_range_residual<1, FILL>;
    }
}

// the arguments every pass shares, and the launch
IvRes common_args(const ivx::Args &g, const ivx::Plan &p) {
    IvRes a = {};
    a.nlist = g.nlist; a.off = (const uint64_t *)g.offsets; a.ntotal = g.ntotal; a.codes = (const uint8_t *)g.codes; a.d = g.d; a.M = g.M;
    a.cb = (const float *)g.codebooks; a.cent = (const float *)g.centroids; a.nq = g.nq; a.xq = (const float *)g.xq; a.nprobe = g.nprobe;
    a.probes = (const int64_t *)g.probes; a.S = p.S; a.vec4 = p.vec4 ? 1u : 0u;
    a.row_bytes = (uint32_t)ivx::row_bytes(g.nprobe);
    a.vec_bytes = (uint32_t)ivx::vec_bytes(g.d);
    return a;
}
int launch(vidc_ctx *ctx, ResKernel fn, const ivx::Plan &p, const IvRes &a) {
    if (p.lds > 64u * 1024u)  // (a table of about 48 sub-quantisers and more: above the default cap of a launch)
        VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL(fn, dim3(p.nslots), dim3(64), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

}  // namespace

extern "C" int vidc_ivf_scan_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                          uint32_t d, uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                                          const float *d_xq, uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D,
                                          int64_t *d_labels, uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf residual scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivx::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes};
    if (const char *msg = ivx::check_scan(args, k, d_D, d_labels)) {
        set_error("ivf residual scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivx::Plan p = ivx::scan_plan((uint32_t)ctx->num_cu, d, M, nq, nprobe, k, (uintptr_t)d_codes, (uintptr_t)d_codebooks);
    Scratch s_runs;
    if (p.S > 1) VIDC_TRY(s_runs.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the runs go back to the cache)
    IvRes a = common_args(args, p);
    a.pool_bytes = (uint32_t)ivx::pool_bytes(k);
    a.k = k;
    a.runs = p.S > 1 ? s_runs.as<uint64_t>() : nullptr;
    a.run_stats = p.S > 1 ? (uint32_t *)(s_runs.as<uint64_t>() + ivs::scratch_keys(nq, p.S, k)) : nullptr;
    a.D = d_D; a.labels = d_labels; a.stats = d_stats;
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(launch(ctx, scan_kernel(p.W), p, a));
    if (p.S > 1) {
        hipLaunchKernelGGL(k_ivf_merge, req_grid(ctx, nq, 1), dim3(64), p.merge_lds, ctx->stream, (const uint64_t *)a.runs,
                           (const uint32_t *)a.run_stats, nq, p.S, k, d_offsets, nlist, d_D, d_labels, d_stats);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(t.finish());  // the call's one wait: the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}

extern "C" int vidc_ivf_range_count_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                                                 const uint8_t *d_codes, uint32_t d, uint32_t M, const float *d_codebooks,
                                                 const float *d_centroids, uint64_t nq, const float *d_xq, uint32_t nprobe,
                                                 const int64_t *d_probes, float radius, uint64_t *d_slot_lims, uint64_t *total) {
    if (!ctx) {
        set_error("ivf residual range count: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivx::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes};
    if (const char *msg = ivx::check_count(args, d_slot_lims)) {
        set_error("ivf residual range count: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) {
        if (d_slot_lims) {
            VIDC_HIP(hipSetDevice(ctx->device));
            VIDC_HIP(hipMemsetAsync(d_slot_lims, 0, 8, ctx->stream));
            VIDC_HIP(vidc_stream_wait(ctx->stream));
        }
        if (total) *total = 0;
        return VIDC_OK;
    }
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivx::Plan p = ivx::range_plan((uint32_t)ctx->num_cu, d, M, nq, nprobe, (uintptr_t)d_codes, (uintptr_t)d_codebooks);
    const uint32_t nslots = (uint32_t)(nq * nprobe);  // (below 2^32 - 1: checked)
    Scratch s_counts, s_tiles;
    Pinned h_total;
    VIDC_TRY(s_counts.get(ctx, (size_t)p.scratch));
    if (total) VIDC_TRY(h_total.get(ctx, 8));
    StreamGuard guard(ctx);  // (an early return waits before the counts go back to the cache)
    IvRes a = common_args(args, p);
    a.radius = radius;
    a.counts = s_counts.as<uint32_t>();
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(launch(ctx, range_kernel<false>(p.W), p, a));
    VIDC_TRY(device_exscan(ctx, s_counts.as<uint32_t>(), nslots, d_slot_lims, s_tiles));
    VIDC_HIP(t.mark());
    if (total) VIDC_HIP(hipMemcpyAsync(h_total.p, d_slot_lims + nslots, 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));  // the call's one wait: the counts go back to the context's cache
    guard.disarm();
    ctx->last_kernel_ms = t.elapsed();
    if (total) {
        std::memcpy(total, h_total.p, 8);
        ctx->d2h_bytes += 8;
    }
    return VIDC_OK;
}

extern "C" int vidc_ivf_range_fill_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                                                const uint8_t *d_codes, uint32_t d, uint32_t M, const float *d_codebooks,
                                                const float *d_centroids, uint64_t nq, const float *d_xq, uint32_t nprobe,
                                                const int64_t *d_probes, float radius, const uint64_t *d_slot_lims, uint64_t capacity,
                                                float *d_D, int64_t *d_labels) {
    if (!ctx) {
        set_error("ivf residual range fill: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivx::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes};
    if (const char *msg = ivx::check_fill(args, d_slot_lims, capacity, d_D, d_labels)) {
        set_error("ivf residual range fill: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq || !capacity) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivx::Plan p = ivx::range_plan((uint32_t)ctx->num_cu, d, M, nq, nprobe, (uintptr_t)d_codes, (uintptr_t)d_codebooks);
    IvRes a = common_args(args, p);
    a.radius = radius;
    a.lims = d_slot_lims; a.capacity = capacity; a.D = d_D; a.labels = d_labels;
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(launch(ctx, range_kernel<true>(p.W), p, a));
    VIDC_TRY(t.finish());  // the call's one wait
    return VIDC_OK;
}
