// ivf_range.hip -- range search over IVF lists on the device (vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev, include/vidc.h):
// every stored vector of a query's probed lists that is closer than the radius, as (distance, list_no << 32 | offset), in probe-row
// order and then offset order.  Two passes with the caller's allocation between them: count -> slot limits, fill -> D and labels.
//
// The rules (slot, hit, place of a hit, write bound) are csrc/ivf_range_ref.h, which the kernel calls and tests/ivf_range_test.cpp
// runs serially; what the host decides (checks, LDS, resident wavefronts, the cut S, load widths) is csrc/ivf_range_plan.h; the probe
// row, the clamp of a list range and the label of a position are the scan's (csrc/ivf_scan_ref.h); the distance of a trip is
// csrc/ivf_dist.h, the function k_ivf_scan calls.  tests/ivf_range_ref.py is the statement of the result.
//
// k_ivf_range<KIND, V, FILL>.  One workgroup = one wavefront; wavefronts take items (query, piece) = item / S, item % S in a
// grid-stride loop, the cut of the scan: a small batch still fills the device, and a PQ table is built once per item.
//   * the query vector, the de-duplicated probe row and the PQ table sit in LDS (the row is de-duplicated over the WHOLE row before
//     the piece is cut, as in k_ivf_scan).  No pools.
//   * a slot is entry j of the row; the pieces of a query own disjoint slots, so there is nothing to merge and no run scratch.
//   * a trip takes 64 codes of the slot's list; the hits are a ballot of dist < radius.
//     count: the popcount goes to the slot's counter; lane 0 stores the uint32 count when the slot is done, 0 for a slot without
//       candidates.  Every one of the nq * nprobe counts is written by exactly one wavefront: the scratch needs no memset.
//     fill: a hit's place is slot_lims[slot] + the hits of the slot's earlier trips + the hits at lower lanes; it is stored only if
//       the place is below slot_lims[slot + 1] and below the capacity.  No atomics: the order does not depend on the cut.
// Every loop that holds a cross-lane operation has a wavefront-uniform trip count.  Nothing spins and no wavefront waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_dist.h"
#include "ivf_range_plan.h"
#include "ivf_range_ref.h"
#include "scan.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

struct IvRange {
    uint64_t nlist;
    const uint64_t *off;
    uint64_t ntotal;
    const uint8_t *codes;
    uint32_t d, M;
    const float *cb;
    uint64_t nq;
    const float *xq;
    uint32_t nprobe;
    const int64_t *probes;
    float radius;
    uint32_t S, G, logG;
    uint32_t head_bytes, row_bytes;  // LDS: the trip's distances (PQ8: the query vector), the probe row
    uint32_t *counts;                // count: [nq * nprobe]
    const uint64_t *lims;            // fill:  [nq * nprobe + 1]
    uint64_t capacity;
    float *D;
    int64_t *labels;
};

// KIND FLAT: V components per load (4 or 1).  KIND PQ8: V is W, the bytes of a code load.
template <int KIND, int V, bool FILL>
__global__ void __launch_bounds__(64) k_ivf_range(IvRange a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivr::lds_bytes
    const uint32_t d = a.d, nprobe = a.nprobe, lane = lane_id();
    float *cdist = (float *)lds;  // (FLAT)
    int32_t *row = (int32_t *)((uint8_t *)lds + a.head_bytes);
    float *behind = (float *)((uint8_t *)lds + a.head_bytes + a.row_bytes);
    float *qv = KIND == ivs::PQ8 ? (float *)lds : behind;
    const float *table = behind;  // (PQ8)
    const uint64_t items = a.nq * a.S;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        for (uint32_t i = lane; i < d; i += 64) qv[i] = a.xq[q * d + i];
        for (uint32_t j = lane; j < nprobe; j += 64) row[j] = ivs::probe_list(a.probes[q * nprobe + j], a.nlist);
        __syncthreads();
        // the duplicate rule over the whole row, in place (k_ivf_scan's passes)
        for (uint32_t j0 = 0; j0 < nprobe; j0 += 64) {
            const uint32_t j = j0 + lane, end = j0 + 64u < nprobe ? j0 + 64u : nprobe;
            const int32_t mine = j < nprobe ? row[j] : -1;
            bool dup = false;
            for (uint32_t i = 0; i < end; i++) dup = dup || (i < j && row[i] == mine);
            __syncthreads();
            if (dup && mine >= 0) row[j] = -1;
            __syncthreads();
        }
        if (KIND == ivs::PQ8) {
            const uint32_t dsub = d / a.M;
            for (uint32_t e = lane; e < a.M * 256u; e += 64) behind[e] = ivs::pq_entry(qv, a.cb, dsub, e >> 8, e & 255u);
            __syncthreads();
        }

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
                for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                    const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                    const float dist = ivf_trip_distance<KIND, V>(a.codes, p0, n, lane, d, a.M, qv, table, cdist, a.G, a.logG);
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

typedef void (*RangeKernel)(IvRange);
template <bool FILL>
RangeKernel range_kernel(int kind, const ivr::Plan &p) {
    if (kind == ivs::FLAT) return p.grp.V == 4 ? k_ivf_range<ivs::FLAT, 4, FILL> : k_ivf_range<ivs::FLAT, 1, FILL>;
    switch (p.W) {
        case 16: return k_ivf_range<ivs::PQ8, 16, FILL>;
        case 8: return k_ivf_range<ivs::PQ8, 8, FILL>;
        case 4: return k_ivf_range<ivs::PQ8, 4, FILL>;
        case 2: return k_ivf_range<ivs::PQ8, 2, FILL>;
        default: return k_ivf_range<ivs::PQ8, 1, FILL>;
    }
}

// the arguments both passes share, and the launch
IvRange range_args(const ivr::Args &g, const ivr::Plan &p, float radius) {
    IvRange a = {};
    a.nlist = g.nlist; a.off = (const uint64_t *)g.offsets; a.ntotal = g.ntotal; a.codes = (const uint8_t *)g.codes; a.d = g.d; a.M = g.M;
    a.cb = (const float *)g.codebooks; a.nq = g.nq; a.xq = (const float *)g.xq; a.nprobe = g.nprobe; a.probes = (const int64_t *)g.probes;
    a.radius = radius; a.S = p.S; a.G = p.grp.G;
    while ((1u << a.logG) < a.G) a.logG++;
    a.head_bytes = (uint32_t)ivr::head_bytes(g.kind, g.d);
    a.row_bytes = (uint32_t)ivr::row_bytes(g.nprobe);
    return a;
}
int range_launch(vidc_ctx *ctx, RangeKernel fn, const ivr::Plan &p, const IvRange &a) {
    if (p.lds > 64u * 1024u)  // (a PQ table of more than 48 sub-quantisers: above the default cap of a launch)
        VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL(fn, dim3(p.nslots), dim3(64), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

}  // namespace

extern "C" int vidc_ivf_range_count_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                        int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                                        uint32_t nprobe, const int64_t *d_probes, float radius, uint64_t *d_slot_lims, uint64_t *total) {
    if (!ctx) {
        set_error("ivf range count: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivr::Args args = {nlist, d_offsets, ntotal, d_codes, code_kind, d, M, d_codebooks, nq, d_xq, nprobe, d_probes, d_slot_lims};
    if (const char *msg = ivr::check_count(args)) {
        set_error("ivf range count: %s", msg);
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
    const ivr::Plan p = ivr::make_plan((uint32_t)ctx->num_cu, code_kind, d, M, nq, nprobe, (uintptr_t)d_codes, (uintptr_t)d_xq);
    const uint32_t nslots = (uint32_t)(nq * nprobe);  // (below 2^32 - 1: checked)
    Scratch s_counts, s_tiles;
    Pinned h_total;
    VIDC_TRY(s_counts.get(ctx, (size_t)ivr::count_bytes(nq, nprobe)));
    if (total) VIDC_TRY(h_total.get(ctx, 8));
    StreamGuard guard(ctx);  // (an early return waits before the counts go back to the cache)
    IvRange a = range_args(args, p, radius);
    a.counts = s_counts.as<uint32_t>();
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(range_launch(ctx, range_kernel<false>(code_kind, p), p, a));
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

extern "C" int vidc_ivf_range_fill_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                       int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                                       uint32_t nprobe, const int64_t *d_probes, float radius, const uint64_t *d_slot_lims,
                                       uint64_t capacity, float *d_D, int64_t *d_labels) {
    if (!ctx) {
        set_error("ivf range fill: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivr::Args args = {nlist, d_offsets, ntotal, d_codes, code_kind, d, M, d_codebooks, nq, d_xq, nprobe, d_probes, d_slot_lims};
    if (const char *msg = ivr::check_fill(args, capacity, d_D, d_labels)) {
        set_error("ivf range fill: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq || !capacity) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivr::Plan p = ivr::make_plan((uint32_t)ctx->num_cu, code_kind, d, M, nq, nprobe, (uintptr_t)d_codes, (uintptr_t)d_xq);
    IvRange a = range_args(args, p, radius);
    a.lims = d_slot_lims; a.capacity = capacity; a.D = d_D; a.labels = d_labels;
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(range_launch(ctx, range_kernel<true>(code_kind, p), p, a));
    VIDC_TRY(t.finish());  // the call's one wait
    return VIDC_OK;
}
