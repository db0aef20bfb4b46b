// ivf_scan.hip -- the IVF list scan with deferred id decoding on the device (vidc_ivf_scan_dev, include/vidc.h): every probed list of a
// query is scanned by a wavefront and the k best (distance, list_no << 32 | offset) stay; D and the labels never leave the device.
//
// The rules (key, probe row, clamp of a list range, drop test, insert by rank, S-way merge, label of a position) are
// csrc/ivf_scan_ref.h, which these kernels call and tests/ivf_scan_test.cpp runs serially; what the host decides (checks, slots, the
// cut S, scratch, LDS, lane grouping, load width) is csrc/ivf_scan_plan.h.  tests/ivf_scan_ref.py is the statement of the result.
//
// k_ivf_scan.  One workgroup = one wavefront = one SLOT; slots take items (query, piece) = item / S, item % S in a grid-stride loop.
//   * the query vector and the probe row sit in LDS.  The row is mapped to list numbers (-1: no list) and de-duplicated in place over
//     the WHOLE row, 64 entries a pass: lane j compares its entry with every entry in front of it (uniform trip count); the piece
//     [piece_begin(s), piece_begin(s + 1)) is cut afterwards.
//   * a trip takes 64 codes of a list, whose range was clamped to a <= b <= ntotal, and gives one distance per lane
//     (csrc/ivf_dist.h, shared with ivf_range.hip: the FLAT G-lane butterfly, the PQ8 table walk).  PQ8: the wavefront builds the
//     query's M x 256 table in LDS once per item.
//   * a candidate whose key is not below the pool's last key is dropped by a ballot; the survivors are ranked among themselves by
//     lane reads, against the pool by binary search, and every element is stored at its place in the other pool array.  No private
//     arrays.
//   * S == 1: the wavefront writes D and the labels itself.  S > 1: it writes its k keys and two counters to context scratch, and
//     k_ivf_merge, a wavefront per query, merges the S sorted runs by rank.
// Every loop that holds a cross-lane operation has a wavefront-uniform trip count.  Nothing spins and no wavefront waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_dist.h"
#include "ivf_merge.h"
#include "ivf_scan_plan.h"
#include "ivf_scan_ref.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

struct IvScan {
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
    uint32_t k, S, G, logG;
    uint32_t head_bytes, row_bytes;  // LDS: the pools (PQ8: or the query vector), the probe row
    uint64_t *runs;                  // S > 1: [nq, S, k]
    uint32_t *run_stats;             //        [nq, S, 2]
    float *D;
    int64_t *labels;
    uint32_t *stats;
};

// KIND FLAT: V components per load (4 or 1).  KIND PQ8: V is W, the bytes of a code load.
template <int KIND, int V>
__global__ void __launch_bounds__(64) k_ivf_scan(IvScan a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivs::lds_bytes
    const uint32_t k = a.k, d = a.d, nprobe = a.nprobe, lane = lane_id();
    uint64_t *pool = lds, *other = lds + k, *ckey = lds + 2u * k;
    float *cdist = (float *)(ckey + ivs::TRIP);
    int32_t *row = (int32_t *)((uint8_t *)lds + a.head_bytes);
    float *behind = (float *)((uint8_t *)lds + a.head_bytes + a.row_bytes);
    float *qv = KIND == ivs::PQ8 ? (float *)lds : behind;
    const float *table = behind;  // (PQ8)
    const uint32_t logG = a.logG, G = a.G;
    const uint64_t items = a.nq * a.S;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        for (uint32_t i = lane; i < d; i += 64) qv[i] = a.xq[q * d + i];
        for (uint32_t j = lane; j < nprobe; j += 64) row[j] = ivs::probe_list(a.probes[q * nprobe + j], a.nlist);
        __syncthreads();
        // the duplicate rule over the whole row, in place: a pass clears the later mentions among its 64 entries, so every pass
        // behind it still finds the first one
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
            float *tw = behind;
            const uint32_t dsub = d / a.M;
            for (uint32_t e = lane; e < a.M * 256u; e += 64) tw[e] = ivs::pq_entry(qv, a.cb, dsub, e >> 8, e & 255u);
            __syncthreads();  // (the query vector is done with: the pools take its bytes)
        }
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
            for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                const float dist = ivf_trip_distance<KIND, V>(a.codes, p0, n, lane, d, a.M, qv, table, cdist, G, logG);
                const uint64_t key = lane < n ? ivs::key_make(dist, (uint32_t)(p0 + lane)) : ivs::EMPTY;
                const bool keep = lane < n && !ivs::key_dropped(key, pool[k - 1u]);
                const uint64_t keepm = __ballot(keep);
                const uint32_t C = popc64(keepm);
                if (C == 0) continue;

                // insert by rank: the survivors among themselves, against the pool, everything into the other array
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

// k_ivf_merge, a wavefront per query: csrc/ivf_merge.h (the residual scan of ivf_residual.hip launches it too)

typedef void (*ScanKernel)(IvScan);
ScanKernel scan_kernel(int kind, const ivs::Plan &p) {
    if (kind == ivs::FLAT) return p.grp.V == 4 ? k_ivf_scan<ivs::FLAT, 4> : k_ivf_scan<ivs::FLAT, 1>;
    switch (p.W) {
        case 16: return k_ivf_scan<ivs::PQ8, 16>;
        case 8: return k_ivf_scan<ivs::PQ8, 8>;
        case 4: return k_ivf_scan<ivs::PQ8, 4>;
        case 2: return k_ivf_scan<ivs::PQ8, 2>;
        default: return k_ivf_scan<ivs::PQ8, 1>;
    }
}

}  // namespace

extern "C" int vidc_ivf_scan_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                 int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                                 uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D, int64_t *d_labels, uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivs::Args args = {nlist, d_offsets, ntotal, d_codes, code_kind, d, M, d_codebooks, nq, d_xq, nprobe, d_probes, k, d_D, d_labels};
    if (const char *msg = ivs::check_args(args)) {
        set_error("ivf scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivs::Plan p = ivs::make_plan((uint32_t)ctx->num_cu, code_kind, d, M, nq, nprobe, k, (uintptr_t)d_codes, (uintptr_t)d_xq);
    Scratch s_runs;
    if (p.S > 1) VIDC_TRY(s_runs.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the runs go back to the cache)
    IvScan a = {};
    a.nlist = nlist; a.off = d_offsets; a.ntotal = ntotal; a.codes = d_codes; a.d = d; a.M = M; a.cb = d_codebooks; a.nq = nq; a.xq = d_xq;
    a.nprobe = nprobe; a.probes = d_probes; a.k = k; a.S = p.S; a.G = p.grp.G;
    while ((1u << a.logG) < a.G) a.logG++;
    const size_t pools = (size_t)2 * k * 8 + (size_t)ivs::TRIP * 12, qbytes = ivs::round16((size_t)d * 4);
    a.head_bytes = (uint32_t)(code_kind == ivs::PQ8 && qbytes > pools ? qbytes : pools);
    a.row_bytes = (uint32_t)ivs::round16((size_t)nprobe * 4);
    a.runs = p.S > 1 ? s_runs.as<uint64_t>() : nullptr;
    a.run_stats = p.S > 1 ? (uint32_t *)(s_runs.as<uint64_t>() + ivs::scratch_keys(nq, p.S, k)) : nullptr;
    a.D = d_D; a.labels = d_labels; a.stats = d_stats;
    const ScanKernel fn = scan_kernel(code_kind, p);
    if (p.lds > 64u * 1024u)  // (a PQ table of more than 48 sub-quantisers: above the default cap of a launch)
        VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(fn, dim3(p.nslots), dim3(64), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    if (p.S > 1) {
        hipLaunchKernelGGL(k_ivf_merge, req_grid(ctx, nq, 1), dim3(64), p.merge_lds, ctx->stream, (const uint64_t *)a.runs,
                           (const uint32_t *)a.run_stats, nq, p.S, k, d_offsets, nlist, d_D, d_labels, d_stats);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(t.finish());  // the call's one wait: the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
