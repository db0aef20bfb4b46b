// ivf_probe.hip -- the coarse quantiser on the device (vidc_ivf_probe_dev, include/vidc.h): for every query the nprobe nearest
// centroids in ascending (squared L2 distance, list number) order.  The distance matrix is a GEMM, and the one place in this library
// where matrix instructions fit: float32 MFMA (v_mfma_f32_16x16x4_f32), no narrower format, so that the result is exact on integer
// grids and bit-equal however the work was cut.
//
// What the host decides (checks, TQ, LDS, resident workgroups, the cut S, piece bounds, scratch, load width) is
// csrc/ivf_probe_plan.h; the selection step is csrc/ivf_probe_select.h, with the rules of csrc/ivf_scan_ref.h.
//
// k_ivf_probe.  A workgroup of four wavefronts takes items (query tile, piece) = item / S, item % S in a grid-stride loop.
//   * a piece is streamed in tiles of TC = 128 centroids; a tile is walked KC = 32 components at a time.  A chunk is the query rows
//     [TQ, 32] and the centroid rows [128, 32], staged in LDS in rows of 36 floats.  Thread t loads components 4 * (t % 8) .. + 3 of
//     the rows t / 8 + 32 * i, as one 16-byte load where d and the pointers allow and as four guarded 4-byte loads otherwise: rows
//     beyond the piece or the batch and components beyond d are zeros, which add nothing.  Two buffers: the loads of chunk c + 1 are
//     issued before the MFMAs of chunk c and stored behind them, one barrier a chunk.
//   * wavefront w owns the columns 32 * w .. + 31 of the tile: TQ / 16 x 2 accumulator blocks of 16 x 16.  A lane reads four
//     consecutive components of its row with one 16-byte LDS load and feeds them to four MFMAs, so MFMA j of a 16-component block
//     sums the components 4 * g + j, g = 0 .. 3.  The order is the same for every pair (q, c), every tile and every cut, and the
//     component loop always runs over round_up(d, 32).
//   * the norms are summed from the registers of the staging loads: every lane adds its four squares to a running float32 sum with
//     fmaf, chunk after chunk, and the eight lanes of a row meet in a three-step butterfly at the end.  The order depends on d alone.
//     The queries' norms are summed over the first tile of an item.
//   * the tile ends as max(0, (|q|^2 + |c|^2) - 2 q.c) in a [TQ, 128] float tile in LDS.  Wavefront w owns the queries TQ / 4 * w
//     .. of the tile and runs every one's row through probe_select_trip, 64 columns a trip; both pools of a query stay in LDS for
//     the whole item.
//   * S == 1: the wavefront writes d_probes / d_cdist itself.  S > 1: it writes its nprobe sorted keys to context scratch and
// k_ivf_probe_merge, a wavefront per query, streams the S runs through the same function and writes the result.
// Every loop that holds a barrier or a cross-lane operation has a uniform trip count.  Nothing spins; no workgroup waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_probe_plan.h"
#include "ivf_probe_select.h"
#include "ivf_scan_ref.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct IvProbe {
    uint64_t nlist;
    const float *cent;
    uint32_t d;
    uint64_t nq;
    const float *xq;
    uint32_t nprobe, S;
    uint64_t ntiles, items;
    uint64_t *runs;  // S > 1: [nq, S, nprobe]
    int64_t *probes;
    float *cdist;
};

// components k0 .. k0 + 3 of a row of d floats; beyond d: zeros
template <bool VEC>
__device__ __forceinline__ v4f load4(const float *row, uint32_t k0, uint32_t d) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (k0 < d) v = *(const v4f *)(row + k0);  // (d % 4 == 0: the four lie inside the row)
    } else {
        if (k0 < d) v.x = row[k0];
        if (k0 + 1u < d) v.y = row[k0 + 1u];
        if (k0 + 2u < d) v.z = row[k0 + 2u];
        if (k0 + 3u < d) v.w = row[k0 + 3u];
    }
    return v;
}
__device__ __forceinline__ float add_squares(float s, v4f v) {
    s = __builtin_fmaf(v.x, v.x, s);
    s = __builtin_fmaf(v.y, v.y, s);
    s = __builtin_fmaf(v.z, v.z, s);
    return __builtin_fmaf(v.w, v.w, s);
}
// the sum over the eight lanes of a row: every lane ends with the same value
__device__ __forceinline__ float row_sum8(float s) {
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    return s;
}
__device__ __forceinline__ void write_result(const uint64_t *pool, uint32_t k, uint32_t lane, int64_t *probes, float *cdist) {
    for (uint32_t i = lane; i < k; i += 64) {
        const uint64_t key = pool[i];
        probes[i] = key == ivs::EMPTY ? -1 : (int64_t)ivs::key_pos(key);
        if (cdist) cdist[i] = key == ivs::EMPTY ? __builtin_inff() : ivs::key_dist(key);
    }
}

template <int TQ, bool VEC>
__global__ void __launch_bounds__(256) k_ivf_probe(IvProbe a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivp::lds_bytes
    constexpr uint32_t MT = TQ / 16, QW = TQ / 4, TC = ivp::TC, KC = ivp::KC, LDW = ivp::LDW, DTW = ivp::DTW;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, k = a.nprobe, d = a.d;
    uint64_t *pools = lds + (size_t)w * QW * 2u * k;  // this wavefront's queries: [QW][2][k]
    uint64_t *ckey = lds + (size_t)2 * TQ * k + w * 64u;
    float *stage = (float *)(lds + (size_t)2 * TQ * k + 256u);
    float *tile = stage + 2u * (TQ + TC) * LDW;
    float *cnorm = tile + TQ * DTW, *qnorm = cnorm + TC;
    const uint32_t nch = (d + KC - 1u) / KC;
    const uint32_t lr = tid >> 3, lc = (tid & 7u) * 4u;      // staging: row lr (+ 32 i), components lc .. lc + 3 of the chunk
    const uint32_t fr = lane & 15u, fk = (lane >> 4) * 4u;   // MFMA: row fr of a 16-row block, components fk .. fk + 3 of 16
    const bool loads_q = TQ == 32 || tid < 128u;

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint64_t q0 = item / a.S * TQ;
        const uint32_t s = (uint32_t)(item % a.S);
        const uint64_t cb = ivp::piece_tile(a.ntiles, a.S, s) * TC, ce_ = ivp::piece_tile(a.ntiles, a.S, s + 1u) * TC;
        const uint64_t ce = ce_ < a.nlist ? ce_ : a.nlist;
        for (uint32_t i = lane; i < QW * 2u * k; i += 64) pools[i] = ivs::EMPTY;
        wave_lds_sync();
        uint32_t cur = 0;  // bit ql: which of the two pools of this wavefront's query ql holds its keys
        float qacc = 0.f;

        for (uint64_t c0 = cb; c0 < ce; c0 += TC) {
            const bool first = c0 == cb;
            v4f acc[MT][2];
#pragma unroll
            for (uint32_t m = 0; m < MT; m++) acc[m][0] = acc[m][1] = (v4f){0.f, 0.f, 0.f, 0.f};
            float cacc[4] = {0.f, 0.f, 0.f, 0.f};
            v4f rq = {0.f, 0.f, 0.f, 0.f}, rc[4];

            auto fetch = [&](uint32_t ch) {
                const uint32_t k0 = ch * KC + lc;
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    const uint64_t row = c0 + lr + 32u * i;
                    rc[i] = (v4f){0.f, 0.f, 0.f, 0.f};
                    if (row < ce) rc[i] = load4<VEC>(a.cent + row * d, k0, d);
                }
                if (loads_q) {
                    rq = (v4f){0.f, 0.f, 0.f, 0.f};
                    if (q0 + lr < a.nq) rq = load4<VEC>(a.xq + (q0 + lr) * d, k0, d);
                }
            };
            auto put = [&](uint32_t buf) {
                float *sq = stage + buf * (TQ + TC) * LDW, *sc = sq + TQ * LDW;
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    *(v4f *)(sc + (lr + 32u * i) * LDW + lc) = rc[i];
                    cacc[i] = add_squares(cacc[i], rc[i]);
                }
                if (loads_q) {
                    *(v4f *)(sq + lr * LDW + lc) = rq;
                    if (first) qacc = add_squares(qacc, rq);
                }
            };

            fetch(0);
            put(0);
            __syncthreads();
            for (uint32_t ch = 0; ch < nch; ch++) {
                if (ch + 1u < nch) fetch(ch + 1u);
                const float *sq = stage + (ch & 1u) * (TQ + TC) * LDW, *sc = sq + TQ * LDW + w * 32u * LDW;
#pragma unroll
                for (uint32_t kb = 0; kb < KC; kb += 16) {
                    v4f af[MT], bf[2];
#pragma unroll
                    for (uint32_t m = 0; m < MT; m++) af[m] = *(const v4f *)(sq + (m * 16u + fr) * LDW + kb + fk);
#pragma unroll
                    for (uint32_t n = 0; n < 2; n++) bf[n] = *(const v4f *)(sc + (n * 16u + fr) * LDW + kb + fk);
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++)
#pragma unroll
                        for (uint32_t m = 0; m < MT; m++)
#pragma unroll
                            for (uint32_t n = 0; n < 2; n++)
                                acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[m][j], bf[n][j], acc[m][n], 0, 0, 0);
                }
                if (ch + 1u < nch) put((ch + 1u) & 1u);
                __syncthreads();
            }

#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                const float n2 = row_sum8(cacc[i]);
                if ((tid & 7u) == 0) cnorm[lr + 32u * i] = n2;
            }
            if (first) {
                const float n2 = row_sum8(qacc);
                if (loads_q && (tid & 7u) == 0) qnorm[lr] = n2;
            }
            __syncthreads();
            // accumulator r of block (m, n): query 16 m + 4 (lane / 16) + r of the tile, centroid 32 w + 16 n + lane % 16
#pragma unroll
            for (uint32_t m = 0; m < MT; m++)
#pragma unroll
                for (uint32_t n = 0; n < 2; n++)
#pragma unroll
                    for (uint32_t r = 0; r < 4; r++) {
                        const uint32_t row = m * 16u + (lane >> 4) * 4u + r, col = w * 32u + n * 16u + fr;
                        tile[row * DTW + col] = __builtin_fmaxf(0.f, (qnorm[row] + cnorm[col]) - 2.f * acc[m][n][r]);
                    }
            __syncthreads();

            for (uint32_t ql = 0; ql < QW; ql++) {
                if (q0 + w * QW + ql >= a.nq) continue;  // (the same for the whole wavefront)
                for (uint32_t t = 0; t < TC; t += 64) {
                    const uint64_t c = c0 + t + lane;
                    const uint64_t key = c < ce ? ivs::key_make(tile[(w * QW + ql) * DTW + t + lane], (uint32_t)c) : ivs::EMPTY;
                    uint64_t *pool = pools + (size_t)ql * 2u * k + ((cur >> ql) & 1u) * k;
                    uint64_t *other = pools + (size_t)ql * 2u * k + (((cur >> ql) & 1u) ^ 1u) * k;
                    if (probe_select_trip(key, pool, other, ckey, k, lane)) cur ^= 1u << ql;
                }
            }
            __syncthreads();  // (the next tile rewrites the norms and the distance tile)
        }

        for (uint32_t ql = 0; ql < QW; ql++) {
            const uint64_t q = q0 + w * QW + ql;
            if (q >= a.nq) continue;
            const uint64_t *pool = pools + (size_t)ql * 2u * k + ((cur >> ql) & 1u) * k;
            if (a.S == 1) {
                write_result(pool, k, lane, a.probes + q * k, a.cdist ? a.cdist + q * k : nullptr);
            } else {
                for (uint32_t i = lane; i < k; i += 64) a.runs[(q * a.S + s) * k + i] = pool[i];
            }
        }
        wave_lds_sync();  // (the next item refills this wavefront's pools)
    }
}

// a wavefront per query: the S sorted runs of its pieces, 64 keys a trip, through the selection step -> d_probes, d_cdist
__global__ void __launch_bounds__(64) k_ivf_probe_merge(const uint64_t *__restrict__ runs, uint64_t nq, uint32_t S, uint32_t k,
                                                        int64_t *__restrict__ probes, float *__restrict__ cdist) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // two pools of k keys, the survivors' 64
    const uint32_t lane = lane_id(), n = S * k;
    uint64_t *ckey = lds + 2u * k;
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        uint64_t *pool = lds, *other = lds + k;
        for (uint32_t i = lane; i < k; i += 64) pool[i] = ivs::EMPTY;
        wave_lds_sync();
        for (uint32_t e0 = 0; e0 < n; e0 += 64) {
            const uint64_t key = e0 + lane < n ? runs[q * n + e0 + lane] : ivs::EMPTY;
            if (probe_select_trip(key, pool, other, ckey, k, lane)) {
                uint64_t *t = pool;
                pool = other;
                other = t;
            }
        }
        write_result(pool, k, lane, probes + q * k, cdist ? cdist + q * k : nullptr);
        wave_lds_sync();  // (the next query refills the pool)
    }
}

typedef void (*ProbeKernel)(IvProbe);
ProbeKernel probe_kernel(const ivp::Plan &p) {
    if (p.TQ == 32) return p.vec ? k_ivf_probe<32, true> : k_ivf_probe<32, false>;
    return p.vec ? k_ivf_probe<16, true> : k_ivf_probe<16, false>;
}

}  // namespace

extern "C" int vidc_ivf_probe_dev(vidc_ctx *ctx, uint64_t nlist, const float *d_centroids, uint32_t d, uint64_t nq, const float *d_xq,
                                  uint32_t nprobe, int64_t *d_probes, float *d_cdist) {
    if (!ctx) {
        set_error("ivf probe: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivp::Args args = {nlist, d_centroids, d, nq, d_xq, nprobe, d_probes};
    if (const char *msg = ivp::check_args(args)) {
        set_error("ivf probe: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivp::Plan p = ivp::make_plan((uint32_t)ctx->num_cu, nlist, d, nq, nprobe, (uintptr_t)d_centroids, (uintptr_t)d_xq);
    Scratch s_runs;
    if (p.S > 1) VIDC_TRY(s_runs.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the runs go back to the cache)
    IvProbe a = {};
    a.nlist = nlist; a.cent = d_centroids; a.d = d; a.nq = nq; a.xq = d_xq; a.nprobe = nprobe; a.S = p.S; a.ntiles = p.ntiles;
    a.items = p.items; a.runs = p.S > 1 ? s_runs.as<uint64_t>() : nullptr; a.probes = d_probes; a.cdist = d_cdist;
    const ProbeKernel fn = probe_kernel(p);
    if (p.lds > 64u * 1024u)  // (above the default cap of a launch)
        VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(ivp::THREADS), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    if (p.S > 1) {
        hipLaunchKernelGGL(k_ivf_probe_merge, req_grid(ctx, nq, 1), dim3(64), p.merge_lds, ctx->stream, (const uint64_t *)a.runs, nq, p.S,
                           nprobe, d_probes, d_cdist);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(t.finish());  // the call's one wait: the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
