// ivf_aq.hip -- the IVF scan over additive-quantiser codes (vidc_ivf_aq_lut_dev, vidc_ivf_scan_aq_dev, include/vidc.h):
// RQ<M>x8_Nfloat, a row of M stage indices and the float32 norm of the stored vector, raw or by_residual.
//
// |xq - y|^2 = |xq|^2 + |y|^2 - 2 <xq, y> with y = centroid + sum of the M codewords: the norm is stored, the inner product is linear
// in the query, so one table of <xq, codeword> per QUERY serves every list and the centroid enters as the scalar <xq, centroid>.
// The rules are the 8-bit scan's (csrc/ivf_scan_ref.h, ivf_merge.h) and are called, not restated; what the host decides, the layout
// and the distance of a row are csrc/ivf_aq_plan.h.
//
// k_ivf_aq_lut.  The tables of a query batch as one GEMM, nq x (M * 256) x d, on v_mfma_f32_16x16x4_f32.  A workgroup of four
// wavefronts takes tiles of 64 queries x 128 table entries in a grid-stride loop; a wavefront owns 32 entries (two column blocks) of
// all 64 queries (four row blocks): eight accumulator quads.
//   * KC = 32 components of the 64 query rows and the 128 codeword rows are staged per pass with guarded 4-byte loads (rows beyond nq
//     and components beyond d are zeros: nothing outside the arrays is read, neither array needs an alignment).  Inside a block of
//     16 components the staging transposes 4 x 4: component 4 t + g is stored at place 4 g + t.  Lane group g = lane / 16 then takes
//     its operands of FOUR consecutive MFMAs with one 16-byte LDS read, and MFMA t of the block multiplies the components
//     4 t .. 4 t + 3: an entry is accumulated over the components in ascending order, four an instruction, on one accumulator.
//   * rows are KC + 4 floats apart: 16-byte aligned, and the 16 rows of a fragment read start in distinct bank groups.
//   * a zero pad adds +0 to the chain, so an entry's bits depend on the query and the codeword alone.
// k_ivf_scan_aq.  One workgroup = one wavefront = one slot, slots take items (query, piece) in a grid-stride loop; the kernel calls
// ivf_item_head, ivf_insert_trip and ivf_write_item (csrc/ivf_scan_steps.h), a trip takes 64 rows, and a cut call is merged by
// k_ivf_merge.  Per item the wavefront copies the query's table (1024 M bytes) from scratch into LDS, 16 bytes
// a lane and pass, and reduces qn = |xq|^2; per probed list that is not empty it reduces cq = <xq, centroid> (wave_dot: a lane's
// components lane, lane + 64, ... with fmaf, then a six-step butterfly -- the order depends on d alone).  The trip's rows go
// through LDS as the aligned 16-byte chunks that cover them (stage_span, ivf_stage.h); a lane walks its M index bytes through the
// table and takes its norm through a window of two aligned LDS words.
// Every loop that holds a barrier or a cross-lane operation has a wavefront-uniform trip count.  Nothing spins and no wavefront or
// workgroup waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_aq_dist.h"
#include "ivf_aq_plan.h"
#include "ivf_merge.h"
#include "ivf_scan_ref.h"
#include "ivf_scan_steps.h"
#include "ivf_stage.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct AqLut {
    const float *cb, *xq;
    float *lut;
    uint64_t nq, tiles;
    uint32_t d, M, ctiles;
};

// rows [r0, r0 + R) of the row-major src (nrows x d), components [k0, k0 + KC) -> dst[R][LDW], transposed 4 x 4 inside every block
// of 16 components; beyond the rows or the components: zeros
template <uint32_t R>
__device__ __forceinline__ void stage_rows(const float *__restrict__ src, uint64_t nrows, uint64_t r0, uint32_t d, uint32_t k0, uint32_t tid,
                                           float *dst) {
    for (uint32_t e = tid; e < R * iaq::KC; e += iaq::LUT_THREADS) {
        const uint32_t r = e / iaq::KC, c = e % iaq::KC, t = (c >> 2) & 3u, g = c & 3u;
        float v = 0.f;
        if (r0 + r < nrows && k0 + c < d) v = src[(r0 + r) * d + k0 + c];
        dst[r * iaq::LDW + (c & ~15u) + 4u * g + t] = v;
    }
}

__global__ void __launch_bounds__(iaq::LUT_THREADS) k_ivf_aq_lut(AqLut a) {
    __shared__ __attribute__((aligned(16))) float As[iaq::TQ * iaq::LDW];
    __shared__ __attribute__((aligned(16))) float Bs[iaq::TN * iaq::LDW];
    constexpr uint32_t TQ = iaq::TQ, TN = iaq::TN, KC = iaq::KC, LDW = iaq::LDW;
    static_assert(sizeof(As) + sizeof(Bs) == iaq::lut_lds_bytes(), "the plan states the LDS of the table GEMM");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, fr = lane & 15u, g = lane >> 4, d = a.d;
    const uint64_t N = (uint64_t)a.M * iaq::KSUB;

    for (uint64_t item = blockIdx.x; item < a.tiles; item += gridDim.x) {
        const uint64_t q0 = item / a.ctiles * TQ, n0 = item % a.ctiles * TN;
        v4f acc[4][2];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
#pragma unroll
            for (uint32_t j = 0; j < 2; j++) acc[i][j] = (v4f){0.f, 0.f, 0.f, 0.f};
        for (uint32_t k0 = 0; k0 < d; k0 += KC) {
            __syncthreads();  // (the fragments of the pass before have been read)
            stage_rows<TQ>(a.xq, a.nq, q0, d, k0, tid, As);
            stage_rows<TN>(a.cb, N, n0, d, k0, tid, Bs);
            __syncthreads();
            for (uint32_t kb = 0; kb < KC && k0 + kb < d; kb += 16u) {
                v4f af[4], bf[2];
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) af[i] = *(const v4f *)(As + (16u * i + fr) * LDW + kb + 4u * g);
#pragma unroll
                for (uint32_t j = 0; j < 2; j++) bf[j] = *(const v4f *)(Bs + (32u * w + 16u * j + fr) * LDW + kb + 4u * g);
#pragma unroll
                for (uint32_t t = 0; t < 4; t++)
#pragma unroll
                    for (uint32_t i = 0; i < 4; i++)
#pragma unroll
                        for (uint32_t j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][t], bf[j][t], acc[i][j], 0, 0, 0);
            }
        }
        // accumulator r of block (i, j): query q0 + 16 i + 4 g + r, entry n0 + 32 w + 16 j + fr
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
#pragma unroll
            for (uint32_t r = 0; r < 4; r++) {
                const uint64_t q = q0 + 16u * i + 4u * g + r;
                if (q < a.nq) {
#pragma unroll
                    for (uint32_t j = 0; j < 2; j++) a.lut[q * N + n0 + 32u * w + 16u * j + fr] = acc[i][j][r];
                }
            }
    }
}

struct IvAq {
    uint64_t nlist;
    const uint64_t *off;
    uint64_t ntotal;
    const uint8_t *codes;
    uint32_t d, M, cs;  // cs: bytes of a code row
    const float *lut;   // [nq, M, 256]
    const float *cent;  // NULL: codes of the raw vector
    uint64_t nq;
    const float *xq;
    uint32_t nprobe;
    const int64_t *probes;
    uint32_t S, k;
    uint32_t pool_bytes, row_bytes, vec_bytes, stage_bytes;
    uint64_t *runs;       // S > 1: [nq, S, k]
    uint32_t *run_stats;  //        [nq, S, 2]
    float *D;
    int64_t *labels;
    uint32_t *stats;
};

// wave_dot and aq_distance: csrc/ivf_aq_dist.h (the wide scan of ivf_wide.hip calls them too)

__global__ void __launch_bounds__(64) k_ivf_scan_aq(IvAq a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of iaq::lds_bytes
    const uint32_t k = a.k, d = a.d, nprobe = a.nprobe, lane = lane_id();
    uint64_t *pool = lds, *other = lds + k, *ckey = lds + 2u * k;
    int32_t *row = (int32_t *)((uint8_t *)lds + a.pool_bytes);
    float *qv = (float *)((uint8_t *)row + a.row_bytes);
    uint32_t *stage = (uint32_t *)((uint8_t *)qv + a.vec_bytes);
    float *table = (float *)((uint8_t *)stage + a.stage_bytes);
    const uint64_t items = a.nq * a.S, total = a.ntotal * a.cs;
    const uint32_t tvec = a.M * (iaq::KSUB / 4u);  // 16-byte groups of a table
    const bool res = a.cent != nullptr;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        ivf_item_head(a.xq, a.probes, a.nlist, q, d, nprobe, lane, qv, row);
        {  // the query's table: built once per query by k_ivf_aq_lut, copied here
            const uint4 *src = (const uint4 *)(a.lut + q * (uint64_t)a.M * iaq::KSUB);
            for (uint32_t e = lane; e < tvec; e += 64) ((uint4 *)table)[e] = src[e];
        }
        for (uint32_t i = lane; i < k; i += 64) pool[i] = ivs::EMPTY;
        const float qn = wave_dot(qv, qv, d, lane);
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
            float cq = 0.f;
            if (res && ra < rb) cq = wave_dot(qv, a.cent + (uint64_t)l * d, d, lane);  // (wavefront-uniform)
            for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                __syncthreads();  // (the lanes have taken the rows of the trip before)
                const uint32_t head = stage_span(a.codes, total, p0 * a.cs, n * a.cs, lane, stage);
                __syncthreads();
                const float dist = lane < n ? aq_distance(stage, head + lane * a.cs, table, a.M, cq, qn, res) : 0.f;
                const uint64_t key = lane < n ? ivs::key_make(dist, (uint32_t)(p0 + lane)) : ivs::EMPTY;
                if (!ivf_insert_trip(key, lane < n, pool, other, ckey, k, lane)) continue;
                uint64_t *t = pool;
                pool = other;
                other = t;
                __syncthreads();
            }
        }

        ivf_write_item(pool, k, lane, q, item, a.S, a.off, a.nlist, nlists, ncodes, a.D, a.labels, a.stats, a.runs, a.run_stats);
        __syncthreads();  // (the next item rewrites the pool, the row, the query vector and the table)
    }
}

}  // namespace

// the tables of nq queries into lut, on the context's stream
int vidc::ivf_aq_launch_lut(vidc_ctx *ctx, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq, float *lut) {
    AqLut a = {};
    a.cb = d_codebooks; a.xq = d_xq; a.lut = lut; a.nq = nq; a.d = d; a.M = M;
    a.ctiles = (uint32_t)iaq::lut_col_tiles(M);
    a.tiles = iaq::lut_tiles(nq, M);
    hipLaunchKernelGGL(k_ivf_aq_lut, dim3(iaq::lut_grid((uint32_t)ctx->num_cu, a.tiles)), dim3(iaq::LUT_THREADS), 0, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

extern "C" int vidc_ivf_aq_lut_dev(vidc_ctx *ctx, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq, float *d_lut) {
    if (!ctx) {
        set_error("ivf aq lut: NULL context");
        return VIDC_ERR_INVALID;
    }
    const iaq::LutArgs args = {d, M, d_codebooks, nq, d_xq, d_lut};
    if (const char *msg = iaq::check_lut(args)) {
        set_error("ivf aq lut: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    StreamGuard guard(ctx);
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(ivf_aq_launch_lut(ctx, d, M, d_codebooks, nq, d_xq, d_lut));
    VIDC_TRY(t.finish());  // the call's one wait
    guard.disarm();
    return VIDC_OK;
}

extern "C" int vidc_ivf_scan_aq_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes, uint32_t d,
                                    uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq, const float *d_xq,
                                    uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D, int64_t *d_labels, uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf aq scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const iaq::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes, k, d_D, d_labels};
    if (const char *msg = iaq::check_scan(args)) {
        set_error("ivf aq scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    // the queries go in chunks whose tables fit the scratch cap; a full chunk and the tail make different plans, the runs of a cut
    // call take the larger of the two
    const uint64_t chunk = iaq::chunk_queries(M), first = nq < chunk ? nq : chunk, tail = nq % chunk;
    const iaq::Plan pf = iaq::scan_plan((uint32_t)ctx->num_cu, d, M, first, nprobe, k);
    const iaq::Plan pt = tail && nq > chunk ? iaq::scan_plan((uint32_t)ctx->num_cu, d, M, tail, nprobe, k) : pf;
    const uint64_t run_bytes = pf.scratch > pt.scratch ? pf.scratch : pt.scratch;
    Scratch s_lut, s_runs;
    VIDC_TRY(s_lut.get(ctx, (size_t)iaq::lut_bytes(first, M)));
    if (run_bytes) VIDC_TRY(s_runs.get(ctx, (size_t)run_bytes));
    StreamGuard guard(ctx);  // (an early return waits before the tables and the runs go back to the cache)
    IvAq a = {};
    a.nlist = nlist; a.off = d_offsets; a.ntotal = ntotal; a.codes = d_codes; a.d = d; a.M = M; a.cs = (uint32_t)iaq::code_size(M);
    a.lut = s_lut.as<float>(); a.cent = d_centroids; a.nprobe = nprobe; a.k = k;
    a.pool_bytes = (uint32_t)ivx::pool_bytes(k); a.row_bytes = (uint32_t)ivx::row_bytes(nprobe); a.vec_bytes = (uint32_t)ivx::vec_bytes(d);
    a.stage_bytes = (uint32_t)iaq::stage_bytes(M);
    VIDC_TRY(ivf_lds_cap(k_ivf_scan_aq, pf.lds));  // (M = 64 with a long probe row or query)
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    for (uint64_t c = 0; c < iaq::chunks(nq, M); c++) {
        const uint64_t q0 = c * chunk, n = nq - q0 < chunk ? nq - q0 : chunk;
        const iaq::Plan &p = n == first ? pf : pt;
        VIDC_TRY(ivf_aq_launch_lut(ctx, d, M, d_codebooks, n, d_xq + q0 * d, s_lut.as<float>()));
        a.nq = n; a.xq = d_xq + q0 * d; a.probes = d_probes + q0 * nprobe; a.S = p.S;
        ivf_carve_runs(a, s_runs, n, p.S, k);
        a.D = d_D + q0 * k; a.labels = d_labels + q0 * k; a.stats = d_stats ? d_stats + q0 * 2 : nullptr;
        VIDC_TRY(ivf_launch_scan(ctx, k_ivf_scan_aq, p, a));
    }
    VIDC_TRY(t.finish());  // the call's one wait: the tables and the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
