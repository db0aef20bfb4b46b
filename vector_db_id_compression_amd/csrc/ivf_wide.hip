// ivf_wide.hip -- the IVF list scan for short lists of up to 2048 results (vidc_ivf_scan_wide_dev, vidc_ivf_scan_aq_wide_dev,
// include/vidc.h): a workgroup of four wavefronts per item, a threshold filter into an unsorted LDS buffer, and a bitonic flush.
//
// The result is the narrow scans' (csrc/ivf_scan_ref.h: key, probe row, clamp, strict drop test, label of a position;
// tests/ivf_scan_ref.py and tests/ivf_aq_ref.py are the statement); what the host decides is csrc/ivf_wide_plan.h.  The narrow kernels
// rewrite their whole pool on every trip that keeps a candidate, which is what k <= 256 can pay; here a pool of k keys is touched
// only by a flush.
//
// k_ivf_scan_wide<FORM, V>.  One workgroup of 256 threads per item (query, piece) in a grid-stride loop.
//   * head: the query vector and the probe row go to LDS, the row is mapped by ivs::probe_list and the first mention of a list wins
//     over the WHOLE row (ivf_item_head's rules, 256 entries a pass); the piece is cut afterwards.  PQ8: the 256 threads build the
//     M x 256 table by ivs::pq_entry; AQ: they copy the table k_ivf_aq_lut made, 16 bytes a thread, and every wavefront reduces
//     qn (and cq in front of every list that is not empty) itself by wave_dot: the same bits in all four.
//   * a list is walked in rounds of 256 codes: wavefront w takes the trip of 64 codes at p0 + 64 w with the narrow kernels' per-trip
//     code (ivf_trip_distance, stage_span + aq_distance).  A wavefront behind the list's end takes a trip of no codes: the number
//     of rounds is workgroup-uniform and every barrier sits at workgroup-uniform control flow.
//   * filter: thr = pool[k - 1] (EMPTY until k keys are in), read at the start of the round.  A lane keeps its key when
//     !ivs::key_dropped(key, thr).  thr only falls, so a dropped key is never among the k smallest.  Survivors go, unsorted, to the
//     wavefront's own quarter of the buffer at its own count (ballot, popcount, prefix rank): no atomics, and no wavefront writes
//     where another reads.  The counts are published per round into the even or the odd control row, so a wavefront that is already
//     in the next round does not change what a slower one still reads.
//   * flush (wide_flush): when after a round's barrier some quarter could not take 64 more keys, and at the end of the item.  The
//     quarters are padded with EMPTY, the buffer is sorted by an LDS bitonic network on the 64-bit keys, and wide_merge takes the
//     lower half of (pool, buffer): new[i] = min(pool[i], buffer[K2 - 1 - i]) is bitonic, log2(K2) half-cleaner steps sort it.
//     The buffer's order never reaches the result.
//   * S == 1: the workgroup writes D, the labels and stats.  S > 1: its k keys and two counters go to the run of the item
//     (ivf_carve_runs' layout) and k_ivf_merge_wide, a workgroup per query, starts from run 0 and merges every further run into it
//     with wide_merge: runs are sorted already, and two of them sit in LDS at a time, never S.
// Nothing spins and no workgroup waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_aq_dist.h"
#include "ivf_dist.h"
#include "ivf_merge.h"
#include "ivf_scan_ref.h"
#include "ivf_stage.h"
#include "ivf_wide_plan.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

struct IvWide {
    uint64_t nlist;
    const uint64_t *off;
    uint64_t ntotal;
    const uint8_t *codes;
    uint32_t d, M, cs;  // cs (AQ): bytes of a code row
    const float *cb;    // PQ8: the codebooks; AQ: the tables [nq, M, 256]
    const float *cent;  // AQ: NULL for codes of the raw vector
    uint64_t nq;
    const float *xq;
    uint32_t nprobe;
    const int64_t *probes;
    uint32_t k, K2, B, S, G, logG;
    uint32_t row_bytes, vec_bytes, stage_bytes;
    uint64_t *runs;       // S > 1: [nq, S, k]
    uint32_t *run_stats;  //        [nq, S, 2]
    float *D;
    int64_t *labels;
    uint32_t *stats;
};

// one compare-exchange step of a bitonic network over n keys (a power of two): pair p is (i, i | j); ascending where (i & kk) == 0
// (kk >= n: everywhere).  Ends behind a barrier.
__device__ __forceinline__ void wide_step(uint64_t *keys, uint32_t n, uint32_t kk, uint32_t j, uint32_t tid) {
    for (uint32_t p = tid; p < n / 2u; p += ivw::THREADS) {
        const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u)), l = i | j;
        const uint64_t x = keys[i], y = keys[l];
        if (ivs::key_less(y, x) == ((i & kk) == 0u)) {
            keys[i] = y;
            keys[l] = x;
        }
    }
    __syncthreads();
}

// pool and run: K2 ascending keys each, EMPTY padded -> pool holds the K2 smallest of both, ascending.  Called behind a barrier by
// all 256 threads; ends behind one.
__device__ __forceinline__ void wide_merge(uint64_t *pool, const uint64_t *run, uint32_t K2, uint32_t tid) {
    for (uint32_t i = tid; i < K2; i += ivw::THREADS) {
        const uint64_t r = run[K2 - 1u - i];
        if (ivs::key_less(r, pool[i])) pool[i] = r;
    }
    __syncthreads();
    for (uint32_t j = K2 >> 1; j; j >>= 1) wide_step(pool, K2, K2, j, tid);
}

// the flush: wavefront w holds cnt keys at the start of its quarter of the B buffer keys.  Called by all 256 threads behind a
// barrier; ends behind one, the buffer is free again.
__device__ __forceinline__ void wide_flush(uint64_t *pool, uint64_t *buf, uint32_t K2, uint32_t B, uint32_t cnt, uint32_t tid) {
    const uint32_t Q = B / ivw::WAVES, w = tid >> 6, lane = tid & 63u;
    for (uint32_t i = cnt + lane; i < Q; i += 64) buf[w * Q + i] = ivs::EMPTY;
    __syncthreads();
    for (uint32_t kk = 2; kk <= B; kk <<= 1)
        for (uint32_t j = kk >> 1; j; j >>= 1) wide_step(buf, B, kk, j, tid);
    wide_merge(pool, buf, K2, tid);
}

// FORM FLAT: V components per load (4 or 1).  PQ8: V is W, the bytes of a code load.  AQ: V is unused.
template <int FORM, int V>
__global__ void __launch_bounds__(ivw::THREADS) k_ivf_scan_wide(IvWide a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ivw::lds_bytes
    const uint32_t k = a.k, K2 = a.K2, B = a.B, Q = B / ivw::WAVES, d = a.d, nprobe = a.nprobe;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = rfl(tid >> 6);
    uint64_t *pool = lds, *buf = lds + K2;
    uint32_t *cnts = (uint32_t *)(buf + B);  // [2][WAVES]
    int32_t *row = (int32_t *)((uint8_t *)cnts + ivw::CONTROL_BYTES);
    float *qv = (float *)((uint8_t *)row + a.row_bytes);
    uint8_t *behind = (uint8_t *)qv + a.vec_bytes;
    float *cdist = (float *)behind + w * ivs::TRIP;                     // FLAT
    uint32_t *stage = (uint32_t *)(behind + w * a.stage_bytes);         // AQ
    float *table = (float *)(behind + ivw::WAVES * a.stage_bytes);      // PQ8 (stage_bytes == 0), AQ
    const uint64_t items = a.nq * a.S, total = a.ntotal * a.cs;
    const bool res = a.cent != nullptr;
    uint32_t par = 0;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        // the head of the item: ivf_item_head's rules, 256 entries a pass
        for (uint32_t i = tid; i < d; i += ivw::THREADS) qv[i] = a.xq[q * d + i];
        for (uint32_t j = tid; j < nprobe; j += ivw::THREADS) row[j] = ivs::probe_list(a.probes[q * nprobe + j], a.nlist);
        for (uint32_t i = tid; i < K2; i += ivw::THREADS) pool[i] = ivs::EMPTY;
        __syncthreads();
        for (uint32_t j0 = 0; j0 < nprobe; j0 += ivw::THREADS) {
            const uint32_t j = j0 + tid, end = j0 + ivw::THREADS < nprobe ? j0 + ivw::THREADS : nprobe;
            const int32_t mine = j < nprobe ? row[j] : -1;
            bool dup = false;
            for (uint32_t i = 0; i < end; i++) dup = dup || (i < j && row[i] == mine);
            __syncthreads();
            if (dup && mine >= 0) row[j] = -1;
            __syncthreads();
        }
        float qn = 0.f;
        if (FORM == ivw::PQ8) {
            const uint32_t dsub = d / a.M;
            for (uint32_t e = tid; e < a.M * 256u; e += ivw::THREADS) table[e] = ivs::pq_entry(qv, a.cb, dsub, e >> 8, e & 255u);
        } else if (FORM == ivw::AQ) {
            const uint4 *src = (const uint4 *)(a.cb + q * (uint64_t)a.M * iaq::KSUB);
            for (uint32_t e = tid; e < a.M * (iaq::KSUB / 4u); e += ivw::THREADS) ((uint4 *)table)[e] = src[e];
            qn = wave_dot(qv, qv, d, lane);
        }
        __syncthreads();

        uint32_t nlists = 0, ncodes = 0, cnt = 0;  // cnt: the keys in this wavefront's quarter (wavefront-uniform)
        const uint32_t jb = ivs::piece_begin(nprobe, a.S, s), je = ivs::piece_begin(nprobe, a.S, s + 1u);
        for (uint32_t j = jb; j < je; j++) {
            const int32_t l = (int32_t)rfl((uint32_t)row[j]);
            if (l < 0) continue;
            const ivs::Range r = ivs::list_range(a.off[l], a.off[(uint64_t)l + 1], a.ntotal);
            const uint32_t ra = rfl((uint32_t)r.a), rb = rfl((uint32_t)r.b);  // (a <= b <= ntotal < 2^32)
            nlists++;
            ncodes += rb - ra;
            float cq = 0.f;
            if (FORM == ivw::AQ && res && ra < rb) cq = wave_dot(qv, a.cent + (uint64_t)l * d, d, lane);
            for (uint64_t p0 = ra; p0 < rb; p0 += ivw::ROUND) {  // (workgroup-uniform)
                const uint64_t thr = pool[k - 1u];
                const uint64_t wp = p0 + 64u * w;
                const uint32_t n = wp < rb ? (rb - wp < ivs::TRIP ? (uint32_t)(rb - wp) : ivs::TRIP) : 0u;
                float dist;
                if (FORM == ivw::AQ) {
                    uint32_t head = 0;
                    if (n) head = stage_span(a.codes, total, wp * a.cs, n * a.cs, lane, stage);
                    __syncthreads();
                    dist = lane < n ? aq_distance(stage, head + lane * a.cs, table, a.M, cq, qn, res) : 0.f;
                } else {
                    dist = ivf_trip_distance<FORM, V>(a.codes, wp, n, lane, d, a.M, qv, table, cdist, a.G, a.logG);
                }
                const uint64_t key = lane < n ? ivs::key_make(dist, (uint32_t)(wp + lane)) : ivs::EMPTY;
                const bool keep = lane < n && !ivs::key_dropped(key, thr);
                const uint64_t keepm = __ballot(keep);
                if (keep) buf[w * Q + cnt + mbcnt(keepm)] = key;  // (cnt + 64 <= Q at the start of every round)
                cnt += popc64(keepm);
                if (lane == 0) cnts[par * ivw::WAVES + w] = cnt;
                __syncthreads();
                bool full = false;
                for (uint32_t v = 0; v < ivw::WAVES; v++) full = full || cnts[par * ivw::WAVES + v] + ivs::TRIP > Q;
                par ^= 1u;
                if (full) {  // (workgroup-uniform: every thread read the same four counts)
                    wide_flush(pool, buf, K2, B, cnt, tid);
                    cnt = 0;
                }
            }
        }
        // the end of the item: what the buffer still holds
        if (lane == 0) cnts[par * ivw::WAVES + w] = cnt;
        __syncthreads();
        uint32_t left = 0;
        for (uint32_t v = 0; v < ivw::WAVES; v++) left += cnts[par * ivw::WAVES + v];
        par ^= 1u;
        if (left) wide_flush(pool, buf, K2, B, cnt, tid);

        if (a.S == 1) {
            for (uint32_t i = tid; i < k; i += ivw::THREADS) {
                const uint64_t ki = pool[i];
                a.D[q * k + i] = ki == ivs::EMPTY ? __builtin_inff() : ivs::key_dist(ki);
                a.labels[q * k + i] = ki == ivs::EMPTY ? -1 : ivs::key_label(a.off, a.nlist, ki);
            }
            if (a.stats && tid == 0) {
                a.stats[q * 2] = nlists;
                a.stats[q * 2 + 1] = ncodes;
            }
        } else {
            for (uint32_t i = tid; i < k; i += ivw::THREADS) a.runs[item * k + i] = pool[i];
            if (tid == 0) {
                a.run_stats[item * 2] = nlists;
                a.run_stats[item * 2 + 1] = ncodes;
            }
        }
        __syncthreads();  // (the next item rewrites the pool, the row, the query vector and the table)
    }
}

// a workgroup per query: run 0 of its S sorted runs of k keys, every further run merged into it -> D, labels, stats
__global__ void __launch_bounds__(ivw::THREADS) k_ivf_merge_wide(const uint64_t *__restrict__ runs, const uint32_t *__restrict__ run_stats,
                                                                 uint64_t nq, uint32_t S, uint32_t k, uint32_t K2,
                                                                 const uint64_t *__restrict__ off, uint64_t nlist, float *__restrict__ D,
                                                                 int64_t *__restrict__ labels, uint32_t *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // two runs of K2 keys
    uint64_t *pool = lds, *run = lds + K2;
    const uint32_t tid = threadIdx.x;
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        for (uint32_t i = tid; i < K2; i += ivw::THREADS) pool[i] = i < k ? runs[q * S * k + i] : ivs::EMPTY;
        for (uint32_t s = 1; s < S; s++) {
            for (uint32_t i = tid; i < K2; i += ivw::THREADS) run[i] = i < k ? runs[(q * S + s) * k + i] : ivs::EMPTY;
            __syncthreads();
            wide_merge(pool, run, K2, tid);
        }
        __syncthreads();
        for (uint32_t i = tid; i < k; i += ivw::THREADS) {
            const uint64_t ki = pool[i];
            D[q * k + i] = ki == ivs::EMPTY ? __builtin_inff() : ivs::key_dist(ki);
            labels[q * k + i] = ki == ivs::EMPTY ? -1 : ivs::key_label(off, nlist, ki);
        }
        if (stats && tid == 0) {
            uint32_t nl = 0, nc = 0;
            for (uint32_t s = 0; s < S; s++) {
                nl += run_stats[(q * S + s) * 2];
                nc += run_stats[(q * S + s) * 2 + 1];
            }
            stats[q * 2] = nl;
            stats[q * 2 + 1] = nc;
        }
        __syncthreads();  // (the next query rewrites both runs)
    }
}

typedef void (*WideKernel)(IvWide);
WideKernel wide_kernel(int form, const ivw::Plan &p) {
    if (form == ivw::AQ) return k_ivf_scan_wide<ivw::AQ, 1>;
    if (form == ivw::FLAT) return p.grp.V == 4 ? k_ivf_scan_wide<ivw::FLAT, 4> : k_ivf_scan_wide<ivw::FLAT, 1>;
    switch (p.W) {
        case 16: return k_ivf_scan_wide<ivw::PQ8, 16>;
        case 8: return k_ivf_scan_wide<ivw::PQ8, 8>;
        case 4: return k_ivf_scan_wide<ivw::PQ8, 4>;
        case 2: return k_ivf_scan_wide<ivw::PQ8, 2>;
        default: return k_ivf_scan_wide<ivw::PQ8, 1>;
    }
}

// what a plan fixes of the kernel's arguments
void apply_plan(IvWide &a, const ivw::Plan &p, uint32_t nprobe, uint32_t d) {
    a.K2 = p.K2; a.B = p.buffer; a.S = p.S; a.G = p.grp.G; a.logG = 0;
    while ((1u << a.logG) < a.G) a.logG++;
    a.row_bytes = (uint32_t)ivx::row_bytes(nprobe);
    a.vec_bytes = (uint32_t)ivx::vec_bytes(d);
}

// the scan kernel, a workgroup per resident place, and behind it the merge of a cut call, both on the context's stream
int launch_wide(vidc_ctx *ctx, WideKernel fn, const ivw::Plan &p, const IvWide &a) {
    hipLaunchKernelGGL(fn, dim3(p.nwg), dim3(ivw::THREADS), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    if (p.S > 1) {
        hipLaunchKernelGGL(k_ivf_merge_wide, req_grid(ctx, a.nq, 1), dim3(ivw::THREADS), p.merge_lds, ctx->stream, (const uint64_t *)a.runs,
                           (const uint32_t *)a.run_stats, a.nq, p.S, a.k, p.K2, a.off, a.nlist, a.D, a.labels, a.stats);
        VIDC_HIP(hipGetLastError());
    }
    return VIDC_OK;
}

}  // namespace

extern "C" int vidc_ivf_scan_wide_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                      int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                                      uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D, int64_t *d_labels, uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf wide scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ivs::Args args = {nlist, d_offsets, ntotal, d_codes, code_kind, d, M, d_codebooks, nq, d_xq, nprobe, d_probes, k, d_D, d_labels};
    if (const char *msg = ivw::check_args(args)) {
        set_error("ivf wide scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ivw::Plan p = ivw::make_plan((uint32_t)ctx->num_cu, code_kind, d, M, nq, nprobe, k, (uintptr_t)d_codes, (uintptr_t)d_xq);
    Scratch s_runs;
    if (p.S > 1) VIDC_TRY(s_runs.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the runs go back to the cache)
    IvWide a = {};
    a.nlist = nlist; a.off = d_offsets; a.ntotal = ntotal; a.codes = d_codes; a.d = d; a.M = M; a.cb = d_codebooks; a.nq = nq; a.xq = d_xq;
    a.nprobe = nprobe; a.probes = d_probes; a.k = k;
    apply_plan(a, p, nprobe, d);
    ivf_carve_runs(a, s_runs, nq, p.S, k);
    a.D = d_D; a.labels = d_labels; a.stats = d_stats;
    const WideKernel fn = wide_kernel(code_kind, p);
    VIDC_TRY(ivf_lds_cap(fn, p.lds));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(launch_wide(ctx, fn, p, a));
    VIDC_TRY(t.finish());  // the call's one wait: the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}

extern "C" int vidc_ivf_scan_aq_wide_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                         uint32_t d, uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                                         const float *d_xq, uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D,
                                         int64_t *d_labels, uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf aq wide scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const iaq::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes, k, d_D, d_labels};
    if (const char *msg = ivw::check_aq(args)) {
        set_error("ivf aq wide scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    // the chunks of vidc_ivf_scan_aq_dev: a full chunk and the tail make different plans, the runs of a cut call take the larger
    const uint64_t chunk = iaq::chunk_queries(M), first = nq < chunk ? nq : chunk, tail = nq % chunk;
    const uint32_t num_cu = (uint32_t)ctx->num_cu;
    const ivw::Plan pf = ivw::make_plan(num_cu, ivw::AQ, d, M, first, nprobe, k, 0, 0);
    const ivw::Plan pt = tail && nq > chunk ? ivw::make_plan(num_cu, ivw::AQ, d, M, tail, nprobe, k, 0, 0) : pf;
    const uint64_t run_bytes = pf.scratch > pt.scratch ? pf.scratch : pt.scratch;
    Scratch s_lut, s_runs;
    VIDC_TRY(s_lut.get(ctx, (size_t)iaq::lut_bytes(first, M)));
    if (run_bytes) VIDC_TRY(s_runs.get(ctx, (size_t)run_bytes));
    StreamGuard guard(ctx);  // (an early return waits before the tables and the runs go back to the cache)
    IvWide a = {};
    a.nlist = nlist; a.off = d_offsets; a.ntotal = ntotal; a.codes = d_codes; a.d = d; a.M = M; a.cs = (uint32_t)iaq::code_size(M);
    a.cb = s_lut.as<float>(); a.cent = d_centroids; a.nprobe = nprobe; a.k = k;
    a.stage_bytes = (uint32_t)iaq::stage_bytes(M);
    const WideKernel fn = wide_kernel(ivw::AQ, pf);
    VIDC_TRY(ivf_lds_cap(fn, pf.lds));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    for (uint64_t c = 0; c < iaq::chunks(nq, M); c++) {
        const uint64_t q0 = c * chunk, n = nq - q0 < chunk ? nq - q0 : chunk;
        const ivw::Plan &p = n == first ? pf : pt;
        VIDC_TRY(ivf_aq_launch_lut(ctx, d, M, d_codebooks, n, d_xq + q0 * d, s_lut.as<float>()));
        a.nq = n; a.xq = d_xq + q0 * d; a.probes = d_probes + q0 * nprobe;
        apply_plan(a, p, nprobe, d);
        ivf_carve_runs(a, s_runs, n, p.S, k);
        a.D = d_D + q0 * k; a.labels = d_labels + q0 * k; a.stats = d_stats ? d_stats + q0 * 2 : nullptr;
        VIDC_TRY(launch_wide(ctx, fn, p, a));
    }
    VIDC_TRY(t.finish());  // the call's one wait: the tables and the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
