// ivf_pqbits.hip -- the IVF scan over packed PQ codes of 1 .. 12 bits a sub-quantiser (vidc_ivf_scan_pqbits_dev, include/vidc.h): a code
// row is one little-endian bit string of ceil(M * nbits / 8) bytes (PQ8x10: 10 bytes), raw or of (vector - centroids[l]).
//
// The rules are the 8-bit scan's (csrc/ivf_scan_ref.h, ivf_merge.h) and are called, not restated; what the host decides, the layout
// and the table entry are csrc/ivf_pqbits_plan.h.  One workgroup = one wavefront = one slot, slots take items (query, piece) in a
// grid-stride loop; the kernel calls ivf_item_head, ivf_insert_trip and ivf_write_item (csrc/ivf_scan_steps.h), and a cut call is
// merged by k_ivf_merge.  What is this unit's own:
//   * the trip's codes go through LDS.  64 consecutive rows are one span of 64 * code_size bytes that starts on no particular
//     boundary; the wavefront copies the aligned 16-byte chunks that cover it (stage_span), one chunk a lane and pass.  A chunk that
//     is not wholly inside [d_codes, d_codes + ntotal * code_size) -- only the first and the last of the array can be -- is put
//     together from aligned words and, at the very edge, guarded bytes: nothing outside the array is read.
//   * a lane takes its M fields from the staged span through a 64-bit window of two aligned LDS words: field m starts at bit
//     (m * nbits) & 7 of byte (m * nbits) >> 3 of the row, both wavefront-uniform, so only the row's own byte phase varies by lane; a
//     field of at most 12 bits behind a phase of at most 31 bits never leaves the window.  A field indexes 2^nbits entries: always
//     inside the table, whatever the codes hold.
//   * the table has M * 2^nbits entries (build_table).  From 256 codewords on a lane keeps the entries lane + 64 u, u = 0 .. 3, of a
//     block of 256 codewords of one sub-quantiser in flight, as residual_table does; below, one entry at a time.  Either way an entry
//     is ipb::entry: the same subtractions, squares and additions in component order; 16-byte codebook loads under
//     ivx::codebook_vec4.  Raw: once per item from the query vector.  Residual: once per probed list that is not empty, from
//     r = q - centroids[l] in LDS, with the barriers of residual_table.
// Every loop that holds a barrier or a cross-lane operation has a wavefront-uniform trip count.  Nothing spins and no wavefront waits
// for another.
#include "common.h"
#include "host_call.h"
#include "ivf_merge.h"
#include "ivf_pqbits_plan.h"
#include "ivf_scan_ref.h"
#include "ivf_scan_steps.h"
#include "ivf_stage.h"
#include "requests.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::dev;

namespace {

struct IvBits {
    uint64_t nlist;
    const uint64_t *off;
    uint64_t ntotal;
    const uint8_t *codes;
    uint32_t d, M, nbits, cs;  // cs: bytes of a code row
    const float *cb, *cent;    // cent NULL: raw
    uint64_t nq;
    const float *xq;
    uint32_t nprobe;
    const int64_t *probes;
    uint32_t S, vec4, k;
    uint32_t pool_bytes, row_bytes, vec_bytes, stage_bytes;
    uint64_t *runs;       // S > 1: [nq, S, k]
    uint32_t *run_stats;  //        [nq, S, 2]
    float *D;
    int64_t *labels;
    uint32_t *stats;
};

// the distance of the code row that starts at stage byte rs: its M fields through a 64-bit window, the table entries added in m order
__device__ __forceinline__ float bits_distance(const uint32_t *stage, uint32_t rs, const float *table, uint32_t M, uint32_t nbits) {
    const uint32_t ksub = 1u << nbits, mask = ksub - 1u;
    float s = 0.f;
    for (uint32_t m = 0, bit = 0; m < M; m++, bit += nbits) {
        const uint32_t o = rs + (bit >> 3), wi = o >> 2, sh = (o & 3u) * 8u + (bit & 7u);  // (sh <= 31, sh + nbits <= 43)
        const uint64_t win = (uint64_t)stage[wi] | ((uint64_t)stage[wi + 1u] << 32);
        s += table[m * ksub + ((uint32_t)(win >> sh) & mask)];
    }
    return s;
}

// the M x ksub table of the vector v (d floats of LDS, 16-byte aligned): entry (m, c) = ipb::entry.  RES: v = r, which the wavefront
// first writes as qv - centroid.  Holds the barriers of residual_table: every lane of the wavefront calls it.
template <bool RES>
__device__ __forceinline__ void build_table(const float *qv, const float *__restrict__ centroid, const float *__restrict__ codebooks, uint32_t d,
                                            uint32_t M, uint32_t nbits, bool vec4, uint32_t lane, float *r, float *table) {
    __syncthreads();  // (lanes may still read the previous table)
    if (RES) {
        for (uint32_t i = lane; i < d; i += 64) r[i] = qv[i] - centroid[i];
        __syncthreads();
    }
    const float *v = RES ? r : qv;
    const uint32_t dsub = d / M, ksub = 1u << nbits;
    if (ksub >= ipb::BUILD4_KSUB) {
        const uint64_t step = (uint64_t)64 * dsub;
        for (uint32_t m = 0; m < M; m++) {
            const float *vm = v + m * dsub;
            for (uint32_t c0 = 0; c0 < ksub; c0 += 256u) {
                const float *row = codebooks + ((uint64_t)m * ksub + c0 + lane) * dsub;  // entry (m, c0 + lane); + 64 u is 64 u rows on
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                if (vec4) {
                    for (uint32_t i = 0; i < dsub; i += 4) {
                        const float4 y = *(const float4 *)(vm + i);
                        const float4 x0 = *(const float4 *)(row + i), x1 = *(const float4 *)(row + step + i);
                        const float4 x2 = *(const float4 *)(row + 2 * step + i), x3 = *(const float4 *)(row + 3 * step + i);
                        float t;
                        t = y.x - x0.x; s0 += t * t; t = y.y - x0.y; s0 += t * t; t = y.z - x0.z; s0 += t * t; t = y.w - x0.w; s0 += t * t;
                        t = y.x - x1.x; s1 += t * t; t = y.y - x1.y; s1 += t * t; t = y.z - x1.z; s1 += t * t; t = y.w - x1.w; s1 += t * t;
                        t = y.x - x2.x; s2 += t * t; t = y.y - x2.y; s2 += t * t; t = y.z - x2.z; s2 += t * t; t = y.w - x2.w; s2 += t * t;
                        t = y.x - x3.x; s3 += t * t; t = y.y - x3.y; s3 += t * t; t = y.z - x3.z; s3 += t * t; t = y.w - x3.w; s3 += t * t;
                    }
                } else {
                    for (uint32_t i = 0; i < dsub; i++) {
                        const float y = vm[i], x0 = row[i], x1 = row[step + i], x2 = row[2 * step + i], x3 = row[3 * step + i];
                        float t;
                        t = y - x0; s0 += t * t;
                        t = y - x1; s1 += t * t;
                        t = y - x2; s2 += t * t;
                        t = y - x3; s3 += t * t;
                    }
                }
                float *tm = table + m * ksub + c0 + lane;
                tm[0] = s0; tm[64] = s1; tm[128] = s2; tm[192] = s3;
            }
        }
    } else {
        const uint32_t total = M << nbits;
        for (uint32_t e = lane; e < total; e += 64) {
            const uint32_t m = e >> nbits;
            const float *vm = v + m * dsub, *row = codebooks + (uint64_t)e * dsub;  // (e = m * ksub + c)
            float s = 0.f;
            if (vec4) {
                for (uint32_t i = 0; i < dsub; i += 4) {
                    const float4 y = *(const float4 *)(vm + i), x = *(const float4 *)(row + i);
                    float t;
                    t = y.x - x.x; s += t * t; t = y.y - x.y; s += t * t; t = y.z - x.z; s += t * t; t = y.w - x.w; s += t * t;
                }
            } else {
                for (uint32_t i = 0; i < dsub; i++) {
                    const float t = vm[i] - row[i];
                    s += t * t;
                }
            }
            table[e] = s;
        }
    }
    __syncthreads();
}

template <bool RES>
__global__ void __launch_bounds__(64) k_ivf_scan_pqbits(IvBits a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];  // the layout of ipb::lds_bytes
    const uint32_t k = a.k, d = a.d, nprobe = a.nprobe, lane = lane_id();
    uint64_t *pool = lds, *other = lds + k, *ckey = lds + 2u * k;
    int32_t *row = (int32_t *)((uint8_t *)lds + a.pool_bytes);
    float *qv = (float *)((uint8_t *)row + a.row_bytes);
    float *rv = (float *)((uint8_t *)qv + a.vec_bytes);  // (raw: no residual, the span starts here)
    uint32_t *stage = (uint32_t *)((uint8_t *)rv + (RES ? a.vec_bytes : 0u));
    float *table = (float *)((uint8_t *)stage + a.stage_bytes);
    const uint64_t items = a.nq * a.S, total = a.ntotal * a.cs;

    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint64_t q = item / a.S;
        const uint32_t s = (uint32_t)(item % a.S);
        ivf_item_head(a.xq, a.probes, a.nlist, q, d, nprobe, lane, qv, row);
        if (!RES) build_table<false>(qv, nullptr, a.cb, d, a.M, a.nbits, a.vec4 != 0, lane, nullptr, table);
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
            if (RES && ra < rb) build_table<true>(qv, a.cent + (uint64_t)l * d, a.cb, d, a.M, a.nbits, a.vec4 != 0, lane, rv, table);  // (wavefront-uniform)
            for (uint64_t p0 = ra; p0 < rb; p0 += ivs::TRIP) {
                const uint32_t n = rb - p0 < ivs::TRIP ? (uint32_t)(rb - p0) : ivs::TRIP;
                __syncthreads();  // (the lanes have taken the fields of the trip before)
                const uint32_t head = stage_span(a.codes, total, p0 * a.cs, n * a.cs, lane, stage);
                __syncthreads();
                const float dist = lane < n ? bits_distance(stage, head + lane * a.cs, table, a.M, a.nbits) : 0.f;
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

extern "C" int vidc_ivf_scan_pqbits_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                        uint32_t d, uint32_t M, uint32_t nbits, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                                        const float *d_xq, uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D, int64_t *d_labels,
                                        uint32_t *d_stats) {
    if (!ctx) {
        set_error("ivf pqbits scan: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ipb::Args args = {nlist, d_offsets, ntotal, d_codes, d, M, nbits, d_codebooks, d_centroids, nq, d_xq, nprobe, d_probes, k, d_D, d_labels};
    if (const char *msg = ipb::check_scan(args)) {
        set_error("ivf pqbits scan: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!nq) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const bool res = d_centroids != nullptr;
    const ipb::Plan p = ipb::scan_plan((uint32_t)ctx->num_cu, d, M, nbits, res, nq, nprobe, k, (uintptr_t)d_codebooks);
    Scratch s_runs;
    if (p.S > 1) VIDC_TRY(s_runs.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the runs go back to the cache)
    IvBits a = {};
    a.nlist = nlist; a.off = d_offsets; a.ntotal = ntotal; a.codes = d_codes; a.d = d; a.M = M; a.nbits = nbits;
    a.cs = (uint32_t)ipb::code_size(M, nbits); a.cb = d_codebooks; a.cent = d_centroids; a.nq = nq; a.xq = d_xq; a.nprobe = nprobe;
    a.probes = d_probes; a.S = p.S; a.vec4 = p.vec4 ? 1u : 0u; a.k = k;
    a.pool_bytes = (uint32_t)ivx::pool_bytes(k); a.row_bytes = (uint32_t)ivx::row_bytes(nprobe); a.vec_bytes = (uint32_t)ivx::vec_bytes(d);
    a.stage_bytes = (uint32_t)ipb::stage_bytes(M, nbits);
    ivf_carve_runs(a, s_runs, nq, p.S, k);
    a.D = d_D; a.labels = d_labels; a.stats = d_stats;
    void (*fn)(IvBits) = res ? k_ivf_scan_pqbits<true> : k_ivf_scan_pqbits<false>;
    VIDC_TRY(ivf_lds_cap(fn, p.lds));  // (a table of more than about 15000 entries)
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    VIDC_TRY(ivf_launch_scan(ctx, fn, p, a));
    VIDC_TRY(t.finish());  // the call's one wait: the runs go back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
