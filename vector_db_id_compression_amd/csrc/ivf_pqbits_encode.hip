// ivf_pqbits_encode.hip -- the PQ encoder for sub-quantisers of 1 .. 12 bits (vidc_ivf_pq_encode_bits_dev, include/vidc.h): the packed
// codes of a vector batch, raw or of the residual x - centroids[assign].  Field m of row i is the smallest j that minimises
// fmaf(-2, r.c_j, |c_j|^2) over the 2^nbits codewords of sub-quantiser m: vidc_ivf_pq_encode_dev's score and tie rule on the same
// float32 MFMA products (v_mfma_f32_16x16x4_f32), so the result is exact on integer grids and the same bits however the batch was cut.
//
// What the host decides (checks, held whole or streamed, LDS, the cut S, load width, scratch) is csrc/ivf_pqbits_encode_plan.h.
//
// k_pqbits_norms.  A thread per (m, j): |c|^2 with fmaf in component order, to scratch.
// k_ivf_pqbits_argmin.  k_kmeans_assign's form: a workgroup of four wavefronts takes items (sub-quantiser m, piece s of the vector
//   range) in a grid-stride loop and walks the piece in blocks of 128 vectors, 32 rows a wavefront.
//   * vectors never touch LDS: lane l loads the components 4 * (l / 16) .. + 3 of a 16-component block of the sub-vector of row
//     l % 16 (+ 16) straight into MFMA A operands; the residual form gathers the centroid row through assign and subtracts in the
//     same registers.  Rows beyond n, rows with an assign outside [0, nlist) and components beyond dsub are zeros.
//   * WHOLE: the ksub codewords of m are staged once per item as [ksub][round_up(dsub, 4) + 4] floats, pad columns zero; a fragment
//     row beyond ksub (ksub < 16) reads row ksub - 1, whose score is never looked at: a padded column cannot win.  Otherwise they
//     stream through two staging buffers in tiles of 128 codewords x 32 components: the loads of step t + 1 are issued before the
//     MFMAs of step t and stored behind them, one barrier a step.
//   * MFMA j of a 16-component block sums the components 4 * q + j, q = 0 .. 3, blocks in ascending order: the order depends on dsub
//     alone, is the same in both forms and is k_ivf_pq_encode's.
//   * score = fmaf(-2, acc, |c|^2); a lane keeps a running (score, j) over its column blocks in ascending j with a strict <, the 16
//     lanes of a row meet in one four-step butterfly where the lower j wins an equal score, and lane 0 of the group stores the index
//     as uint16 idx[row][m] in context scratch (0 for a row whose assign is outside [0, nlist)).
// k_pqbits_pack.  Sub-quantisers m and m + 1 share a byte wherever nbits % 8 != 0, so no (m, piece) item may store code bytes.  A
//   thread per output byte gathers the bits of the fields that overlap its byte from idx and stores it whole: exactly n * code_size
//   bytes, pad bits zero, no atomics.
// Every loop that holds a barrier or a cross-lane operation has a uniform trip count.  Nothing spins; no workgroup waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_pqbits_encode_plan.h"
#include "requests.h"

using namespace vidc;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct IvBitsEncode {
    uint64_t n;
    const float *x;
    uint32_t d, M, dsub, ksub, S;
    const float *pq, *norms;
    uint64_t nlist;
    const float *cent;  // NULL: raw
    const int64_t *assign;
    uint16_t *idx;  // [n, M]
    uint64_t ntiles, items;
};

// components k0 .. k0 + 3 of a row of dsub floats; beyond dsub: zeros
template <bool VEC>
__device__ __forceinline__ v4f pb_load4(const float *row, uint32_t k0, uint32_t dsub) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (k0 < dsub) v = *(const v4f *)(row + k0);  // (dsub % 4 == 0: the four lie inside the row)
    } else {
        if (k0 < dsub) v.x = row[k0];
        if (k0 + 1u < dsub) v.y = row[k0 + 1u];
        if (k0 + 2u < dsub) v.z = row[k0 + 2u];
        if (k0 + 3u < dsub) v.w = row[k0 + 3u];
    }
    return v;
}

__global__ void __launch_bounds__(256) k_pqbits_norms(const float *__restrict__ c, uint32_t words, uint32_t dsub, float *__restrict__ norms) {
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < words; l += gridDim.x * blockDim.x) {
        const float *row = c + (size_t)l * dsub;
        float n2 = 0.f;
        for (uint32_t q = 0; q < dsub; q++) n2 = __builtin_fmaf(row[q], row[q], n2);
        norms[l] = n2;
    }
}

template <bool VEC, bool WHOLE, bool RES>
__global__ void __launch_bounds__(256, 2) k_ivf_pqbits_argmin(IvBitsEncode a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // WHOLE: [ksub][row_floats]; else [2][TC][LDW]
    constexpr uint32_t MT = ikm::MT, TV = ikm::TV, TC = ikm::TC, KC = ikm::KC, LDW = ikm::LDW, NB = TC / 16u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, dsub = a.dsub, k = a.ksub, d = a.d;
    const uint32_t dsubp = ikm::round4(dsub), ldw = ikm::row_floats(dsub), nkb = (dsub + 15u) / 16u, nct = (k + TC - 1u) / TC;
    const uint32_t fr = lane & 15u, fk = (lane >> 4) * 4u;  // MFMA: row fr of a 16-row block, components fk .. fk + 3 of 16

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint32_t m = (uint32_t)(item / a.S), s = (uint32_t)(item % a.S);
        const uint64_t t0 = ikm::piece_tile(a.ntiles, a.S, s), t1 = ikm::piece_tile(a.ntiles, a.S, s + 1u);
        const float *cg = a.pq + (size_t)m * k * dsub, *ng = a.norms + (size_t)m * k, *xs = a.x + (size_t)m * dsub;
        const float *cs = RES ? a.cent + (size_t)m * dsub : nullptr;
        if (WHOLE) {
            __syncthreads();  // (the previous item's blocks have read their last fragment)
            if (VEC) {
                const uint32_t q4 = dsub / 4u;
                for (uint32_t q = tid; q < k * q4; q += 256u) *(v4f *)(lds + (q / q4) * ldw + (q % q4) * 4u) = *(const v4f *)(cg + 4u * q);
            } else {
                for (uint32_t e = tid; e < k * dsub; e += 256u) lds[(e / dsub) * ldw + e % dsub] = cg[e];
            }
            for (uint32_t r = tid; r < k; r += 256u)
                for (uint32_t q = dsub; q < ldw; q++) lds[r * ldw + q] = 0.f;  // the pad columns
            __syncthreads();
        }

        // the A operands of block kb of the vector block: rows tile * 128 + 32 w + 16 i + fr
        auto fetch = [&](uint64_t tile, uint32_t kb, v4f *out) {
#pragma unroll
            for (uint32_t i = 0; i < MT; i++) {
                const uint64_t row = tile * TV + w * 16u * MT + i * 16u + fr;
                v4f v = {0.f, 0.f, 0.f, 0.f};
                if (row < a.n) {
                    if (RES) {
                        const int64_t l = a.assign[row];
                        if (l >= 0 && (uint64_t)l < a.nlist)
                            v = pb_load4<VEC>(xs + row * d, kb + fk, dsub) - pb_load4<VEC>(cs + (uint64_t)l * d, kb + fk, dsub);
                    } else {
                        v = pb_load4<VEC>(xs + row * d, kb + fk, dsub);
                    }
                }
                out[i] = v;
            }
        };

        for (uint64_t tile = t0; tile < t1; tile++) {
            float best[MT][4];
            uint32_t arg[MT][4];
#pragma unroll
            for (uint32_t i = 0; i < MT; i++)
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    best[i][r] = __builtin_inff();
                    arg[i][r] = 0xffffffffu;
                }
            // streamed: thread tid stages the components 4 (tid % 8) .. + 3 of the rows tid / 8 + 32 q, q = 0 .. 3, of a step's chunk
            const uint32_t nch = (dsub + KC - 1u) / KC, sr = tid >> 3, sq = (tid & 7u) * 4u;
            v4f sreg[4];
            auto gload = [&](uint32_t col0, uint32_t ch) {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) {
                    const uint32_t col = col0 + sr + 32u * q;
                    v4f v = {0.f, 0.f, 0.f, 0.f};
                    if (col < k) v = pb_load4<VEC>(cg + (size_t)col * dsub, ch * KC + sq, dsub);
                    sreg[q] = v;
                }
            };
            auto sstore = [&](float *buf) {
#pragma unroll
                for (uint32_t q = 0; q < 4; q++) *(v4f *)(buf + (sr + 32u * q) * LDW + sq) = sreg[q];
            };
            uint32_t st = 0;  // steps of this block so far: step st reads staging buffer st % 2
            if (!WHOLE) {
                gload(0, 0);
                sstore(lds);  // (the barrier behind the last step of the block before this one covers its readers)
                __syncthreads();
            }
            for (uint32_t ct = 0; ct < nct; ct++) {
                const uint32_t c0 = ct * TC;
                const uint32_t nbmax = (k - c0 + 15u) / 16u < NB ? (k - c0 + 15u) / 16u : NB;  // column blocks that hold a codeword
                v4f acc[NB][MT];
#pragma unroll
                for (uint32_t nb = 0; nb < NB; nb++)
#pragma unroll
                    for (uint32_t i = 0; i < MT; i++) acc[nb][i] = (v4f){0.f, 0.f, 0.f, 0.f};

                if (WHOLE) {
                    v4f nxt[MT];
                    fetch(tile, 0, nxt);
                    for (uint32_t kb = 0; kb < nkb * 16u; kb += 16u) {
                        v4f af[MT];
#pragma unroll
                        for (uint32_t i = 0; i < MT; i++) af[i] = nxt[i];
                        if (kb + 16u < nkb * 16u) fetch(tile, kb + 16u, nxt);
                        const uint32_t koff = kb + fk < dsubp ? kb + fk : dsubp;  // (beyond the row: its zero pad)
#pragma unroll
                        for (uint32_t nb = 0; nb < NB; nb++) {
                            if (nb < nbmax) {
                                const uint32_t col = c0 + nb * 16u + fr;
                                const v4f bf = *(const v4f *)(lds + (col < k ? col : k - 1u) * ldw + koff);
#pragma unroll
                                for (uint32_t j = 0; j < 4; j++)
#pragma unroll
                                    for (uint32_t i = 0; i < MT; i++)
                                        acc[nb][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][j], bf[j], acc[nb][i], 0, 0, 0);
                            }
                        }
                    }
                } else {
                    for (uint32_t ch = 0; ch < nch; ch++) {
                        const float *buf = lds + (st & 1u) * TC * LDW;
                        v4f af[2][MT];
                        fetch(tile, ch * KC, af[0]);
                        const bool second = ch * KC + 16u < dsub;
                        if (second) fetch(tile, ch * KC + 16u, af[1]);
                        const bool more = st + 1u < nct * nch;  // (the next step: the next chunk, or chunk 0 of the next tile)
                        if (more) gload(ch + 1u < nch ? c0 : c0 + TC, ch + 1u < nch ? ch + 1u : 0u);
#pragma unroll
                        for (uint32_t h = 0; h < 2; h++) {
                            if (h == 0 || second) {
                                const float *bp = buf + fr * LDW + h * 16u + fk;
#pragma unroll
                                for (uint32_t nb = 0; nb < NB; nb++) {
                                    if (nb < nbmax) {
                                        const v4f bf = *(const v4f *)(bp + nb * 16u * LDW);
#pragma unroll
                                        for (uint32_t j = 0; j < 4; j++)
#pragma unroll
                                            for (uint32_t i = 0; i < MT; i++)
                                                acc[nb][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[h][i][j], bf[j], acc[nb][i], 0, 0, 0);
                                    }
                                }
                            }
                        }
                        if (more) sstore(lds + ((st + 1u) & 1u) * TC * LDW);
                        __syncthreads();
                        st++;
                    }
                }

                // accumulator r of block (nb, i): row 16 i + 4 (lane / 16) + r of the wavefront's 32, codeword c0 + 16 nb + fr
#pragma unroll
                for (uint32_t nb = 0; nb < NB; nb++) {
                    const uint32_t col = c0 + nb * 16u + fr;
                    if (col < k) {  // (a padded column never wins)
                        const float c2 = ng[col];
#pragma unroll
                        for (uint32_t i = 0; i < MT; i++)
#pragma unroll
                            for (uint32_t r = 0; r < 4; r++) {
                                const float sc = __builtin_fmaf(-2.f, acc[nb][i][r], c2);
                                if (sc < best[i][r]) {
                                    best[i][r] = sc;
                                    arg[i][r] = col;
                                }
                            }
                    }
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < MT; i++)
#pragma unroll
                for (uint32_t r = 0; r < 4; r++) {
                    float b = best[i][r];
                    uint32_t j = arg[i][r];
#pragma unroll
                    for (uint32_t o = 1; o < 16; o <<= 1) {
                        const float ob = __shfl_xor(b, o, 64);
                        const uint32_t oj = __shfl_xor(j, o, 64);
                        if (ob < b || (ob == b && oj < j)) {
                            b = ob;
                            j = oj;
                        }
                    }
                    const uint64_t row = tile * TV + w * 16u * MT + i * 16u + (lane >> 4) * 4u + r;
                    if (fr == 0 && row < a.n) {
                        bool ok = j < k;  // (no finite score: 0)
                        if (RES) {
                            const int64_t l = a.assign[row];
                            ok = ok && l >= 0 && (uint64_t)l < a.nlist;
                        }
                        a.idx[row * a.M + m] = ok ? (uint16_t)j : (uint16_t)0;
                    }
                }
        }
    }
}

typedef void (*ArgminKernel)(IvBitsEncode);
template <bool VEC, bool WHOLE>
ArgminKernel pick_res(bool res) { return res ? k_ivf_pqbits_argmin<VEC, WHOLE, true> : k_ivf_pqbits_argmin<VEC, WHOLE, false>; }
ArgminKernel argmin_kernel(bool vec, bool whole, bool res) {
    if (whole) return vec ? pick_res<true, true>(res) : pick_res<false, true>(res);
    return vec ? pick_res<true, false>(res) : pick_res<false, false>(res);
}

// byte e % cs of row e / cs: the bits [8 b, 8 b + 8) of the row's bit string, from the fields that overlap them
__global__ void __launch_bounds__(256) k_pqbits_pack(const uint16_t *__restrict__ idx, uint64_t n, uint32_t M, uint32_t nbits, uint32_t cs,
                                                     uint8_t *__restrict__ codes) {
    const uint64_t total = n * cs;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = e / cs;
        const uint32_t lo = (uint32_t)(e % cs) * 8u, hi = lo + 8u;
        uint32_t byte = 0;
        for (uint32_t m = lo / nbits; m < M && m * nbits < hi; m++) {
            const uint32_t f = idx[row * M + m], at = m * nbits;  // the field's bit 0 is bit `at` of the row
            byte |= at >= lo ? f << (at - lo) : f >> (lo - at);
        }
        codes[e] = (uint8_t)byte;
    }
}

}  // namespace

extern "C" int vidc_ivf_pq_encode_bits_dev(vidc_ctx *ctx, uint64_t n, const float *d_x, uint32_t d, uint32_t M, uint32_t nbits, const float *d_pq,
                                           uint64_t nlist, const float *d_centroids, const int64_t *d_assign, uint8_t *d_codes) {
    if (!ctx) {
        set_error("ivf pq encode bits: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ipbe::Args args = {n, d_x, d, M, nbits, d_pq, nlist, d_centroids, d_assign, d_codes};
    if (const char *msg = ipbe::check_args(args)) {
        set_error("ivf pq encode bits: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!n) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ipbe::Plan p = ipbe::make_plan((uint32_t)ctx->num_cu, n, d, M, nbits, (uintptr_t)d_x, (uintptr_t)d_pq, (uintptr_t)d_centroids);
    Scratch s_work;
    VIDC_TRY(s_work.get(ctx, (size_t)p.scratch));
    StreamGuard guard(ctx);  // (an early return waits before the scratch goes back to the cache)
    float *norms = s_work.as<float>();
    uint16_t *idx = (uint16_t *)((uint8_t *)s_work.p + ipbe::norm_bytes(M, nbits));
    IvBitsEncode a = {};
    a.n = n; a.x = d_x; a.d = d; a.M = M; a.dsub = p.dsub; a.ksub = p.ksub; a.S = p.S; a.pq = d_pq; a.norms = norms; a.nlist = nlist;
    a.cent = d_centroids; a.assign = d_assign; a.idx = idx; a.ntiles = p.ntiles; a.items = p.items;
    const ArgminKernel fn = argmin_kernel(p.vec, p.whole, d_centroids != nullptr);
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(k_pqbits_norms, req_grid(ctx, (uint64_t)M * p.ksub), dim3(256), 0, ctx->stream, d_pq, M * p.ksub, p.dsub, norms);
    VIDC_HIP(hipGetLastError());
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(ikm::THREADS), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_pqbits_pack, req_grid(ctx, n * p.cs), dim3(256), 0, ctx->stream, (const uint16_t *)idx, n, M, nbits, p.cs, d_codes);
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());  // the call's one wait: the scratch goes back to the context's cache
    guard.disarm();
    return VIDC_OK;
}
