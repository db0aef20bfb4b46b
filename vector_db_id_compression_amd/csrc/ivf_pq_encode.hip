// ivf_pq_encode.hip -- the PQ encoder on the device (vidc_ivf_pq_encode_dev, include/vidc.h): the 8-bit codes of a vector batch,
// raw or of the residual x - centroids[assign].  code[i][m] is the smallest j that minimises |c_j|^2 - 2 r.c_j over the 256 codewords
// of sub-quantiser m; the products are float32 MFMA (v_mfma_f32_16x16x4_f32), so the result is exact on integer grids and the same
// bits however the batch was cut.
//
// What the host decides (checks, LDS, resident workgroups, the cut S, piece bounds, load width) is csrc/ivf_pq_encode_plan.h.
//
// k_ivf_pq_encode.  A workgroup of four wavefronts takes items (sub-quantiser m, piece s of the vector range) = item / S, item % S
// in a grid-stride loop.
//   * the codebook of m is staged once per item as [256][round_up(dsub, 4) + 4] floats, pad columns zero; thread j then sums |c_j|^2
//     with fmaf in component order.  Three barriers an item, none inside the vector loop.
//   * the piece is streamed in tiles of 128 vectors, 32 per wavefront.  Vectors never touch LDS: lane l loads the components
//     4 * (l / 16) .. + 3 of every 16-component block of the sub-vector of row l % 16 (+ 16) straight into MFMA A operands, as one
//     16-byte load where the plan allows it and as four guarded 4-byte loads otherwise; the residual form gathers the centroid row
//     through assign and subtracts in the same registers.  Rows beyond n, rows with an assign outside [0, nlist) and components
//     beyond dsub are zeros.  The operands of the next step (block, or first block of the next tile) are loaded before the MFMAs
//     of this one.
//   * a B fragment is one 16-byte LDS read of row 16 * nb + l % 16 whose four components feed four MFMAs, so MFMA j of a block sums
//     the components 4 * g + j, g = 0 .. 3; a lane whose components lie beyond the row reads the zero pad.  The order depends on dsub
//     alone.  16 column blocks x 2 row blocks of accumulators: all 256 scores of a row stay in registers.
//   * score = fmaf(-2, acc, |c|^2).  A lane reduces its 16 column blocks in ascending order with a strict <, the 16 lanes of a row
//     group meet in a four-step butterfly on (score, index) where the lower index wins an equal score, and lane 0 of the group
//     stores the byte codes[row * M + m] (0 for a row whose assign is outside [0, nlist)).
// Every loop that holds a barrier or a cross-lane operation has a uniform trip count.  Nothing spins; no workgroup waits for another.
#include "common.h"
#include "host_call.h"
#include "ivf_pq_encode_plan.h"

using namespace vidc;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct IvEncode {
    uint64_t n;
    const float *x;
    uint32_t d, M, dsub, S;
    const float *pq;
    uint64_t nlist;
    const float *cent;  // NULL: raw
    const int64_t *assign;
    uint8_t *codes;
    uint64_t ntiles, items;
};

// components k0 .. k0 + 3 of a sub-vector of dsub floats; beyond dsub: zeros
template <bool VEC>
__device__ __forceinline__ v4f load4(const float *sub, uint32_t k0, uint32_t dsub) {
    v4f v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (k0 < dsub) v = *(const v4f *)(sub + k0);  // (dsub % 4 == 0: the four lie inside the sub-vector)
    } else {
        if (k0 < dsub) v.x = sub[k0];
        if (k0 + 1u < dsub) v.y = sub[k0 + 1u];
        if (k0 + 2u < dsub) v.z = sub[k0 + 2u];
        if (k0 + 3u < dsub) v.w = sub[k0 + 3u];
    }
    return v;
}

template <bool VEC, bool RES>
__global__ void __launch_bounds__(256, 2) k_ivf_pq_encode(IvEncode a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // the layout of ipe::lds_bytes
    constexpr uint32_t MT = ipe::MT, TV = ipe::TV, KSUB = ipe::KSUB;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, d = a.d, dsub = a.dsub;
    const uint32_t dsubp = (dsub + 3u) & ~3u, ldw = ipe::row_floats(dsub), nkb = (dsub + 15u) / 16u;
    const uint32_t fr = lane & 15u, fk = (lane >> 4) * 4u;  // MFMA: row fr of a 16-row block, components fk .. fk + 3 of 16
    float *cb = lds, *cnorm = lds + KSUB * ldw;

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint32_t m = (uint32_t)(item / a.S), s = (uint32_t)(item % a.S);
        const uint64_t t0 = ipe::piece_tile(a.ntiles, a.S, s), t1 = ipe::piece_tile(a.ntiles, a.S, s + 1u);
        const float *book = a.pq + (size_t)m * KSUB * dsub;
        __syncthreads();  // (the previous item's tiles have read their last fragment)
        if (VEC) {
            const uint32_t q4 = dsub / 4u;
            for (uint32_t q = tid; q < KSUB * q4; q += 256u) *(v4f *)(cb + (q / q4) * ldw + (q % q4) * 4u) = *(const v4f *)(book + 4u * q);
        } else {
            for (uint32_t e = tid; e < KSUB * dsub; e += 256u) cb[(e / dsub) * ldw + e % dsub] = book[e];
        }
        for (uint32_t k = dsub; k < ldw; k++) cb[tid * ldw + k] = 0.f;  // the pad columns of row tid
        __syncthreads();
        {
            float n2 = 0.f;
            for (uint32_t k = 0; k < dsub; k++) n2 = __builtin_fmaf(cb[tid * ldw + k], cb[tid * ldw + k], n2);
            cnorm[tid] = n2;
        }
        __syncthreads();

        const float *xs = a.x + (size_t)m * dsub, *cs = RES ? a.cent + (size_t)m * dsub : nullptr;
        // the A operands of block kb of the tile: rows tile * 128 + 32 w + 16 i + fr
        auto fetch = [&](uint64_t tile, uint32_t kb, v4f *out) {
#pragma unroll
            for (uint32_t i = 0; i < MT; i++) {
                const uint64_t row = tile * TV + w * 16u * MT + i * 16u + fr;
                v4f v = {0.f, 0.f, 0.f, 0.f};
                if (row < a.n) {
                    if (RES) {
                        const int64_t l = a.assign[row];
                        if (l >= 0 && (uint64_t)l < a.nlist) v = load4<VEC>(xs + row * d, kb + fk, dsub) - load4<VEC>(cs + (uint64_t)l * d, kb + fk, dsub);
                    } else {
                        v = load4<VEC>(xs + row * d, kb + fk, dsub);
                    }
                }
                out[i] = v;
            }
        };

        v4f nxt[MT];
        fetch(t0, 0, nxt);
        for (uint64_t tile = t0; tile < t1; tile++) {
            v4f acc[16][MT];
#pragma unroll
            for (uint32_t nb = 0; nb < 16; nb++)
#pragma unroll
                for (uint32_t i = 0; i < MT; i++) acc[nb][i] = (v4f){0.f, 0.f, 0.f, 0.f};
            for (uint32_t kb = 0; kb < nkb * 16u; kb += 16u) {
                v4f af[MT];
#pragma unroll
                for (uint32_t i = 0; i < MT; i++) af[i] = nxt[i];
                if (kb + 16u < nkb * 16u) fetch(tile, kb + 16u, nxt);
                else if (tile + 1u < t1) fetch(tile + 1u, 0, nxt);
                const float *bp = cb + fr * ldw + (kb + fk < dsubp ? kb + fk : dsubp);  // (beyond the row: its zero pad)
#pragma unroll
                for (uint32_t nb = 0; nb < 16; nb++) {
                    const v4f bf = *(const v4f *)(bp + nb * 16u * ldw);
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++)
#pragma unroll
                        for (uint32_t i = 0; i < MT; i++) acc[nb][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][j], bf[j], acc[nb][i], 0, 0, 0);
                }
            }

            // accumulator r of block (nb, i): row 16 i + 4 (lane / 16) + r of the wavefront's 32, codeword 16 nb + fr
            float best[MT][4];
            uint32_t arg[MT][4];
#pragma unroll
            for (uint32_t nb = 0; nb < 16; nb++) {
                const float c2 = cnorm[nb * 16u + fr];
#pragma unroll
                for (uint32_t i = 0; i < MT; i++)
#pragma unroll
                    for (uint32_t r = 0; r < 4; r++) {
                        const float sc = __builtin_fmaf(-2.f, acc[nb][i][r], c2);
                        if (nb == 0 || sc < best[i][r]) {
                            best[i][r] = sc;
                            arg[i][r] = nb * 16u + fr;
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
                        bool ok = true;
                        if (RES) {
                            const int64_t l = a.assign[row];
                            ok = l >= 0 && (uint64_t)l < a.nlist;
                        }
                        a.codes[row * a.M + m] = ok ? (uint8_t)j : (uint8_t)0;
                    }
                }
        }
    }
}

typedef void (*EncodeKernel)(IvEncode);
EncodeKernel encode_kernel(bool vec, bool res) {
    if (res) return vec ? k_ivf_pq_encode<true, true> : k_ivf_pq_encode<false, true>;
    return vec ? k_ivf_pq_encode<true, false> : k_ivf_pq_encode<false, false>;
}

}  // namespace

extern "C" int vidc_ivf_pq_encode_dev(vidc_ctx *ctx, uint64_t n, const float *d_x, uint32_t d, uint32_t M, const float *d_pq, uint64_t nlist,
                                      const float *d_centroids, const int64_t *d_assign, uint8_t *d_codes) {
    if (!ctx) {
        set_error("ivf pq encode: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ipe::Args args = {n, d_x, d, M, d_pq, nlist, d_centroids, d_assign, d_codes};
    if (const char *msg = ipe::check_args(args)) {
        set_error("ivf pq encode: %s", msg);
        return VIDC_ERR_INVALID;
    }
    if (!n) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const ipe::Plan p = ipe::make_plan((uint32_t)ctx->num_cu, n, d, M, (uintptr_t)d_x, (uintptr_t)d_pq, (uintptr_t)d_centroids);
    StreamGuard guard(ctx);
    IvEncode a = {};
    a.n = n; a.x = d_x; a.d = d; a.M = M; a.dsub = p.dsub; a.S = p.S; a.pq = d_pq; a.nlist = nlist; a.cent = d_centroids;
    a.assign = d_assign; a.codes = d_codes; a.ntiles = p.ntiles; a.items = p.items;
    const EncodeKernel fn = encode_kernel(p.vec, d_centroids != nullptr);
    if (p.lds > 64u * 1024u)  // (above the default cap of a launch)
        VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(fn, dim3(p.grid), dim3(ipe::THREADS), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());  // the call's one wait
    guard.disarm();
    return VIDC_OK;
}
