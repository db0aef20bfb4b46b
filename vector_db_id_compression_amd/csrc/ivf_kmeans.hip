// ivf_kmeans.hip -- one Lloyd iteration on the device (vidc_ivf_kmeans_step_dev, include/vidc.h), batched over G independent groups
// of columns: the coarse centroids of an IVF index are G = 1, its PQ codebooks G = M.  The assignment is the PQ encoder's score and
// tie rule on float32 MFMA (v_mfma_f32_16x16x4_f32); the update adds the members of a cluster in ascending point order, 256 to a
// partial, partials in order: no float atomic and no atomic-decided position enters a value, so the same inputs give the same bits on
// every context and however the work is cut.
//
// What the host decides (checks, held-whole or streamed, LDS, the cut S, load widths, update batches, scratch) is csrc/ivf_kmeans_plan.h.
//
// k_kmeans_norms.  A thread per (g, j): |c|^2 with fmaf in component order, to scratch.
// k_kmeans_assign.  A workgroup of four wavefronts takes items (group g, piece s of the point range) = item / S, item % S in a
//   grid-stride loop and walks the piece in blocks of 128 points, 32 rows a wavefront.
//   * points never touch LDS: lane l loads the components 4 * (l / 16) .. + 3 of a 16-component block of the columns of group g of
//     row l % 16 (+ 16) straight into MFMA A operands (one 16-byte load where the plan allows it, four guarded 4-byte loads
//     otherwise); rows beyond n and components beyond dsub are zeros.
//   * WHOLE: the k centroids of g are staged once per item as [k][round_up(dsub, 4) + 4] floats, pad columns zero (the encoder's
//     codebook); a fragment row beyond k reads row k - 1, whose score is never looked at.  Otherwise they stream through two staging
//     buffers in tiles of 128 centroids x 32 components, rows beyond k and components beyond dsub zero: the loads of step t + 1 are
//     issued before the MFMAs of step t and stored behind them, one barrier a step.
//   * a B fragment is one 16-byte LDS read whose four components feed four MFMAs, so MFMA j of a 16-component block sums the
//     components 4 * q + j, q = 0 .. 3, blocks in ascending order: the order depends on dsub alone and is the same in both forms (a
//     block of zeros adds nothing).  8 column blocks x 2 row blocks of accumulators stay in registers across the chunks of a tile.
//   * score = fmaf(-2, acc, |c|^2) for the columns below k only; a lane keeps a running (score, j) best over its columns across all
//     tiles with a strict <, the 16 lanes of a row meet in one four-step butterfly on (score, j) where the lower j wins an equal
//     score, and lane 0 of the group stores the int32 (0 where no score was finite).  No selection pool.
// members.  Keys g * k + j of the pairs (g, i) in [G, n] order, the stable LSD radix sort of append.h (pair numbers ascend inside a
//   key), k_kmeans_bounds: first sorted position of every key by binary search, and the chunks of 256 of every cluster.
// k_kmeans_partial.  Lanes over components (plan: ikm::Lanes); a lane adds the rows of its chunk strictly in member order, four loads
//   in flight, and writes partial[chunk][component].
// k_kmeans_finish.  A thread per (cluster, component): partials in chunk order, one IEEE division by (float)count; an empty cluster
//   copies c_in; component 0 writes the count.
// Every loop that holds a barrier or a cross-lane operation has a uniform trip count.  Nothing spins; no workgroup waits for another.
#include "append.h"
#include "common.h"
#include "host_call.h"
#include "ivf_kmeans_plan.h"

using namespace vidc;

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

struct KmAssign {
    uint64_t n;
    const float *x;
    uint32_t ld, dsub, k, S;
    const float *c, *norms;
    int32_t *assign;
    uint64_t ntiles, items;
};

// components k0 .. k0 + 3 of a row of dsub floats; beyond dsub: zeros
template <bool VEC>
__device__ __forceinline__ v4f km_load4(const float *row, uint32_t k0, uint32_t dsub) {
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

__global__ void __launch_bounds__(256) k_kmeans_norms(const float *__restrict__ c, uint32_t clusters, uint32_t dsub, float *__restrict__ norms) {
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < clusters; l += gridDim.x * blockDim.x) {
        const float *row = c + (size_t)l * dsub;
        float n2 = 0.f;
        for (uint32_t q = 0; q < dsub; q++) n2 = __builtin_fmaf(row[q], row[q], n2);
        norms[l] = n2;
    }
}

template <bool VEC, bool WHOLE>
__global__ void __launch_bounds__(256, 2) k_kmeans_assign(KmAssign a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // WHOLE: [k][row_floats]; else [2][TC][LDW]
    constexpr uint32_t MT = ikm::MT, TV = ikm::TV, TC = ikm::TC, KC = ikm::KC, LDW = ikm::LDW, NB = TC / 16u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, dsub = a.dsub, k = a.k, ld = a.ld;
    const uint32_t dsubp = ikm::round4(dsub), ldw = ikm::row_floats(dsub), nkb = (dsub + 15u) / 16u, nct = (k + TC - 1u) / TC;
    const uint32_t fr = lane & 15u, fk = (lane >> 4) * 4u;  // MFMA: row fr of a 16-row block, components fk .. fk + 3 of 16

    for (uint64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const uint32_t g = (uint32_t)(item / a.S), s = (uint32_t)(item % a.S);
        const uint64_t t0 = ikm::piece_tile(a.ntiles, a.S, s), t1 = ikm::piece_tile(a.ntiles, a.S, s + 1u);
        const float *cg = a.c + (size_t)g * k * dsub, *ng = a.norms + (size_t)g * k, *xs = a.x + (size_t)g * dsub;
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

        // the A operands of block kb of the point block: rows tile * 128 + 32 w + 16 i + fr
        auto fetch = [&](uint64_t tile, uint32_t kb, v4f *out) {
#pragma unroll
            for (uint32_t i = 0; i < MT; i++) {
                const uint64_t row = tile * TV + w * 16u * MT + i * 16u + fr;
                v4f v = {0.f, 0.f, 0.f, 0.f};
                if (row < a.n) v = km_load4<VEC>(xs + row * ld, kb + fk, dsub);
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
                    if (col < k) v = km_load4<VEC>(cg + (size_t)col * dsub, ch * KC + sq, dsub);
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
                const uint32_t nbmax = (k - c0 + 15u) / 16u < NB ? (k - c0 + 15u) / 16u : NB;  // column blocks that hold a centroid
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

                // accumulator r of block (nb, i): row 16 i + 4 (lane / 16) + r of the wavefront's 32, centroid c0 + 16 nb + fr
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
                    if (fr == 0 && row < a.n) a.assign[(size_t)g * a.n + row] = j < k ? (int32_t)j : 0;
                }
        }
    }
}

typedef void (*AssignKernel)(KmAssign);
AssignKernel assign_kernel(bool vec, bool whole) {
    if (whole) return vec ? k_kmeans_assign<true, true> : k_kmeans_assign<false, true>;
    return vec ? k_kmeans_assign<true, false> : k_kmeans_assign<false, false>;
}

// ---- members: pair p = gl * n + i of a batch (gl: group inside the batch) has the key gl * k + assign
__global__ void __launch_bounds__(256) k_kmeans_keys(const int32_t *__restrict__ assign, uint32_t pairs, uint32_t n, uint32_t k, uint32_t *__restrict__ keys) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += (uint64_t)gridDim.x * blockDim.x)
        keys[p] = ((uint32_t)p / n) * k + (uint32_t)assign[p];
}

// bnd[l] = first sorted position whose key is >= l, l = 0 .. clusters; cnt[l] = chunks of cluster l
__global__ void __launch_bounds__(256) k_kmeans_bounds(const uint32_t *__restrict__ keys, uint32_t pairs, uint32_t clusters, uint32_t *__restrict__ bnd,
                                                       uint32_t *__restrict__ cnt) {
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l <= clusters; l += gridDim.x * blockDim.x) {
        uint32_t at[2];
#pragma unroll
        for (uint32_t e = 0; e < 2; e++) {
            uint32_t lo = 0, hi = pairs;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (keys[mid] < l + e) lo = mid + 1u; else hi = mid;
            }
            at[e] = lo;
        }
        bnd[l] = at[0];
        if (l < clusters) cnt[l] = (at[1] - at[0] + ikm::KM_CHUNK - 1u) / ikm::KM_CHUNK;
    }
}

struct KmUpdate {
    uint64_t n;
    const float *x;
    uint32_t ld, dsub, k, clusters, g0;  // the batch holds the groups g0 .. and `clusters` of their clusters
    uint32_t W, slots;
    const uint32_t *vals, *bnd;
    const uint64_t *off;  // [clusters + 1]: first chunk of every cluster
    const Chunk *items;
    float *part;          // [chunks][dsub]
    const float *c_in;
    float *c_out;
    uint32_t *counts;
};

template <uint32_t V>
__global__ void __launch_bounds__(256) k_kmeans_partial(KmUpdate a) {
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const uint64_t total = a.off[a.clusters];
    const uint32_t lane = threadIdx.x & 63u, W = a.W, side = 64u / W, sub = lane / W, sl = lane % W, dsub = a.dsub;
    const uint64_t wave = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t cbase = wave * side; cbase < total; cbase += nwaves * side) {
        const uint64_t c = cbase + sub;
        if (c >= total) continue;
        const Chunk ch = a.items[c];
        const uint32_t b0 = a.bnd[ch.list] + ch.start, left = a.bnd[ch.list + 1u] - b0;
        const uint32_t cnt = left < ikm::KM_CHUNK ? left : ikm::KM_CHUNK, gl = ch.list / a.k;
        const uint32_t *mem = a.vals + b0;
        const uint64_t first = (uint64_t)gl * a.n;  // pair number of point 0 of the group
        const float *xs = a.x + (size_t)(a.g0 + gl) * dsub;
        for (uint32_t slot = sl; slot < a.slots; slot += W) {
            const float *col = xs + slot * V;
            vec_t sum = 0.f;
            for (uint32_t m = 0; m < cnt; m += 4u) {
                vec_t v[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++)
                    if (m + u < cnt) v[u] = *(const vec_t *)(col + (mem[m + u] - first) * a.ld);
#pragma unroll
                for (uint32_t u = 0; u < 4; u++)
                    if (m + u < cnt) sum += v[u];
            }
            *(vec_t *)(a.part + c * dsub + slot * V) = sum;
        }
    }
}

__global__ void __launch_bounds__(256) k_kmeans_finish(KmUpdate a) {
    const uint64_t total = (uint64_t)a.clusters * a.dsub;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = (uint32_t)(e / a.dsub), q = (uint32_t)(e % a.dsub), cnt = a.bnd[l + 1u] - a.bnd[l];
        const size_t at = ((size_t)a.g0 * a.k + l) * a.dsub + q;
        if (cnt) {
            float sum = 0.f;
            for (uint64_t c = a.off[l]; c < a.off[l + 1u]; c++) sum += a.part[c * a.dsub + q];
            a.c_out[at] = __fdiv_rn(sum, (float)cnt);
        } else {
            a.c_out[at] = a.c_in[at];
        }
        if (q == 0 && a.counts) a.counts[(size_t)a.g0 * a.k + l] = cnt;
    }
}

__global__ void __launch_bounds__(256) k_kmeans_zero(uint32_t *p, uint32_t count) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) p[i] = 0u;
}

}  // namespace

extern "C" int vidc_ivf_kmeans_step_dev(vidc_ctx *ctx, uint64_t n, const float *d_x, uint32_t ld, uint32_t G, uint32_t dsub, uint32_t k,
                                        const float *d_c_in, float *d_c_out, int32_t *d_assign, uint32_t *d_counts) {
    if (!ctx) {
        set_error("ivf kmeans step: NULL context");
        return VIDC_ERR_INVALID;
    }
    const ikm::Args args = {n, d_x, ld, G, dsub, k, d_c_in, d_c_out};
    if (const char *msg = ikm::check_args(args)) {
        set_error("ivf kmeans step: %s", msg);
        return VIDC_ERR_INVALID;
    }
    VIDC_HIP(hipSetDevice(ctx->device));
    const uint32_t all = G * k;
    if (!n) {  // c_out = c_in, no members
        if (d_c_in && d_c_out) VIDC_HIP(hipMemcpyAsync(d_c_out, d_c_in, (size_t)all * dsub * 4, hipMemcpyDeviceToDevice, ctx->stream));
        if (d_counts) {
            hipLaunchKernelGGL(k_kmeans_zero, req_grid(ctx, all), dim3(256), 0, ctx->stream, d_counts, all);
            VIDC_HIP(hipGetLastError());
        }
        VIDC_HIP(vidc_stream_wait(ctx->stream));
        return VIDC_OK;
    }
    const ikm::Plan p = ikm::make_plan((uint32_t)ctx->num_cu, n, ld, G, dsub, k, (uintptr_t)d_x, (uintptr_t)d_c_in);
    const uint64_t P = (uint64_t)p.gb * n, L = (uint64_t)p.gb * k, cbound = ikm::chunk_bound(P, L);
    Scratch s_norms, s_assign, s_sort, s_hist, s_scan, s_tmp, s_bnd, s_off, s_items, s_part;
    StreamGuard guard(ctx);
    VIDC_TRY(s_norms.get(ctx, (size_t)all * 4));
    if (!d_assign) {
        VIDC_TRY(s_assign.get(ctx, (size_t)G * n * 4));
        d_assign = s_assign.as<int32_t>();
    }
    VIDC_TRY(s_sort.get(ctx, (size_t)P * 4 * 4));
    VIDC_TRY(s_bnd.get(ctx, (size_t)(L + 1) * 8));
    VIDC_TRY(s_off.get(ctx, (size_t)(L + 1) * 8));
    VIDC_TRY(s_items.get(ctx, (size_t)(cbound + 1) * sizeof(Chunk)));
    VIDC_TRY(s_part.get(ctx, (size_t)cbound * dsub * 4));
    uint32_t *bnd = s_bnd.as<uint32_t>(), *cnt = bnd + L + 1;

    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(k_kmeans_norms, req_grid(ctx, all), dim3(256), 0, ctx->stream, d_c_in, all, dsub, s_norms.as<float>());
    KmAssign a = {};
    a.n = n; a.x = d_x; a.ld = ld; a.dsub = dsub; a.k = k; a.S = p.S; a.c = d_c_in; a.norms = s_norms.as<float>(); a.assign = d_assign;
    a.ntiles = p.ntiles; a.items = p.items;
    hipLaunchKernelGGL(assign_kernel(p.vec, p.whole), dim3(p.grid), dim3(ikm::THREADS), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());

    for (uint32_t g0 = 0; g0 < G; g0 += p.gb) {  // the update, a batch of whole groups at a time (one batch unless G * n is huge)
        const uint32_t gb = G - g0 < p.gb ? G - g0 : p.gb, pairs = (uint32_t)((uint64_t)gb * n), clusters = gb * k;
        AppSort s;
        s.n = pairs;
        s.kb[0] = s_sort.as<uint32_t>(); s.kb[1] = s.kb[0] + P; s.vb[0] = s.kb[1] + P; s.vb[1] = s.vb[0] + P;
        VIDC_TRY(app_sort_scratch(ctx, s, s_hist, s_scan));
        const int32_t *asg = d_assign + (size_t)g0 * n;
        VIDC_TRY(app_sort_phase(ctx, s, ikm::key_bits(clusters), s_hist, s_scan, s_tmp, [&](uint32_t *kdst, const uint32_t *) {
            hipLaunchKernelGGL(k_kmeans_keys, req_grid(ctx, pairs), dim3(256), 0, ctx->stream, asg, pairs, (uint32_t)n, k, kdst);
        }));
        hipLaunchKernelGGL(k_kmeans_bounds, req_grid(ctx, clusters + 1), dim3(256), 0, ctx->stream, s.kin, pairs, clusters, bnd, cnt);
        VIDC_HIP(hipGetLastError());
        VIDC_TRY(device_exscan(ctx, cnt, clusters, s_off.as<uint64_t>(), s_tmp));
        launch_fill_items(ctx->stream, s_off.as<uint64_t>(), clusters, ikm::KM_CHUNK, s_items.as<Chunk>(), ikm::chunk_bound(pairs, clusters),
                          (uint32_t)ctx->num_cu);
        VIDC_HIP(hipGetLastError());
        KmUpdate u = {};
        u.n = n; u.x = d_x; u.ld = ld; u.dsub = dsub; u.k = k; u.clusters = clusters; u.g0 = g0; u.W = p.lanes.W; u.slots = p.lanes.slots;
        u.vals = s.vin; u.bnd = bnd; u.off = s_off.as<uint64_t>(); u.items = s_items.as<Chunk>(); u.part = s_part.as<float>();
        u.c_in = d_c_in; u.c_out = d_c_out; u.counts = d_counts;
        const uint64_t waves = (ikm::chunk_bound(pairs, clusters) + p.lanes.side - 1) / p.lanes.side;
        const dim3 pgrid((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((waves + 3) / 4, (uint64_t)ctx->num_cu * 16)));
        if (p.lanes.V == 4) hipLaunchKernelGGL(k_kmeans_partial<4>, pgrid, dim3(256), 0, ctx->stream, u);
        else hipLaunchKernelGGL(k_kmeans_partial<1>, pgrid, dim3(256), 0, ctx->stream, u);
        hipLaunchKernelGGL(k_kmeans_finish, req_grid(ctx, (uint64_t)clusters * dsub), dim3(256), 0, ctx->stream, u);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(t.finish());  // the call's one wait
    guard.disarm();
    return VIDC_OK;
}
