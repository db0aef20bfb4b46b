// ivf_dist.h -- the distance trip of the IVF kernels (ivf_scan.hip: k_ivf_scan, ivf_range.hip: k_ivf_range): 64 codes of a list in,
// one float per lane out.  Device only, one wavefront per workgroup.  Everything a result depends on is an argument: the same
// (KIND, V, G, logG) give the same bits for the same codes, whichever kernel asks.
//   FLAT: G lanes share one vector (16-byte loads when V == 4: d % 4 == 0 and both bases aligned, gs::group), partial sums meet in a
//     G-lane butterfly; which lanes sum which components depends on (d, G) only.  cdist: 64 floats of LDS.
//   PQ8: a lane takes one code, its M bytes with loads of W = V bytes, and adds M table reads in m order (a byte indexes 256 entries:
//     always inside).  table: the query's M x 256 entries in LDS.
//   Residual PQ: the PQ8 trip over a table that residual_table built for (query, list).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_scan_ref.h"

namespace vidc {
namespace dev {

// one PQ code -> its distance: M bytes, W at a load, the table entries added in m order
template <int W>
__device__ __forceinline__ float pq_distance(const uint8_t *code, const float *table, uint32_t M) {
    float s = 0.f;
    for (uint32_t m0 = 0; m0 < M; m0 += W) {
        uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (W == 16) {
            const uint4 v = *(const uint4 *)(code + m0);
            w0 = v.x; w1 = v.y; w2 = v.z; w3 = v.w;
        } else if (W == 8) {
            const uint2 v = *(const uint2 *)(code + m0);
            w0 = v.x; w1 = v.y;
        } else if (W == 4) {
            w0 = *(const uint32_t *)(code + m0);
        } else if (W == 2) {
            w0 = *(const uint16_t *)(code + m0);
        } else {
            w0 = code[m0];
        }
#pragma unroll
        for (int b = 0; b < W; b++) {
            const uint32_t w = b < 4 ? w0 : (b < 8 ? w1 : (b < 12 ? w2 : w3));
            s += table[(m0 + b) * 256u + ((w >> ((b & 3) * 8)) & 255u)];
        }
    }
    return s;
}

// Residual PQ (ivf_residual.hip: scan, count and fill call this one function in front of every probed list that is not empty): the
// residual r = qv - centroid, one float32 subtraction per component, goes to LDS and the wavefront builds the list's M x 256 table
// from it; ivf_trip_distance<PQ8, W> then walks that table.  An entry is ivs::pq_entry(r, codebooks, dsub, m, c): the same
// subtractions, squares and additions in the same order, with four entries of a lane in flight (lane e, e + 64, e + 128, e + 192 of
// sub-quantiser m: M * 256 is a multiple of 256, so no entry is out of range) -- a lane that walked one entry at a time waited for
// every load in turn.  vec4: the codebooks are read 16 bytes at a load (dsub % 4 == 0 and a 16-byte aligned base:
// ivx::codebook_vec4), else a float at a load; the value does not depend on it.  A load of the wavefront covers 64 neighbouring
// codebook rows.  qv, r: d floats of LDS each, 16-byte aligned; centroid: the list's row of the centroid array.  Holds three barriers
// (lanes may still read the previous list's table; r is complete; the table is complete): every lane of the wavefront calls it.
__device__ __forceinline__ void residual_table(const float *qv, const float *__restrict__ centroid, const float *__restrict__ codebooks,
                                               uint32_t d, uint32_t M, bool vec4, uint32_t lane, float *r, float *table) {
    __syncthreads();
    for (uint32_t i = lane; i < d; i += 64) r[i] = qv[i] - centroid[i];
    __syncthreads();
    const uint32_t dsub = d / M;
    for (uint32_t m = 0; m < M; m++) {
        const float *rm = r + m * dsub;
        const float *row = codebooks + ((uint64_t)m * 256u + lane) * dsub;  // entry (m, lane); entry (m, lane + 64 u) is 64 u rows on
        const uint64_t step = (uint64_t)64 * dsub;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        if (vec4) {
            for (uint32_t i = 0; i < dsub; i += 4) {
                const float4 y = *(const float4 *)(rm + i);
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
                const float y = rm[i], x0 = row[i], x1 = row[step + i], x2 = row[2 * step + i], x3 = row[3 * step + i];
                float t;
                t = y - x0; s0 += t * t;
                t = y - x1; s1 += t * t;
                t = y - x2; s2 += t * t;
                t = y - x3; s3 += t * t;
            }
        }
        float *tm = table + m * 256u + lane;
        tm[0] = s0; tm[64] = s1; tm[128] = s2; tm[192] = s3;
    }
    __syncthreads();
}

// The trip: codes p0 .. p0 + n of the code array (n <= 64, wavefront-uniform) -> lane c holds the distance of code p0 + c, lanes
// >= n hold 0.  KIND FLAT: V components per load (4 or 1), qv the query vector in LDS.  KIND PQ8: V is W, the bytes of a code load.
// FLAT holds a barrier: every lane of the wavefront calls it.
template <int KIND, int V>
__device__ __forceinline__ float ivf_trip_distance(const uint8_t *codes, uint64_t p0, uint32_t n, uint32_t lane, uint32_t d, uint32_t M,
                                                   const float *qv, const float *table, float *cdist, uint32_t G, uint32_t logG) {
    float dist = 0.f;
    if (KIND == ivs::PQ8) {
        if (lane < n) dist = pq_distance<V>(codes + (p0 + lane) * M, table, M);
    } else {
        const uint32_t per = 64u >> logG, g = lane & (G - 1u);
        for (uint32_t c0 = 0; c0 < n; c0 += per) {
            const uint32_t idx = c0 + (lane >> logG);
            float sum = 0.f;
            if (idx < n) {
                const float *vec = (const float *)(codes + (p0 + idx) * ((uint64_t)d * 4u));
                if (V == 4) {
                    for (uint32_t i = g * 4u; i < d; i += G * 4u) {
                        const float4 x = *(const float4 *)(vec + i), y = *(const float4 *)(qv + i);
                        const float t0 = y.x - x.x, t1 = y.y - x.y, t2 = y.z - x.z, t3 = y.w - x.w;
                        sum += t0 * t0;
                        sum += t1 * t1;
                        sum += t2 * t2;
                        sum += t3 * t3;
                    }
                } else {
                    for (uint32_t i = g; i < d; i += G) {
                        const float t = qv[i] - vec[i];
                        sum += t * t;
                    }
                }
            }
            for (uint32_t o = G >> 1; o; o >>= 1) sum += __shfl_xor(sum, (int)o, 64);
            if (idx < n && g == 0) cdist[idx] = sum;
        }
        __syncthreads();
        if (lane < n) dist = cdist[lane];
    }
    return dist;
}

}  // namespace dev
}  // namespace vidc
