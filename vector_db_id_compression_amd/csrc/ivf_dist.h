// ivf_dist.h -- the distance trip of the IVF kernels (ivf_scan.hip: k_ivf_scan, ivf_range.hip: k_ivf_range): 64 codes of a list in,
// one float per lane out.  Device only, one wavefront per workgroup.  Everything a result depends on is an argument: the same
// (KIND, V, G, logG) give the same bits for the same codes, whichever kernel asks.
//   FLAT: G lanes share one vector (16-byte loads when V == 4: d % 4 == 0 and both bases aligned, gs::group), partial sums meet in a
//     G-lane butterfly; which lanes sum which components depends on (d, G) only.  cdist: 64 floats of LDS.
//   PQ8: a lane takes one code, its M bytes with loads of W = V bytes, and adds M table reads in m order (a byte indexes 256 entries:
//     always inside).  table: the query's M x 256 entries in LDS.
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
