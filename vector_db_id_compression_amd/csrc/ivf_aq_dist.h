// ivf_aq_dist.h -- the two device steps of an additive-quantiser scan that every kernel over such codes takes in the same words
// (ivf_aq.hip: k_ivf_scan_aq, ivf_wide.hip: k_ivf_scan_wide): the fixed reduction behind qn and cq, and the distance of a staged row.
// The same arguments give the same bits, whichever kernel asks.  Behind them the one host step both units take: the launch of the
// table GEMM (k_ivf_aq_lut, ivf_aq.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_aq_plan.h"
#include "ivf_scan_ref.h"

struct vidc_ctx;

namespace vidc {

// the tables of nq queries into lut [nq, M, 256], on the context's stream (defined in ivf_aq.hip)
int ivf_aq_launch_lut(vidc_ctx *ctx, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq, float *lut);

namespace dev {

// <x, y> over d components, the same bits in every lane: lane l sums the components l, l + 64, ... in order with fmaf, then the
// lanes meet in a butterfly (a + b == b + a, so both sides of a step hold the same sum).  The order depends on d alone.
__device__ __forceinline__ float wave_dot(const float *x, const float *y, uint32_t d, uint32_t lane) {
    float s = 0.f;
    for (uint32_t i = lane; i < d; i += 64) s = __builtin_fmaf(x[i], y[i], s);
#pragma unroll
    for (uint32_t o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// the distance of the code row that starts at stage byte rs (iaq::distance): the M table entries added in m order, the norm from the
// four bytes behind the indices through two aligned words
__device__ __forceinline__ float aq_distance(const uint32_t *stage, uint32_t rs, const float *table, uint32_t M, float cq, float qn, bool res) {
    const float t = iaq::table_sum((const uint8_t *)stage + rs, M, table);
    const uint32_t o = rs + M, wi = o >> 2, sh = (o & 3u) * 8u;
    const uint64_t win = (uint64_t)stage[wi] | ((uint64_t)stage[wi + 1u] << 32);
    const float n = ivs::bits_f32((uint32_t)(win >> sh));
    return iaq::finish(t, n, cq, qn, res);
}

}  // namespace dev
}  // namespace vidc
