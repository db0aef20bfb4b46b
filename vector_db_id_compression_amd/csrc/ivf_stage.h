// ivf_stage.h -- the staging of a trip's code rows into LDS, shared by the scans whose rows start on no particular boundary
// (ivf_pqbits.hip: k_ivf_scan_pqbits, ivf_aq.hip: k_ivf_scan_aq).  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vidc {
namespace dev {

// the bytes [g0, g0 + len) of the code array (total bytes in all, len > 0) -> LDS, as the aligned 16-byte chunks that cover them;
// -> the stage byte the span starts at (0 .. 15).  The caller's barriers stand in front of and behind it.
__device__ __forceinline__ uint32_t stage_span(const uint8_t *codes, uint64_t total, uint64_t g0, uint32_t len, uint32_t lane, uint32_t *stage) {
    const uintptr_t base = (uintptr_t)codes, end = base + total, A = base + g0, A0 = A & ~(uintptr_t)15;
    const uint32_t head = (uint32_t)(A - A0), nch = (head + len + 15u) >> 4;
    for (uint32_t c = lane; c < nch; c += 64) {
        const uintptr_t ca = A0 + 16u * c;
        uint4 v;
        if (ca >= base && ca + 16u <= end) {
            v = *(const uint4 *)ca;
        } else {  // the first or the last chunk of the array: words where they lie inside, guarded bytes at the edge
            uint32_t w[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uintptr_t wa = ca + 4u * j;
                uint32_t x = 0;
                if (wa >= base && wa + 4u <= end) {
                    x = *(const uint32_t *)wa;
                } else {
#pragma unroll
                    for (uint32_t b = 0; b < 4; b++)
                        if (wa + b >= base && wa + b < end) x |= (uint32_t)*(const uint8_t *)(wa + b) << (8u * b);
                }
                w[j] = x;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)(stage + 4u * c) = v;
    }
    return head;
}

}  // namespace dev
}  // namespace vidc
