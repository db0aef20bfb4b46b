// u2_div_ref.h -- the data flow of U2_DIV (roc_u2.h) in plain C++, instruction by instruction (no HIP: tests/u2_div_test.cpp
// checks it against unsigned __int128 on the host).
//
// U2_DIV computes q^ = hi64(B * m) for B = {b1, b0} (s[58:59]) and the per-lane reciprocal m = {m1, m0} (v8, v7) =
// floor((2^64 - 1) / d):
//     t  = mul_hi(b0, m0)                       v36            (v37 stays 0)
//     P1 = b0 * m1 + t                          v[38:39]       one v_mad_u64_u32; < 2^64 always: (2^32 - 1)^2 + 2^32 - 1 < 2^64
//     S  = b1 * m0 + P1                         v[42:43]       one v_mad_u64_u32 with the WHOLE pair v[38:39] as addend
//     q^ = b1 * m1 + hi32(S)                    v[46:47]       v_mov v40, v43 (v41 stays 0), one v_mad_u64_u32
// The wanted value is floor((t + b0 m1 + b1 m0) / 2^32) + b1 m1 = hi32(S) + b1 m1 PLUS the carry of S out of 64 bits.  Inside the
// encode loop that carry is always 0: the exit test keeps B < U2_SAFE_HI * 2^32 < 2^63, so b1 < 2^31; a lane that a step reads
// divides by d >= 3 (d >= 2 in a lane that is moved at a block change), so m < 2^63 and m1 < 2^31; hence b1 m0 < 2^63, P1 =
// b0 m1 + t < 2^63 and S < 2^64.  (The carry-free form needs the exit test: B >= 2^63 with d = 2 does carry.)
#pragma once
#include <stdint.h>

namespace vidc {

struct U2DivFlow {
    uint64_t q;      // v[46:47]
    bool carry;      // the carry out of S that U2_DIV drops (0 inside the loop's domain)
};

inline U2DivFlow u2_div_flow(uint64_t B, uint64_t m) {
    const uint32_t b0 = (uint32_t)B, b1 = (uint32_t)(B >> 32), m0 = (uint32_t)m, m1 = (uint32_t)(m >> 32);
    const uint32_t t = (uint32_t)(((uint64_t)b0 * m0) >> 32);  // v_mul_hi_u32 v36, s58, v7
    const uint64_t P1 = (uint64_t)b0 * m1 + (uint64_t)t;       // v_mad_u64_u32 v[38:39], s58, v8, v[36:37]
    const uint64_t X = (uint64_t)b1 * m0;
    const uint64_t S = X + P1;                                 // v_mad_u64_u32 v[42:43], s59, v7, v[38:39]   (wraps like the instruction)
    const uint32_t h = (uint32_t)(S >> 32);                    // v_mov_b32 v40, v43
    U2DivFlow r;
    r.q = (uint64_t)b1 * m1 + (uint64_t)h;                     // v_mad_u64_u32 v[46:47], s59, v8, v[40:41]
    r.carry = S < X;
    return r;
}

}  // namespace vidc
