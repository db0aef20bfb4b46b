// u2_push_ref.h -- the id push of a k_roc_encode_u2 step in plain C++ (no HIP: tests/u2_push_test.cpp runs both forms against each
// other on the host, tests/roc_push_ref.py is the same in Python).  The mirror of u2_pops_ref.h.
//
// An id x of precision P <= 32 is pushed as two slices (codec.cpp:92-105 with :65-76; the slices above bit 32 have width 0 and
// spill only a head >= 2^63, which the loops test on their way out): x_lo with p0 = min(P, 16) bits, then x_hi with
// p1 = clamp(P - 16, 0, 16) bits, and in front of each of them "head >= 2^(63 - p): push(low word), head >>= 32".
//   u2_push_two   that sequence, as the branch-free slices of U2_ENC_PUSH_SLICES (roc_u2.h) run it.
//   u2_push_one   the classified form of the dense step: ONE test of q = the head behind the index pop, one shift by p0 + p1, no
//                 stack access in the common class; the two spilling classes are the side body.
// Two facts make them equal for every q < 2^63 (a head behind an index pop is a quotient by nmax >= 2, possibly refilled: below 2^63):
//   * a step spills at most once: behind a spill of slice 0 the head is below 2^(31 + p0) <= 2^47 <= 2^(63 - p1).
//   * which slice spills depends on q alone, never on x: x_lo < 2^p0 is added to q << p0, whose p0 low bits are zero, so it never
//     carries into the comparison of slice 1.
//       class A  q >= 2^(63 - p0):                 slice 0 spills q's low word.   B = (q >> 32) << (p0 + p1),         mul = 2^p1
//       class B  2^(63 - p0 - p1) <= q < 2^(63 - p0): slice 1 spills (q << p0)'s low word | x_lo.
//                                                                                 B = (q >> (32 - p0)) << p1,         mul = 0
//       class C  q < 2^(63 - p0 - p1):             no spill.                      B = q << (p0 + p1),                 mul = 2^p1
//     and the head the step leaves is B + x_lo * mul + x_hi.  For P <= 16, p1 = 0 and class B is empty.
#pragma once
#include <stdint.h>

namespace vidc {

enum U2PushClass : uint32_t { U2_PUSH_C = 0, U2_PUSH_A = 1, U2_PUSH_B = 2, U2_PUSH_BOTH = 3 };  // BOTH: the reference form only

struct U2Push {
    uint64_t head;    // B + c(x): the head the step leaves
    uint64_t B;       // s[58:59]
    uint32_t mul;     // multiplier of x_lo in c(x) = x_lo * mul + x_hi
    uint32_t word;    // the spilled word (pushed == 1)
    uint32_t pushed;  // words put on the stack
    uint32_t cls;     // U2PushClass
};

inline uint32_t u2_push_p0(uint32_t P) { return P < 16u ? P : 16u; }
inline uint32_t u2_push_p1(uint32_t P) { return P > 16u ? (P - 16u > 16u ? 16u : P - 16u) : 0u; }

// codec.cpp:65-76 twice; push(w) puts a word on the stack
template <class PushFn>
inline U2Push u2_push_two(uint64_t q, uint32_t x, uint32_t p0, uint32_t p1, PushFn push) {
    U2Push r{0, 0, 0, 0, 0, U2_PUSH_C};
    const uint32_t x_lo = x & 0xffffu, x_hi = x >> 16;
    uint64_t head = q;
    if (head >= (((1ull << 31) >> p0) << 32)) { r.word = (uint32_t)head; push(r.word); head >>= 32; r.pushed++; r.cls |= U2_PUSH_A; }
    head = (head << p0) + x_lo;
    if (head >= (((1ull << 31) >> p1) << 32)) { r.word = (uint32_t)head; push(r.word); head >>= 32; r.pushed++; r.cls |= U2_PUSH_B; }
    head = (head << p1) + x_hi;
    r.head = head;
    return r;
}

// the dense step of k_roc_encode_u2 (U2_ENC_PUSH = 1): common path and side body, register by register
inline U2Push u2_push_one(uint64_t q, uint32_t x, uint32_t p0, uint32_t p1) {
    const uint32_t T0 = 0x80000000u >> p0, T1 = 0x80000000u >> p1, T2 = T0 >> p1, sh = p0 + p1;  // s73, s74, s46, s47
    const uint32_t q_lo = (uint32_t)q, q_hi = (uint32_t)(q >> 32);                                // s50, s51
    U2Push r{0, 0, 1u << p1, 0, 0, U2_PUSH_C};
    if (q_hi < T2) {                                        // s_cmp_ge_u32 s51, s46; s_cbranch_scc1 side
        r.B = q << (sh & 63u);                              // s_lshl_b64 s[58:59], s[50:51], s47
    } else {                                                // the side body: the two branch-free slices
        const bool s0 = q_hi >= T0;                         // s_cmp_ge_u32 s51, s73
        const uint64_t a = s0 ? (uint64_t)q_hi : q;         // s_cselect_b32 s52, s51, s50; s_cselect_b32 s53, 0, s51
        const uint64_t A = a << (p0 & 63u);                 // s_lshl_b64 s[54:55], s[52:53], s76
        const bool s1 = (uint32_t)(A >> 32) >= T1;          // s_cmp_ge_u32 s55, s74
        const uint64_t b = s1 ? A >> 32 : A;                // s_cselect_b32 s56, s55, s54; s_cselect_b32 s57, 0, s55
        r.B = b << (p1 & 63u);                              // s_lshl_b64 s[58:59], s[56:57], s77
        r.pushed = (s0 ? 1u : 0u) + (s1 ? 1u : 0u);         // s_addc_u32 s60, s60, 0 (twice)
        r.cls = (s0 ? U2_PUSH_A : 0u) | (s1 ? U2_PUSH_B : 0u);
        r.word = s1 ? ((x & 0xffffu) | (uint32_t)A) : q_lo; // v_writelane v5 at the slot of its slice
        if (s1) r.mul = 0;                                  // s_cselect_b32 s48, 0xffff0000, -1 ... s_and_b32 s40, s40, s48: x_lo leaves c(x)
    }
    r.head = r.B + (uint64_t)((x & 0xffffu) * r.mul + (x >> 16));
    return r;
}

// the class of a head q behind the index pop, from q alone
inline uint32_t u2_push_class(uint64_t q, uint32_t p0, uint32_t p1) {
    return q >= (1ull << (63u - p0)) ? U2_PUSH_A : q >= (1ull << (63u - p0 - p1)) ? U2_PUSH_B : U2_PUSH_C;
}

}  // namespace vidc
