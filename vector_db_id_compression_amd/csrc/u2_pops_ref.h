// u2_pops_ref.h -- the two slice pops of a k_roc_decode_u2 step in plain C++ (no HIP: tests/u2_pops_test.cpp runs both forms against
// each other on the host, tests/roc_pops_ref.py is the same in Python).
//
// An id of precision P <= 32 is popped as two slices (codec.cpp:107-121 with :78-90; the slices above bit 32 have width 0 and never
// refill a head >= 2^31): x_hi with p1 = clamp(P - 16, 0, 16) bits, then x_lo with p0 = min(P, 16) bits, and after each of them
// "head < 2^31: head = (head << 32) | pop()".
//   u2_pops_two   that sequence, as U2_DEC_TOP_L / U2_DEC_SIDE (roc_u2.h) run it.
//   u2_pops_one   U2_DEC_TOP_P / U2_DEC_SIDE_P instruction by instruction: ONE test of head' = the head the previous step left, both
//                 slices out of its low dword, one shift by p1 + p0, at most one refill with the word w the next pop returns.
// Both are defined for head' >= 2^31, which is what every step of the loop starts from.  Two facts make them equal there:
//   * a step refills at most once: a refill leaves head >= 2^(63 - p1) behind slice 1 (head' >> p1 >= 2^(31 - p1)), and the one pop
//     that may follow takes p0 <= 16 bits: head >= 2^(47 - p1) >= 2^31.  Behind slice 0 nothing follows.
//   * which pop refills depends on head' alone: head' < 2^(31 + p1) slice 1; else head' < 2^(31 + p1 + p0) slice 0; else none.
// x_lo = s_bfe_u32(head'_lo, p1, p0) reads bits p1 .. p1 + p0 - 1 of the LOW dword only: p1 + p0 = min(P, 32) <= 32 for every
// precision (20 and 18 at most in the two launches), and the single shift count p1 + p0 <= 32 < 64 is inside the six bits a
// 64-bit scalar shift reads.
#pragma once
#include <stdint.h>

namespace vidc {

enum U2PopClass : uint32_t { U2_POP_NONE = 0, U2_POP_SLICE0 = 1, U2_POP_SLICE1 = 2, U2_POP_BOTH = 3 };  // BOTH: the reference form only

struct U2Pops {
    uint64_t head;    // s[58:59] behind the pops
    uint32_t x;       // s40 behind s_pack_ll_b32_b16
    uint32_t popped;  // words taken from the stack
    uint32_t cls;     // U2PopClass
};

inline uint32_t u2_pop_p1(uint32_t P) { return P > 16u ? (P - 16u > 16u ? 16u : P - 16u) : 0u; }
inline uint32_t u2_pop_p0(uint32_t P) { return P < 16u ? P : 16u; }

// codec.cpp:78-90 twice; pop() returns the next stack word
template <class Pop>
inline U2Pops u2_pops_two(uint64_t head, uint32_t p1, uint32_t p0, Pop pop) {
    U2Pops r{0, 0, 0, U2_POP_NONE};
    const uint32_t x_hi = (uint32_t)(head & ((1ull << p1) - 1ull));
    head >>= p1;
    if (head < (1ull << 31)) { head = (head << 32) | (uint64_t)pop(); r.popped++; r.cls |= U2_POP_SLICE1; }
    const uint32_t x_lo = (uint32_t)(head & ((1ull << p0) - 1ull));
    head >>= p0;
    if (head < (1ull << 31)) { head = (head << 32) | (uint64_t)pop(); r.popped++; r.cls |= U2_POP_SLICE0; }
    r.head = head;
    r.x = (x_hi << 16) | x_lo;
    return r;
}

inline uint32_t u2_s_bfe_u32(uint32_t v, uint32_t operand) {  // s_bfe_u32: offset = operand[4:0], width = operand[22:16]
    const uint32_t off = operand & 31u, width = (operand >> 16) & 127u;
    if (width == 0u) return 0u;
    return width >= 32u ? v >> off : (v >> off) & ((1u << width) - 1u);
}

// U2_DEC_TOP_P with U2_DEC_SIDE_P; w = the ring word at (sp - 1) & 63 (s41)
inline U2Pops u2_pops_one(uint64_t head, uint32_t w, uint32_t p1, uint32_t p0) {
    const uint32_t thr = 31u + p1, bfe = (p0 << 16) | p1, sh = p1 + p0;  // s56, s57, s63
    const uint32_t m1 = (1u << p1) - 1u, m0 = p0 >= 32u ? ~0u : (1u << p0) - 1u;  // s73, s74
    uint32_t lo = (uint32_t)head, hi = (uint32_t)(head >> 32);
    U2Pops r{0, 0, 0, U2_POP_NONE};
    uint32_t x_hi, x_lo;
    if ((head >> (thr & 63u)) != 0ull) {         // s_lshr_b64 s[98:99], s[58:59], s56; s_cbranch_scc0 side
        x_hi = lo & m1;                          // s_and_b32 s46, s58, s73
        x_lo = u2_s_bfe_u32(lo, bfe);            // s_bfe_u32 s40, s58, s57
        head >>= (sh & 63u);                     // s_lshr_b64 s[58:59], s[58:59], s63
        lo = (uint32_t)head; hi = (uint32_t)(head >> 32);
        const bool scc = (head >> 31) != 0ull;   // s_lshr_b64 s[98:99], s[58:59], 31
        hi = scc ? hi : lo;                      // s_cselect_b32 s59, s59, s58
        lo = scc ? lo : w;                       // s_cselect_b32 s58, s58, s41
        if (!scc) { r.popped = 1; r.cls = U2_POP_SLICE0; }  // s_addc_u32 s60, s60, -1
        head = ((uint64_t)hi << 32) | lo;
    } else {                                     // the side path: slice 1 refills, slice 0 cannot
        x_hi = lo & m1;                          // s_and_b32 s46, s58, s73
        head >>= p1;                             // s_lshr_b64 s[58:59], s[58:59], s77
        lo = (uint32_t)head;
        r.popped = 1; r.cls = U2_POP_SLICE1;     // s_sub_u32 s60, s60, 1
        hi = lo;                                 // s_mov_b32 s59, s58
        lo = w;                                  // s_mov_b32 s58, s41
        x_lo = lo & m0;                          // s_and_b32 s40, s58, s74
        head = (((uint64_t)hi << 32) | lo) >> p0;  // s_lshr_b64 s[58:59], s[58:59], s76
    }
    r.head = head;
    r.x = ((x_hi & 0xffffu) << 16) | (x_lo & 0xffffu);  // s_pack_ll_b32_b16 s40, s40, s46
    return r;
}

}  // namespace vidc
