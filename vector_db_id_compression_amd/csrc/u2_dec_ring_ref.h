// u2_dec_ring_ref.h -- the ring traffic of a k_roc_decode_u2 step in plain C++ (no HIP: tests/u2_dec_ring_test.cpp runs both forms
// against each other on the host, tests/roc_dec_ring_ref.py is the same in Python).  It continues u2_pops_ref.h: one decode step from
// head' (the head the previous step left, >= 2^31) to the multiplicand H of "head = H * nmax + rank".
//   u2_dec_ring_ref   the reference form: u2_pops_one, then the index push of codec.cpp:44-63 as U2_DEC_MID_W runs it (the word goes to
//                     slot sp in EVERY step; sp moves over it only if H renormalises), then the read of the carried word.
//   u2_dec_ring_cls   the classified form (U2_DEC_STEP bit 2: U2_DEC_TOP_Q / U2_DEC_SIDE_Q, register by register): one class out of
//                     h = head' >> (p1 + p0) and lq = 2^31 / nmax.  Quiet: H = h, sp, the carried word and the ring untouched.  Every
//                     other class runs the reference sequence.
// On the common path (head' >= 2^(31 + p1)) the refill of the pops and the spill of the push do one of four things:
//   h < lq                refill, no spill    H = (h << 32) | w, sp - 1                                   U2_RING_REFILL
//   lq <= h < 2^31        refill and spill    the spill puts w back into the slot it came from: H = h     U2_RING_QUIET
//   2^31 <= h < lq 2^32   neither             H = h (the reference form writes h_lo ABOVE the top)        U2_RING_QUIET
//   h >= lq 2^32          spill, no refill    H = h_hi, h_lo to slot sp, sp + 1                           U2_RING_SPILL
// so quiet iff lq <= h < lq 2^32.  lq >= 2^15 for nmax <= 65 536 and h < 2^63 (p1 + p0 >= 1), so the two halves never meet.
// U2_RING_SPILL is empty while nmax <= 2^P (h_hi < 2^(31 - P) <= lq); a multiset or imported stream may reach it, so the test is two-sided.
#pragma once
#include <stdint.h>

#include "u2_pops_ref.h"

namespace vidc {

enum U2RingClass : uint32_t { U2_RING_QUIET = 0, U2_RING_REFILL = 1, U2_RING_SPILL = 2, U2_RING_SIDE = 3 };  // SIDE: slice 1 refilled (U2_DEC_SIDE_P)

struct U2DecRing {
    uint32_t cls;    // U2RingClass
    uint64_t H;      // the multiplicand
    uint32_t x;      // the id
    uint32_t sp;     // stack pointer behind the step's first half
    uint32_t w;      // the carried word of the next step: ring[(sp - 1) & 63]
    uint32_t wrote;  // 1 if a ring slot was written ...
    uint32_t slot;   // ... which one ...
    uint32_t word;   // ... and what
};

inline uint32_t u2_ring_lq(uint32_t nmax) { return 0x80000000u / nmax; }

// the class of a common-path step from h and lq alone
inline uint32_t u2_ring_class(uint64_t h, uint32_t lq) {
    return h < (uint64_t)lq ? U2_RING_REFILL : (uint32_t)(h >> 32) >= lq ? U2_RING_SPILL : U2_RING_QUIET;
}

// index push, first half (codec.cpp:44-63 as U2_DEC_MID_W / the side body run it): head -> H, the word at slot sp, the carried word
inline void u2_ring_push(uint64_t head, uint32_t lq, uint32_t *ring, U2DecRing &r) {
    const uint32_t lo = (uint32_t)head, hi = (uint32_t)(head >> 32);
    r.wrote = 1; r.slot = r.sp & 63u; r.word = lo;
    ring[r.slot] = lo;                            // s_and_b32 m0, s60, 63; v_writelane_b32 v5, s58, m0
    const bool spill = hi >= lq;                  // s_cmp_ge_u32 s59, s62
    r.H = spill ? (uint64_t)hi : head;            // s_cselect_b32 (twice)
    r.sp += spill ? 1u : 0u;                      // s_addc_u32 s60, s60, 0
    r.w = ring[(r.sp - 1u) & 63u];                // s_sub_u32 s42, s60, 1; v_readlane_b32 s41, v5, s42
}

// the reference form; ring: the 64 slots of v5, sp: s60
inline U2DecRing u2_dec_ring_ref(uint64_t head, uint32_t sp, uint32_t *ring, uint32_t lq, uint32_t p1, uint32_t p0) {
    const U2Pops p = u2_pops_one(head, ring[(sp - 1u) & 63u], p1, p0);
    U2DecRing r{0, 0, p.x, sp - p.popped, 0, 0, 0, 0};
    u2_ring_push(p.head, lq, ring, r);
    const bool spilled = r.sp != sp - p.popped;
    r.cls = p.cls == U2_POP_SLICE1 ? U2_RING_SIDE : (p.popped == 1u) == spilled ? U2_RING_QUIET : spilled ? U2_RING_SPILL : U2_RING_REFILL;
    return r;
}

// the classified form; w: the carried word (s41), which every way into the loop and every loud step leave equal to ring[(sp - 1) & 63]
inline U2DecRing u2_dec_ring_cls(uint64_t head, uint32_t sp, uint32_t *ring, uint32_t w, uint32_t lq, uint32_t p1, uint32_t p0) {
    const uint32_t thr = 31u + p1, bfe = (p0 << 16) | p1, sh = p1 + p0;  // s56, s57, s63
    const uint32_t m1 = (1u << p1) - 1u, m0 = p0 >= 32u ? ~0u : (1u << p0) - 1u;  // s73, s74
    U2DecRing r{U2_RING_QUIET, 0, 0, sp, w, 0, 0, 0};
    uint32_t x_hi, x_lo;
    if ((head >> (thr & 63u)) != 0ull) {                  // s_lshr_b64 s[98:99], s[58:59], s56; s_cbranch_scc0 side
        x_hi = (uint32_t)head & m1;                       // s_and_b32 s46, s58, s73
        x_lo = u2_s_bfe_u32((uint32_t)head, bfe);         // s_bfe_u32 s40, s58, s57
        head >>= (sh & 63u);                              // s_lshr_b64 s[58:59], s[58:59], s63: h
        uint32_t lo = (uint32_t)head, hi = (uint32_t)(head >> 32);
        const bool borrow = head < (uint64_t)lq;          // s_sub_u32 s98, s58, s62; s_subb_u32 s98, s59, 0
        const uint32_t t = borrow ? 0xffffffffu : hi;     // s_cselect_b32 s98, -1, s59
        if (t >= lq) {                                    // s_cmp_ge_u32 s98, s62; s_cbranch_scc1 loud
            const bool scc = (head >> 31) != 0ull;        // s_lshr_b64 s[98:99], s[58:59], 31
            hi = scc ? hi : lo;                           // s_cselect_b32 s59, s59, s58
            lo = scc ? lo : w;                            // s_cselect_b32 s58, s58, s41
            r.sp -= scc ? 0u : 1u;                        // s_addc_u32 s60, s60, -1
            r.cls = scc ? U2_RING_SPILL : U2_RING_REFILL;
            u2_ring_push(((uint64_t)hi << 32) | lo, lq, ring, r);
        } else {
            r.H = head;                                   // quiet: the multiply reads s[58:59]
        }
    } else {                                              // the side body: slice 1 refills, slice 0 cannot
        x_hi = (uint32_t)head & m1;                       // s_and_b32 s46, s58, s73
        head >>= p1;                                      // s_lshr_b64 s[58:59], s[58:59], s77
        r.sp -= 1u;                                       // s_sub_u32 s60, s60, 1
        const uint32_t hi = (uint32_t)head, lo = w;       // s_mov_b32 s59, s58; s_mov_b32 s58, s41
        x_lo = lo & m0;                                   // s_and_b32 s40, s58, s74
        r.cls = U2_RING_SIDE;
        u2_ring_push((((uint64_t)hi << 32) | lo) >> p0, lq, ring, r);  // s_lshr_b64 s[58:59], s[58:59], s76
    }
    r.x = ((x_hi & 0xffffu) << 16) | (x_lo & 0xffffu);    // s_pack_ll_b32_b16 s40, s40, s46
    return r;
}

}  // namespace vidc
