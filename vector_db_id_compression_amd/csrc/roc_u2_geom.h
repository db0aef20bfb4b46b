// roc_u2_geom.h -- LDS geometry of the round-2 ROC chain kernels (roc_u2.h): plain constants, no device code, so that a host
// compiler can check them (tests/roc_u2_geom_test.cpp).
#pragma once
#include <stdint.h>

namespace vidc {
namespace dev {

template <int UB>
struct U2Geom {
    static_assert(UB == 18 || UB == 20, "universe bits");
    static constexpr uint32_t GSH = UB == 20 ? 2u : 0u;   // log2(bitmap words per level-2 entry)
    static constexpr uint32_t G = 1u << GSH;
    static constexpr uint32_t ESH = 6u + GSH;             // id bits below the entry index
    static constexpr uint32_t NE = 4096u;                 // 64 blocks x 64 entries
    static constexpr uint32_t BITMAP_BYTES = NE * G * 8u;
    static constexpr uint32_t LDS_BYTES = BITMAP_BYTES + 16u;  // + a dummy word: target of the "no pending removal" store
    // k_roc_decode_u2: the level-2 counters u32 row[64][64] in FRONT of the bitmap (row[L1][L2] is dword `entry`; a DS offset field
    // has 16 bits, so nothing that wants one can sit behind a 128 KiB bitmap), and a strip of one dword per lane behind the bitmap.
    // The insertion is a ds_or by ALL lanes: lane 0 hits the bitmap, lane j > 0 its own dword of the strip (no exec write in the step,
    // no two lanes on one address).  147 712 bytes with 20 universe bits, 49 408 with 18 (no set_big_lds).
    static constexpr uint32_t DEC_ROWS_BYTES = 64u * 64u * 4u;
    static constexpr uint32_t DEC_BITMAP_OFF = DEC_ROWS_BYTES;
    static constexpr uint32_t DEC_STRIP_OFF = DEC_BITMAP_OFF + BITMAP_BYTES;
    static constexpr uint32_t DEC_LDS_BYTES = DEC_STRIP_OFF + 256u;
};

// Dense 16-id blocks in POSITION space (k_roc_encode_u2<20> only, lists of 4097 .. 65 536 ids): block b holds the ids at positions
// 16 b .. 16 b + 15 of the ascending input as 16 u16 slots (id - first id of the block) and the first id in a u32 table.  Blocks are
// stored in REVERSED order like the bitmap entries (storage index e = 4095 - b = L1 * 64 + L2 of the reversed counters).  The base
// table sits in FRONT of the slots so that its read takes the 16-bit offset field (one address instruction instead of two); a step
// reads 64 u16 from the block's first slot on, i.e. up to 96 bytes past the block: the pad behind the last block.
struct U2Dense {
    static constexpr uint32_t MIN_N = 4096u;              // shorter lists stay with the lane / general kernels anyway
    static constexpr uint32_t MAX_N = 65536u;             // 4096 blocks
    static constexpr uint32_t BASE_OFF = 16u;             // u32 base[4096]
    static constexpr uint32_t SLOT_OFF = BASE_OFF + 4096u * 4u;  // u16 slot[4096][16]
    // behind the pad: a strip of one dword per lane.  The removal's ds_write_b16 runs in ALL lanes: a lane that shifts hits the slot
    // below its own, every other lane its own dword of the strip (no exec write in the step, no two lanes on one address)
    static constexpr uint32_t STRIP_OFF = SLOT_OFF + 4096u * 32u + 128u;
    static constexpr uint32_t LDS_BYTES = STRIP_OFF + 256u;
};
// LDS bytes of a k_roc_encode_u2<UB, *> launch
template <int UB>
constexpr uint32_t u2_enc_lds_bytes(bool dense) {
    return UB == 20 && dense && U2Dense::LDS_BYTES > U2Geom<UB>::LDS_BYTES ? U2Dense::LDS_BYTES : U2Geom<UB>::LDS_BYTES;
}

}  // namespace dev
}  // namespace vidc
