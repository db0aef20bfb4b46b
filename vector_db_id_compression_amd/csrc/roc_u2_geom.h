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

// k_roc_decode_u2<20, true>: one level-2 counter per bitmap WORD, so that the rank inside an entry is the masked popcount of one word
// (the one-word step of the 18-bit launch).  u16 row[64][256] at the front -- element w = x >> 6 counts the inserted ids of level-1
// block w >> 8 in words below w (at most 255 * 64 = 16 320 for a set) -- and the bitmap of 2^20 bits behind it, word w at
// BITMAP_OFF + 8 w: exactly the 160 KiB a workgroup can have, no strip.  The insertion is a ds_or by all lanes: lane 0 ORs the bit
// into the bitmap dword x >> 5, lane j > 0 ORs 0 into dword j of the rows (an OR of 0 changes nothing).  The row update is a
// ds_add_u64 by all lanes: lane j owns the four fields of words 4 j .. 4 j + 3 of row L1 and adds 1 to those above w & 255.
// A decoded id is below 2^20 whatever the stream holds, so every address below lies inside LDS_BYTES.
// The functions are the step's address and data formation, instruction by instruction (tests/roc_u2_decword_geom_test.cpp).
struct U2DecWord {
    static constexpr uint32_t UB = 20u;
    static constexpr uint32_t ROWS_BYTES = 64u * 256u * 2u;
    static constexpr uint32_t BITMAP_OFF = ROWS_BYTES;
    static constexpr uint32_t BITMAP_BYTES = (1u << UB) / 8u;
    static constexpr uint32_t LDS_BYTES = BITMAP_OFF + BITMAP_BYTES;
    static constexpr uint64_t FIELD_ONES = 0x0001000100010001ull;
    static constexpr uint32_t row_addr(uint32_t x) { return 2u * (x >> 6); }                  // ds_read_u16
    static constexpr uint32_t word_addr(uint32_t x) { return BITMAP_OFF + 8u * (x >> 6); }    // ds_read_b64
    static constexpr uint32_t ins_mul(uint32_t lane) { return lane == 0u ? 4u : 0u; }
    static constexpr uint32_t ins_add(uint32_t lane) { return lane == 0u ? BITMAP_OFF : 4u * lane; }
    static constexpr uint32_t ins_addr(uint32_t x, uint32_t lane) { return (x >> 5) * ins_mul(lane) + ins_add(lane); }  // ds_or_b32
    static constexpr uint32_t ins_data(uint32_t x, uint32_t lane) { return (lane == 0u ? 1u : 0u) << (x & 31u); }
    static constexpr uint32_t add_addr(uint32_t x, uint32_t lane) { return ((x >> 14) << 9) + 8u * lane; }  // ds_add_u64
    // 16 * (fields of the lane at or below w & 255), clamped to 0 .. 63: a 64-bit shift takes six bits of its count, so "no field"
    // is a shift by 63 (the lowest one lands on bit 63) and the AND that follows takes that bit away
    static constexpr uint32_t add_shift(uint32_t x, uint32_t lane) {
        const int32_t t = (int32_t)(16u * ((x >> 6) & 255u)) + 16 - 64 * (int32_t)lane;
        return (uint32_t)(t < 0 ? 0 : (t > 63 ? 63 : t));
    }
    static constexpr uint64_t add_data(uint32_t x, uint32_t lane) { return (FIELD_ONES << add_shift(x, lane)) & 0x7fffffffffffffffull; }
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
