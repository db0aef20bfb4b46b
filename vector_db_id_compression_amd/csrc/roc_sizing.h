// roc_sizing.h -- how much scratch and how many member slots a ROC decoder takes for a list: pure integer arithmetic that the
// kernels (roc_kernels.h, roc_lane.h, roc_grp.h) and the host's decode planner (roc_dec_plan.h: dec_layout) must agree on, word for
// word -- a planner that allots less than a kernel uses lets two work items overlap.  One definition, no HIP include: the planner's
// test builds it with g++.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define VIDC_HD __host__ __device__
#else
#define VIDC_HD
#endif

namespace vidc {
namespace dev {

// capacity of a decoder's private stack scratch (dec_layout allots exactly this): the decoder pushes at most
// ~log2(n) bits per step, so streams of the encoder never outgrow the encoder's own arena bound; a stream whose
// precision is far below log2(n) (reference quirk domain) GROWS while it is decoded and needs that room
VIDC_HD inline uint32_t roc_dec_stack_cap(uint32_t n, uint32_t W) {
    const uint32_t a = (uint32_t)(((uint64_t)n * 37ull) >> 5) + 8u;
    return (a > W ? a : W) + 64u;
}

#define VIDC_DEC_CAP 16u       // members per fine bucket before spilling to the overflow list (lists <= 32768)
#define VIDC_DEC_CAP_BIG 64u   // same for longer lists (average bucket load up to 64)
VIDC_HD inline uint32_t roc_dec_cap(uint32_t n) { return n > 32768u ? VIDC_DEC_CAP_BIG : VIDC_DEC_CAP; }
#define VIDC_DEC_MAX_FB 12u    // <= 64 coarse x 64 fine buckets

// fine-bucket bits used by the decoder for a list of n elements with precision P (host + device)
VIDC_HD inline uint32_t roc_dec_fine_bits(uint32_t n, uint32_t P) {
    uint32_t lg = 0;
    while ((1u << lg) < n) lg++;
    uint32_t fb = lg > 3u ? lg - 3u : 0u;
    if (fb > VIDC_DEC_MAX_FB) fb = VIDC_DEC_MAX_FB;
    if (fb > P) fb = P;
    return fb;
}

// lane-per-list decoders: slots of one bucket row of a list of n ids on NB buckets
template <int NB>
VIDC_HD inline uint32_t roc_lane_cap_nb(uint32_t n) {
    // twice the mean + 16 (round 4; + 12 before: four of S2's 900 000 bucket-row lists -- 1089 .. 3291 ids -- overflowed a bucket,
    // and the pass that redoes them on the wave-per-list kernels waited for the whole decode first: 2.5 ms behind a 71 ms call)
    return (((n / (uint32_t)NB) * 2u + 16u) + 3u) & ~3u;
}
// align = 16 (round 5, RocDecArgs::row_align): rows start on 64-byte boundaries and are a multiple of 64 bytes long, so the four
// 16-byte chunks a step requests together lie in ONE 64-byte sector -- at align = 4 a row starts anywhere and they straddle two
// sectors three times out of four (S2: 1.45 sectors fetched per decoded id of the lane classes)
template <int NB>
VIDC_HD inline uint32_t roc_lane_cap_nb(uint32_t n, uint32_t align) {
    return align > 4u ? (roc_lane_cap_nb<NB>(n) + align - 1u) & ~(align - 1u) : roc_lane_cap_nb<NB>(n);
}

// row-per-list decoder, bucket geometry: 2^B value buckets, B = 8 + F (top 4 bits: registers, next 4: `mid`, last F: `leaf`)
VIDC_HD inline uint32_t roc_grp_dec_fbits(uint32_t n) {  // <= 8 members per bucket on average up to 32 768 ids
    return n <= 2048u ? 0u : (n <= 8192u ? 2u : (n <= 16384u ? 3u : 4u));
}
VIDC_HD inline uint32_t roc_grp_dec_cap(uint32_t n) { return n <= 32768u ? 32u : (n <= 65536u ? 64u : 96u); }
// member rows of one list: 2^(8 + F) rows of `cap` u32
VIDC_HD inline uint64_t roc_grp_dec_slots(uint32_t n) {
    return ((uint64_t)256u << roc_grp_dec_fbits(n)) * roc_grp_dec_cap(n);
}

}  // namespace dev
}  // namespace vidc
