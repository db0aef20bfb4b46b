// merge_plan.h -- the deciding half of the vidc_*_merge_dev calls (merge.h): which source a merged ROC list takes its stream from, what
// a merge refuses before any device work, and what the largest shifted id may be.  Plain C++ (no HIP): the library runs these
// functions, on the host and inside its kernels, and tests/merge_plan_test.cpp compiles them with g++.
#pragma once
#include <stdint.h>

#ifndef VIDC_HD
#ifdef __HIPCC__
#define VIDC_HD __host__ __device__
#else
#define VIDC_HD
#endif
#endif

namespace vidc {

// Where list l of a merged ROC object comes from.  The values are the source numbers of the splice (roc.hip): 0 = a, 1 = b, 2 = the
// fresh encode of the lists that are decoded on both sides.
enum MergeClass : uint32_t { MRG_KEEP_A = 0, MRG_KEEP_B = 1, MRG_ENCODE = 2 };

// a_n, b_n: ids of the list on each side; shifted: add_id != 0.  A list with nothing from b keeps a's stream (an empty list of both
// sides is a's empty list); a list with nothing from a keeps b's stream when its ids are not shifted; every other list is re-encoded.
VIDC_HD inline uint32_t merge_roc_class(uint64_t a_n, uint64_t b_n, bool shifted) {
    if (b_n == 0) return MRG_KEEP_A;
    if (a_n == 0 && !shifted) return MRG_KEEP_B;
    return MRG_ENCODE;
}

enum MergeRefusal { MRG_OK = 0, MRG_NULL, MRG_NLIST, MRG_DEVICE, MRG_NTOTAL };

// the refusals every merge makes before any device work, in the order they are reported
inline MergeRefusal merge_refusal(bool any_null, uint64_t nlist_a, uint64_t nlist_b, int dev_ctx, int dev_a, int dev_b, uint64_t ntotal_a,
                                  uint64_t ntotal_b) {
    if (any_null) return MRG_NULL;
    if (nlist_a != nlist_b) return MRG_NLIST;
    if (dev_a != dev_ctx || dev_b != dev_ctx) return MRG_DEVICE;
    if (ntotal_a >= 0xffffffffull || ntotal_b >= 0xffffffffull || ntotal_a + ntotal_b >= 0xffffffffull) return MRG_NTOTAL;
    return MRG_OK;
}

// max_b: the largest id of the shifted side (only read when it holds ids).  True when max_b + add_id leaves 64 bits or does not fit
// `bits` (64: every id fits).
inline bool merge_shift_overflows(uint64_t max_b, uint64_t add_id, uint32_t bits) {
    const uint64_t s = max_b + add_id;
    if (s < max_b) return true;
    return bits < 64u && (s >> bits) != 0;
}

}  // namespace vidc
