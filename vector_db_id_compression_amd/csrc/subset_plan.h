// subset_plan.h -- the deciding half of the vidc_*_subset_dev calls (subset.h): what a subset refuses before any device work, the
// [i1, i2) range a positional subset type takes from a list, the ROC class of a list, the ID_MOD arithmetic and the bytes a call reads
// back.  Plain C++ (no HIP): the library runs these functions, on the host and inside its kernels, and tests/subset_plan_test.cpp
// compiles them with g++.
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

// the subset types of include/vidc.h ("subset"): Faiss's InvertedLists::subset_type_t
enum SubsetType : int { SUB_ID_RANGE = 0, SUB_ID_MOD = 1, SUB_ELEMENT_RANGE = 2, SUB_INVLIST_FRACTION = 3, SUB_INVLIST = 4 };

enum SubsetRefusal { SUB_OK = 0, SUB_NULL, SUB_TYPE, SUB_ARGS };

// the refusals every subset makes before any device work, in the order they are reported.  T = ntotal of the object (< 2^32).
inline SubsetRefusal subset_refusal(bool any_null, int type, uint64_t a1, uint64_t a2, uint64_t T) {
    if (any_null) return SUB_NULL;
    switch (type) {
    case SUB_ID_RANGE: return SUB_OK;  // (a1 >= a2 is the empty range)
    case SUB_ID_MOD: return a1 >= 1 && a2 < a1 ? SUB_OK : SUB_ARGS;
    case SUB_ELEMENT_RANGE: return a1 <= a2 && a2 <= T ? SUB_OK : SUB_ARGS;
    case SUB_INVLIST_FRACTION: return a1 >= 1 && a1 < (1ull << 32) && a2 < a1 ? SUB_OK : SUB_ARGS;
    case SUB_INVLIST: return SUB_OK;  // (bounds above nlist are clamped; a1 >= a2 takes nothing)
    default: return SUB_TYPE;
    }
}

// types 0 and 1 look at the ids, types 2 .. 4 at positions alone
VIDC_HD inline bool subset_by_id(int type) { return type == SUB_ID_RANGE || type == SUB_ID_MOD; }

// [i1, i2) of list l for the positional types: off0 = off[l], off1 = off[l + 1], T = ntotal > 0.  Every product fits 64 bits: offsets
// and T are below 2^32, a <= T (type 2), a2 + 1 <= a1 < 2^32 (type 3).  i1 > i2 can happen for type 2 (the bounds are differences of
// running totals): nothing is taken then, and [i1, i1) is returned.  i2 <= n always.
VIDC_HD inline void subset_bounds(int type, uint64_t a1, uint64_t a2, uint64_t T, uint64_t l, uint64_t off0, uint64_t off1, uint64_t &i1,
                                  uint64_t &i2) {
    const uint64_t n = off1 - off0;
    if (type == SUB_ELEMENT_RANGE) {
        i1 = off1 * a1 / T - off0 * a1 / T;
        i2 = off1 * a2 / T - off0 * a2 / T;
    } else if (type == SUB_INVLIST_FRACTION) {
        i1 = n * a2 / a1;
        i2 = n * (a2 + 1) / a1;
    } else {  // SUB_INVLIST
        const bool in = a1 <= l && l < a2;
        i1 = 0;
        i2 = in ? n : 0;
    }
    if (i2 < i1) i2 = i1;
}

// What the ROC splice does with a list of n ids that keeps n_new of them: its stream is copied (an empty list of the source is kept as
// it is), it becomes the empty list without any decode, or it is decoded and re-encoded.
enum SubsetClass : uint32_t { SUBC_KEEP = 0, SUBC_EMPTY = 1, SUBC_PARTIAL = 2 };
VIDC_HD inline uint32_t subset_roc_class(uint64_t n, uint64_t n_new) {
    if (n_new == n) return SUBC_KEEP;
    return n_new == 0 ? SUBC_EMPTY : SUBC_PARTIAL;
}

// ID_MOD: how id % a1 is computed.  A power of two is a mask; a1 < 2^32 reduces the high half first, so that no step divides more than
// 64 bits by 32 and an id below 2^32 takes one 32-bit remainder; a larger a1 takes the 64-bit remainder.
enum SubsetModKind : uint32_t { SUBM_MASK = 0, SUBM_U32 = 1, SUBM_U64 = 2 };
VIDC_HD inline uint32_t subset_mod_kind(uint64_t a1) {
    if ((a1 & (a1 - 1)) == 0) return SUBM_MASK;
    return a1 < (1ull << 32) ? SUBM_U32 : SUBM_U64;
}
VIDC_HD inline uint64_t subset_mod(uint64_t id, uint64_t a1, uint32_t kind) {
    if (kind == SUBM_MASK) return id & (a1 - 1);
    if (kind == SUBM_U32) {
        const uint32_t m = (uint32_t)a1, hi = (uint32_t)(id >> 32), lo = (uint32_t)id;
        if (hi == 0) return lo % m;
        const uint64_t r = hi % m;  // < 2^32: (r << 32 | lo) / m fits 32 bits
        return ((r << 32) | lo) % m;
    }
    return id % a1;
}

// the predicate of types 0 and 1 on one decoded id
VIDC_HD inline bool subset_takes_id(int type, uint64_t a1, uint64_t a2, uint32_t mod_kind, uint64_t id) {
    return type == SUB_ID_RANGE ? a1 <= id && id < a2 : subset_mod(id, a1, mod_kind) == a2;
}

// Bytes a call copies device -> host, all of them counts and list numbers (no id): packed bits and Elias-Fano read the size of the
// subset; ROC reads the word total of the splice and, for the id types, the candidate count, the candidates' numbers, the count of
// re-encoded lists with the survivor total and 8 bytes per re-encoded list.  The positional types of ROC read nothing else: the host
// finds the partial lists on its mirror of the offsets.
inline uint64_t subset_readback_bytes(bool roc, int type, uint64_t nlist, uint64_t T, uint64_t n_candidates, uint64_t n_reencoded) {
    if (!roc) return T ? 8 : 0;
    if (!nlist) return 0;
    if (subset_by_id(type) && T) return 8 + 8 + 4 * n_candidates + (n_candidates ? 16 + 8 * n_reencoded : 0);
    return 8;
}

}  // namespace vidc
