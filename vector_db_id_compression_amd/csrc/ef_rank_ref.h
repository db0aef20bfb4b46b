// ef_rank_ref.h -- the arithmetic of a rank inside one Elias-Fano list (vidc_ef_rank_dev), host + device, no HIP runtime: the kernels of
// ef.hip call it and tests/ef_rank_test.cpp builds it with g++ (tests/ef_rank_ref.py is the same in numpy).
//
// A list of m ascending ids, l low bits, largest id u (ef.hip's layout comment): element i sets high bit (x_i >> l) + i, so the high
// stream is unary -- bucket h (the elements whose high part is h) is the run of ones in front of zero number h.  With
//   select0(j) = position of zero number j (0-based)
//   p0 = h ? select0(h - 1) + 1 : 0        p1 = select0(h)
// the bucket holds the elements r0 = p0 - h .. r0 + c - 1, c = p1 - p0, and the rank of x (elements < x) with h = x >> l is
// r0 + the lower bound of x's low l bits among the bucket's low fields.  For x <= u the stream holds (u >> l) + 2 >= h + 2 zeros.
//
// select0 uses the select directory the object already carries (hrank[k] = ones in front of batch k of 64 high words): the zeros in
// front of batch k are 4096 k - hrank[k], non-decreasing in k; the batch of zero j is the LAST one with that figure <= j (a batch of
// ones only and its successor tie; the later one holds the zero).  Inside the batch: popcounts of the inverted words, then the k-th
// set bit of one inverted word.
//
// Every loop here is bounded by its arguments' sizes (nb, 64 bits, c), never by the bits read: a damaged image cannot make a caller
// that clamps r0 and c to m (ef_rank_clamp) read outside the list.
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
namespace efr {

constexpr uint64_t BATCH_BITS = 4096;  // high bits per directory entry (EF_BATCH_BITS)

VIDC_HD inline uint32_t popc(uint64_t w) { return (uint32_t)__builtin_popcountll(w); }

// zeros in front of batch k, from its directory entry
VIDC_HD inline uint64_t zeros_before_batch(uint64_t k, uint32_t hrank_k) { return BATCH_BITS * k - hrank_k; }

// the last batch k < nb with zeros_before_batch(k) <= j (nb >= 1; batch 0 has no zero in front of it, so one always exists)
VIDC_HD inline uint64_t batch_of_zero(const uint32_t *hrank, uint64_t nb, uint64_t j) {
    uint64_t lo = 0, hi = nb;  // invariant: zeros_before(lo) <= j < zeros_before(hi) (hi == nb: behind the list)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (zeros_before_batch(mid, hrank[mid]) <= j) lo = mid; else hi = mid;
    }
    return lo;
}

// position of set bit number k (0-based) of w; k < popcount(w).  Six halving steps (a k that is too large ends at a position <= 63).
VIDC_HD inline uint32_t select_in_word(uint64_t w, uint32_t k) {
    uint32_t pos = 0;
    for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t c = popc((w >> pos) & ((1ull << s) - 1ull));
        if (k >= c) { k -= c; pos += s; }
    }
    return pos;
}

// the inverted high word `wi` of a list of nhw words: its set bits are the stream's zeros; words at or beyond nhw hold none
VIDC_HD inline uint64_t zero_word(const uint64_t *high, uint64_t nhw, uint64_t wi) { return wi < nhw ? ~high[wi] : 0ull; }

// the l-bit field at bit position pos of an LSB-first word stream of nw words (a field that would cross the last word reads zeros
// behind it: the CSR streams carry a padding word, the arena records do not)
VIDC_HD inline uint64_t low_field(const uint64_t *low, uint64_t nw, uint64_t pos, uint32_t l) {
    if (!l) return 0;
    const uint64_t w = pos >> 6;
    const uint32_t sh = (uint32_t)(pos & 63);
    uint64_t v = w < nw ? low[w] >> sh : 0ull;
    if (sh + l > 64 && w + 1 < nw) v |= low[w + 1] << (64 - sh);
    return l >= 64 ? v : (v & ((1ull << l) - 1ull));
}

// r0 and c of a bucket from the two zero positions, kept inside a list of m elements whatever the stream held
struct Bucket {
    uint64_t r0, c;
};
VIDC_HD inline Bucket ef_rank_clamp(uint64_t p0, uint64_t p1, uint64_t h, uint64_t m) {
    Bucket b;
    b.r0 = p0 >= h ? p0 - h : 0;
    if (b.r0 > m) b.r0 = m;
    b.c = p1 >= p0 ? p1 - p0 : 0;
    if (b.c > m - b.r0) b.c = m - b.r0;
    return b;
}

// first k in [0, c) with field(r0 + k) >= xl, or c: the fields of a bucket ascend (the list does)
VIDC_HD inline uint64_t bucket_lower_bound(const uint64_t *low, uint64_t nw, uint32_t l, uint64_t r0, uint64_t c, uint64_t xl) {
    uint64_t lo = 0, hi = c;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (low_field(low, nw, (r0 + mid) * l, l) < xl) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct RankResult {
    uint64_t rank;
    uint32_t found;
};

// the rank inside a bucket (both zero positions known); l == 0: every element of the bucket equals x
VIDC_HD inline RankResult rank_in_bucket(const uint64_t *low, uint64_t nw, uint32_t l, uint64_t m, uint64_t x, uint64_t p0, uint64_t p1) {
    const uint64_t h = l >= 64 ? 0 : x >> l;
    const Bucket b = ef_rank_clamp(p0, p1, h, m);
    RankResult r;
    if (!l) {
        r.rank = b.r0;
        r.found = b.c > 0;
        return r;
    }
    const uint64_t xl = l >= 64 ? x : (x & ((1ull << l) - 1ull));
    const uint64_t k = bucket_lower_bound(low, nw, l, b.r0, b.c, xl);
    r.rank = b.r0 + k;
    r.found = k < b.c && low_field(low, nw, (b.r0 + k) * l, l) == xl;
    return r;
}

// select0(j) of one list, one thread: the directory search, then the batch's words one at a time (the kernels scan them in parallel;
// the arena rows, which have no directory, walk their few words the same way with nb == 1 and hrank == {0}).  A zero that the
// stream does not hold (damaged image) answers nhw * 64.
VIDC_HD inline uint64_t select0_serial(const uint64_t *high, uint64_t nhw, const uint32_t *hrank, uint64_t nb, uint64_t j) {
    const uint64_t k = nb ? batch_of_zero(hrank, nb, j) : 0;
    uint64_t need = j - (nb ? zeros_before_batch(k, hrank[k]) : 0);
    const uint64_t w1 = k * 64 + 64 < nhw ? k * 64 + 64 : nhw;
    for (uint64_t wi = k * 64; wi < w1; wi++) {
        const uint64_t z = ~high[wi];
        const uint32_t c = popc(z);
        if (need < c) return wi * 64 + select_in_word(z, (uint32_t)need);
        need -= c;
    }
    return nhw * 64;
}

// the whole rank of x in one list, one thread (the reference the tests hold the kernels' parts against, and the arena kernel's body)
VIDC_HD inline RankResult rank_serial(const uint64_t *low, uint64_t nlw, const uint64_t *high, uint64_t nhw, const uint32_t *hrank, uint64_t nb,
                                      uint64_t m, uint32_t l, uint64_t u, uint64_t x) {
    RankResult r;
    r.rank = 0; r.found = 0;
    if (!m) return r;
    if (x > u) { r.rank = m; return r; }
    const uint64_t h = x >> l;  // (x <= u: l <= 63)
    const uint64_t p0 = h ? select0_serial(high, nhw, hrank, nb, h - 1) + 1 : 0;
    const uint64_t p1 = select0_serial(high, nhw, hrank, nb, h);
    return rank_in_bucket(low, nlw, l, m, x, p0, p1);
}

}  // namespace efr
}  // namespace vidc
