// ivf_scan_ref.h -- the serial statement of the IVF list scan (vidc_ivf_scan_dev), host + device, no HIP runtime: the kernels of
// ivf_scan.hip call the rules below and tests/ivf_scan_test.cpp builds them with g++ (tests/ivf_scan_ref.py is the same in numpy).
//
// Per query: the candidates are all entries of the distinct valid lists its probe row names; the result is the first k of them in
// ascending (distance, label) order, label = list_no << 32 | offset.
//
// Key.  A candidate is one 64-bit word: float32 bits of the squared distance << 32 | the position in the code array
// (offsets[list] + offset).  A squared distance is never negative, so its bits order like its value; lists lie in list order, so
// position order is label order.  Every position is scanned at most once per query (the probe row is de-duplicated), so the keys of a
// query are distinct and the k smallest are the same set however the row was cut.  ~0 is no key (ntotal < 2^32: a position is at
// most 2^32 - 2): it pads a pool that holds fewer than k candidates.
//
// Insert by rank.  The pool is k sorted keys (padded), the C survivors of a trip are not sorted.  The place of an element of their
// union is the number of elements below it:  pool entry i: i + (survivors below it)   survivor: (pool entries below it) + (survivors
// below it); places < k stay.  The S-way merge of the split is the same rule over S sorted runs.
//
// Every loop is bounded by its arguments (k, nprobe, the clamped length of a list), never by what the arrays hold.
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
namespace ivs {

constexpr uint32_t MAX_K = 256;        // results per query (= pool entries)
constexpr uint32_t MAX_NPROBE = 1024;  // probes per query
constexpr uint32_t MAX_D = 2048;       // vector components
constexpr uint32_t MAX_M = 64;         // PQ sub-quantisers
constexpr uint32_t MAX_S = 16;         // pieces a probe row is cut into
constexpr uint32_t TRIP = 64;          // codes per trip: lane c takes code c
constexpr uint64_t EMPTY = ~0ull;      // no key

enum { FLAT = 0, PQ8 = 1 };  // VIDC_IVF_FLAT, VIDC_IVF_PQ8

VIDC_HD inline uint32_t f32_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
VIDC_HD inline float bits_f32(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

VIDC_HD inline uint64_t key_make(float dist, uint32_t pos) { return ((uint64_t)f32_bits(dist) << 32) | pos; }
VIDC_HD inline uint32_t key_pos(uint64_t k) { return (uint32_t)k; }
VIDC_HD inline float key_dist(uint64_t k) { return bits_f32((uint32_t)(k >> 32)); }
VIDC_HD inline bool key_less(uint64_t a, uint64_t b) { return a < b; }
// the drop test: a candidate that is not below the pool's last key cannot enter it
VIDC_HD inline bool key_dropped(uint64_t key, uint64_t last) { return !key_less(key, last); }

// a probe -> the list it names, or -1 (negative, or >= nlist: Faiss writes -1 for "no list")
VIDC_HD inline int32_t probe_list(int64_t p, uint64_t nlist) { return (p >= 0 && (uint64_t)p < nlist) ? (int32_t)p : -1; }
// the duplicate rule: of equal lists in a row the first stays.  row: the lists of probe_list; -> row[j] names a list an earlier
// entry named.  (Clearing the later ones in place, in ascending j, gives the same row: the first occurrence is never cleared.)
VIDC_HD inline bool probe_repeats(const int32_t *row, uint32_t j) {
    bool dup = false;
    for (uint32_t i = 0; i < j; i++) dup = dup || row[i] == row[j];
    return dup && row[j] >= 0;
}
// piece s of S of a row of nprobe entries: [piece_begin(s), piece_begin(s + 1)), cut after the de-duplication
VIDC_HD inline uint32_t piece_begin(uint32_t nprobe, uint32_t S, uint32_t s) { return (uint32_t)((uint64_t)s * nprobe / S); }

// a list's range, clamped to a <= b <= ntotal before it indexes the codes
struct Range {
    uint64_t a, b;
};
VIDC_HD inline Range list_range(uint64_t off_a, uint64_t off_b, uint64_t ntotal) {
    Range r;
    r.b = off_b < ntotal ? off_b : ntotal;
    r.a = off_a < r.b ? off_a : r.b;
    return r;
}

// entries of the ascending keys[0 .. n) below `key`
VIDC_HD inline uint32_t lower_bound(const uint64_t *keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key_less(keys[mid], key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
VIDC_HD inline bool place_kept(uint32_t place, uint32_t k) { return place < k; }

// the place of entry i of run s in the merge of S sorted runs of k keys each (runs[s * k + i]; EMPTY pads a run and is never asked for)
VIDC_HD inline uint32_t merge_place(const uint64_t *runs, uint32_t S, uint32_t k, uint32_t s, uint32_t i) {
    const uint64_t key = runs[(uint64_t)s * k + i];
    uint32_t place = i;
    for (uint32_t t = 0; t < S; t++)
        if (t != s) place += lower_bound(runs + (uint64_t)t * k, k, key);
    return place;
}

// the list that holds position pos: the last l with offsets[l] <= pos (empty lists in front of it share its offset and lose).  The
// index stays inside [0, nlist) whatever the offsets hold.  nlist >= 1.
VIDC_HD inline uint32_t list_of(const uint64_t *offsets, uint64_t nlist, uint64_t pos) {
    uint64_t lo = 0, hi = nlist;  // invariant: the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= pos) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}
VIDC_HD inline int64_t label_make(uint32_t list, uint64_t offset) { return (int64_t)(((uint64_t)list << 32) | (offset & 0xffffffffull)); }
VIDC_HD inline int64_t key_label(const uint64_t *offsets, uint64_t nlist, uint64_t key) {
    const uint32_t l = list_of(offsets, nlist, key_pos(key));
    return label_make(l, (uint64_t)key_pos(key) - offsets[l]);
}

// squared L2 in float32, components in order (the kernel sums in lane groups: on the integer grids of the tests every order gives
// the same exact integer, on float data the tests allow the summation bound)
VIDC_HD inline float l2_serial(const float *a, const float *b, uint32_t d) {
    float s = 0.f;
    for (uint32_t i = 0; i < d; i++) {
        const float t = a[i] - b[i];
        s += t * t;
    }
    return s;
}
// PQ8: entry (m, c) of the query's table = || xq_m - codebook[m][c] ||^2; a code's distance is the sum of its M entries in m order
VIDC_HD inline float pq_entry(const float *xq, const float *codebooks, uint32_t dsub, uint32_t m, uint32_t c) {
    return l2_serial(xq + (uint64_t)m * dsub, codebooks + ((uint64_t)m * 256u + c) * dsub, dsub);
}

// ---- the serial scan of one (query, piece), from the rules above (what tests/ivf_scan_test.cpp runs; the kernel does the same with
// a lane per code).  row: nprobe words of scratch; pool / tmp: k words each; cand: TRIP words.  table: M * 256 floats (PQ8), or NULL.
// -> pool holds the k best keys of the piece, EMPTY padded.  st: {lists scanned, codes scanned} of the piece.
struct Stats {
    uint32_t lists, codes;
};

inline void insert_trip(uint64_t *pool, uint64_t *tmp, uint32_t k, const uint64_t *cand, uint32_t C) {
    for (uint32_t i = 0; i < k; i++) {
        uint32_t below = 0;
        for (uint32_t c = 0; c < C; c++) below += key_less(cand[c], pool[i]) ? 1u : 0u;
        if (place_kept(i + below, k)) tmp[i + below] = pool[i];
    }
    for (uint32_t c = 0; c < C; c++) {
        uint32_t below = lower_bound(pool, k, cand[c]);
        for (uint32_t c2 = 0; c2 < C; c2++) below += key_less(cand[c2], cand[c]) ? 1u : 0u;
        if (place_kept(below, k)) tmp[below] = cand[c];
    }
    for (uint32_t i = 0; i < k; i++) pool[i] = tmp[i];
}

inline void scan_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, int kind, uint32_t d, uint32_t M,
                        const float *codebooks, const float *xq, uint32_t nprobe, const int64_t *probes, uint32_t k, uint32_t S, uint32_t s,
                        int32_t *row, float *table, uint64_t *pool, uint64_t *tmp, uint64_t *cand, Stats *st) {
    for (uint32_t j = 0; j < nprobe; j++) row[j] = probe_list(probes[j], nlist);
    for (uint32_t j = 0; j < nprobe; j++)
        if (probe_repeats(row, j)) row[j] = -1;
    const uint32_t dsub = kind == PQ8 ? d / M : 0;
    if (kind == PQ8)
        for (uint32_t e = 0; e < M * 256u; e++) table[e] = pq_entry(xq, codebooks, dsub, e >> 8, e & 255u);
    for (uint32_t i = 0; i < k; i++) pool[i] = EMPTY;
    st->lists = st->codes = 0;
    const uint64_t code_size = kind == PQ8 ? (uint64_t)M : (uint64_t)d * 4;
    for (uint32_t j = piece_begin(nprobe, S, s); j < piece_begin(nprobe, S, s + 1); j++) {
        if (row[j] < 0) continue;
        const Range r = list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
        st->lists++;
        st->codes += (uint32_t)(r.b - r.a);
        for (uint64_t p0 = r.a; p0 < r.b; p0 += TRIP) {
            uint32_t C = 0;
            for (uint64_t p = p0; p < r.b && p < p0 + TRIP; p++) {
                const uint8_t *code = codes + p * code_size;
                float dist = 0.f;
                if (kind == PQ8) {
                    for (uint32_t m = 0; m < M; m++) dist += table[m * 256u + code[m]];
                } else {
                    for (uint32_t i = 0; i < d; i++) {  // (byte copies: the code array need not be aligned here)
                        float v;
                        __builtin_memcpy(&v, code + (uint64_t)i * 4, 4);
                        const float t = xq[i] - v;
                        dist += t * t;
                    }
                }
                const uint64_t key = key_make(dist, (uint32_t)p);
                if (!key_dropped(key, pool[k - 1])) cand[C++] = key;
            }
            if (C) insert_trip(pool, tmp, k, cand, C);
        }
    }
}

// the S runs of a query -> its k result keys (EMPTY padded); out: k words
inline void merge_serial(const uint64_t *runs, uint32_t S, uint32_t k, uint64_t *out) {
    for (uint32_t i = 0; i < k; i++) out[i] = EMPTY;
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t i = 0; i < k; i++) {
            if (runs[(uint64_t)s * k + i] == EMPTY) continue;
            const uint32_t place = merge_place(runs, S, k, s, i);
            if (place_kept(place, k)) out[place] = runs[(uint64_t)s * k + i];
        }
}

}  // namespace ivs
}  // namespace vidc
