// graph_search_ref.h -- the serial statement of one step of the best-first graph search (vidc_*_search_dev), host + device, no HIP
// runtime: the kernel of graph_search.hip calls the rules below and tests/graph_search_test.cpp builds them with g++
// (tests/graph_search_ref.py is the same in numpy, graph_search.search the statement both are held against).
//
// Per query: a pool of at most L entries ordered by (distance, node) ascending, an exact visited set of N bits.  One step takes the
// first unexpanded entry, marks it expanded and reads its row; every neighbour < N whose visited bit was clear is CLAIMED (the bit is
// set for good), gets its distance and is inserted; the best L stay.
//
// Key.  An entry is one 64-bit word: float32 bits of the squared distance << 32 | node << 1 | expanded.  A squared distance is never
// negative, so its bits order like its value; node < 2^31 leaves bit 0 for the flag.  A node enters the pool at most once (it is
// claimed at most once), so two entries never agree above bit 0 and every order comparison is on key >> 1: (distance, node).
//
// Insert by rank.  The pool is sorted, the C claimed candidates of a trip are not.  The place of an element of their union is the
// number of elements below it:   pool entry i: i + (candidates below it)     candidate: (pool entries below it) + (candidates below it)
// and the truncation keeps the places < L.  Taking the best L of the union trip by trip (rows wider than 64 fields) gives the best
// L of the whole row: an element dropped early has L better ones in front of it that only ever get replaced by better ones.
//
// Every loop is bounded by its arguments (L, the row's length, N), never by what the row holds.
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
namespace gs {

constexpr uint32_t MAX_L = 256;    // pool entries
constexpr uint32_t MAX_D = 2048;   // vector components
constexpr uint32_t TRIP = 64;      // row fields per trip: lane j takes field j

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

VIDC_HD inline uint64_t key_make(float dist, uint32_t node) { return ((uint64_t)f32_bits(dist) << 32) | ((uint64_t)node << 1); }
VIDC_HD inline uint32_t key_node(uint64_t k) { return (uint32_t)k >> 1; }
VIDC_HD inline float key_dist(uint64_t k) { return bits_f32((uint32_t)(k >> 32)); }
VIDC_HD inline bool key_expanded(uint64_t k) { return (k & 1ull) != 0; }
VIDC_HD inline uint64_t key_expand(uint64_t k) { return k | 1ull; }
VIDC_HD inline bool key_less(uint64_t a, uint64_t b) { return (a >> 1) < (b >> 1); }

// the steps a query may take: every node is expanded at most once, so N bounds the loop whatever the rows hold
VIDC_HD inline uint32_t step_bound(uint64_t N, uint32_t max_rounds) {
    const uint64_t cap = max_rounds ? (uint64_t)max_rounds : N;
    return (uint32_t)(cap < N ? cap : N);
}

// visited set: bit v of a word array (32-bit words: the claim is one atomic OR on the device)
VIDC_HD inline uint64_t vis_word(uint32_t v) { return v >> 5; }
VIDC_HD inline uint32_t vis_bit(uint32_t v) { return 1u << (v & 31u); }
// the claim rule: whoever flips the bit owns the candidate (`old` = the word in front of the OR)
VIDC_HD inline bool claim_won(uint32_t old, uint32_t bit) { return (old & bit) == 0u; }
// a decoded field is a candidate only below N: it is never used as an index otherwise
VIDC_HD inline bool id_usable(uint64_t v, uint64_t N) { return v < N; }

// entries of the ascending keys[0 .. n) below `key`
VIDC_HD inline uint32_t lower_bound(const uint64_t *keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key_less(keys[mid], key)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first unexpanded entry of keys[0 .. n), or n
VIDC_HD inline uint32_t first_unexpanded(const uint64_t *keys, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (!key_expanded(keys[i])) return i;
    return n;
}
VIDC_HD inline uint32_t merged_size(uint32_t P, uint32_t C, uint32_t L) { return P + C < L ? P + C : L; }
VIDC_HD inline bool place_kept(uint32_t place, uint32_t L) { return place < L; }

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

// ---- the serial search of one query, from the rules above (what tests/graph_search_test.cpp runs; the kernel does the same with a
// lane per row field).  pool / tmp: L words each; cand: TRIP words; vis: ceil(N / 32) words, zero.  row(node, j) -> field j of the
// decoded row of `node` (< 0: the row ended), row_len = fields per row.
struct Stats {
    uint32_t steps, dists;
};

template <typename Row>
inline uint32_t search_serial(uint64_t N, uint32_t row_len, Row row, const float *x, uint32_t d, const float *xq, uint32_t L, uint32_t entry,
                              uint32_t max_rounds, uint64_t *pool, uint64_t *tmp, uint64_t *cand, uint32_t *vis, Stats *st) {
    uint32_t P = 1;
    pool[0] = key_make(l2_serial(x + (uint64_t)entry * d, xq, d), entry);
    vis[vis_word(entry)] |= vis_bit(entry);
    st->steps = 0;
    st->dists = 1;
    const uint32_t bound = step_bound(N, max_rounds);
    for (uint32_t step = 0; step < bound; step++) {
        const uint32_t e = first_unexpanded(pool, P);
        if (e == P) break;
        const uint32_t node = key_node(pool[e]);
        pool[e] = key_expand(pool[e]);
        st->steps++;
        bool ended = false;
        for (uint32_t j0 = 0; j0 < row_len && !ended; j0 += TRIP) {
            uint32_t C = 0;
            for (uint32_t j = j0; j < row_len && j < j0 + TRIP; j++) {
                const int64_t f = row(node, j);
                if (f < 0) { ended = true; break; }
                if (!id_usable((uint64_t)f, N)) continue;
                const uint32_t v = (uint32_t)f, bit = vis_bit(v);
                const uint32_t old = vis[vis_word(v)];
                vis[vis_word(v)] = old | bit;
                if (!claim_won(old, bit)) continue;
                cand[C++] = key_make(l2_serial(x + (uint64_t)v * d, xq, d), v);
            }
            st->dists += C;
            // insert by rank, truncate at L
            for (uint32_t i = 0; i < P; i++) {
                uint32_t below = 0;
                for (uint32_t c = 0; c < C; c++) below += key_less(cand[c], pool[i]) ? 1u : 0u;
                if (place_kept(i + below, L)) tmp[i + below] = pool[i];
            }
            for (uint32_t c = 0; c < C; c++) {
                uint32_t below = lower_bound(pool, P, cand[c]);
                for (uint32_t c2 = 0; c2 < C; c2++) below += key_less(cand[c2], cand[c]) ? 1u : 0u;
                if (place_kept(below, L)) tmp[below] = cand[c];
            }
            P = merged_size(P, C, L);
            for (uint32_t i = 0; i < P; i++) pool[i] = tmp[i];
        }
    }
    return P;
}

}  // namespace gs
}  // namespace vidc
