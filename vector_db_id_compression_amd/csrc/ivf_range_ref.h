// ivf_range_ref.h -- the serial statement of the IVF range search (vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev), host + device,
// no HIP runtime: the kernels of ivf_range.hip call the rules below and tests/ivf_range_test.cpp builds them with g++
// (tests/ivf_range_ref.py is the same in numpy).  The probe row, the clamp of a list range, the cut of a row and the label of a
// position are the scan's (ivf_scan_ref.h, ivs::).
//
// Slot.  Entry j of query q's probe row is slot q * nprobe + j.  Its candidates are the entries of the list it names, in ascending
// offset order, if the entry is a valid list number and the first mention of that list in the row; otherwise it has none.
// Hit.  A candidate whose float32 squared distance is strictly below the radius (a NaN, zero or negative radius: none; +inf: all).
// Count.  slot_lims = the exclusive prefix sum of the hits per slot, in slot order; slot_lims[nq * nprobe] is the total.
// Fill.  The r-th hit of slot s goes to place slot_lims[s] + r; it is written only if the place is below slot_lims[s + 1] and below
// the capacity of the output arrays, so slot_lims of another radius or a short capacity give a partial result, never a stray write.
//
// Every loop is bounded by its arguments (nprobe, the clamped length of a list), never by what the arrays hold.
#pragma once
#include <stdint.h>

#include "ivf_scan_ref.h"

namespace vidc {
namespace ivr {

VIDC_HD inline uint64_t slot_of(uint64_t q, uint32_t nprobe, uint32_t j) { return q * nprobe + j; }
// the hit test: strictly below, in float32 (false for every NaN on either side)
VIDC_HD inline bool is_hit(float dist, float radius) { return dist < radius; }
// the place of a hit: the slot's base, the hits of the slot's earlier trips, the hits of this trip at earlier offsets
VIDC_HD inline uint64_t hit_place(uint64_t base, uint32_t running, uint32_t below) { return base + running + below; }
// the write-bound rule
VIDC_HD inline bool place_written(uint64_t place, uint64_t slot_end, uint64_t capacity) { return place < slot_end && place < capacity; }

// ---- the serial form of one (query, piece), from the rules above (what tests/ivf_range_test.cpp runs; the kernel does the same with
// a lane per code).  row: nprobe words of scratch; table: M * 256 floats (PQ8), or NULL.
inline float code_distance(int kind, const uint8_t *code, uint32_t d, uint32_t M, const float *xq, const float *table) {
    float dist = 0.f;
    if (kind == ivs::PQ8) {
        for (uint32_t m = 0; m < M; m++) dist += table[m * 256u + code[m]];
    } else {
        for (uint32_t i = 0; i < d; i++) {  // (byte copies: the code array need not be aligned here)
            float v;
            __builtin_memcpy(&v, code + (uint64_t)i * 4, 4);
            const float t = xq[i] - v;
            dist += t * t;
        }
    }
    return dist;
}
inline void prepare_row(uint64_t nlist, int kind, uint32_t d, uint32_t M, const float *codebooks, const float *xq, uint32_t nprobe,
                        const int64_t *probes, int32_t *row, float *table) {
    for (uint32_t j = 0; j < nprobe; j++) row[j] = ivs::probe_list(probes[j], nlist);
    for (uint32_t j = 0; j < nprobe; j++)
        if (ivs::probe_repeats(row, j)) row[j] = -1;
    if (kind == ivs::PQ8)
        for (uint32_t e = 0; e < M * 256u; e++) table[e] = ivs::pq_entry(xq, codebooks, d / M, e >> 8, e & 255u);
}

// counts: the nprobe hit counts of THIS query's slots; the piece writes every one of its own, the others are left alone
inline void count_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, int kind, uint32_t d, uint32_t M,
                         const float *codebooks, const float *xq, uint32_t nprobe, const int64_t *probes, float radius, uint32_t S,
                         uint32_t s, int32_t *row, float *table, uint32_t *counts) {
    prepare_row(nlist, kind, d, M, codebooks, xq, nprobe, probes, row, table);
    const uint64_t code_size = kind == ivs::PQ8 ? (uint64_t)M : (uint64_t)d * 4;
    for (uint32_t j = ivs::piece_begin(nprobe, S, s); j < ivs::piece_begin(nprobe, S, s + 1); j++) {
        uint32_t hits = 0;
        if (row[j] >= 0) {
            const ivs::Range r = ivs::list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
            for (uint64_t p = r.a; p < r.b; p++) hits += is_hit(code_distance(kind, codes + p * code_size, d, M, xq, table), radius) ? 1u : 0u;
        }
        counts[j] = hits;
    }
}

// lims: the nprobe + 1 slot limits of THIS query (slot_lims + q * nprobe); D / labels: the call's output arrays of `capacity` entries
inline void fill_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, int kind, uint32_t d, uint32_t M,
                        const float *codebooks, const float *xq, uint32_t nprobe, const int64_t *probes, float radius, uint32_t S,
                        uint32_t s, int32_t *row, float *table, const uint64_t *lims, uint64_t capacity, float *D, int64_t *labels) {
    prepare_row(nlist, kind, d, M, codebooks, xq, nprobe, probes, row, table);
    const uint64_t code_size = kind == ivs::PQ8 ? (uint64_t)M : (uint64_t)d * 4;
    for (uint32_t j = ivs::piece_begin(nprobe, S, s); j < ivs::piece_begin(nprobe, S, s + 1); j++) {
        if (row[j] < 0) continue;
        const ivs::Range r = ivs::list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
        uint32_t running = 0;
        for (uint64_t p0 = r.a; p0 < r.b; p0 += ivs::TRIP) {
            uint32_t below = 0;
            for (uint64_t p = p0; p < r.b && p < p0 + ivs::TRIP; p++) {
                const float dist = code_distance(kind, codes + p * code_size, d, M, xq, table);
                if (!is_hit(dist, radius)) continue;
                const uint64_t place = hit_place(lims[j], running, below++);
                if (place_written(place, lims[j + 1], capacity)) {
                    D[place] = dist;
                    labels[place] = ivs::key_label(offsets, nlist, ivs::key_make(dist, (uint32_t)p));
                }
            }
            running += below;
        }
    }
}

}  // namespace ivr
}  // namespace vidc
