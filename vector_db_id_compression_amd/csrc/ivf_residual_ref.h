// ivf_residual_ref.h -- the serial statement of the residual-PQ IVF scan and range search (vidc_ivf_scan_residual_dev,
// vidc_ivf_range_count_residual_dev / vidc_ivf_range_fill_residual_dev), host + device, no HIP runtime: the kernels of ivf_residual.hip
// call the rules below and tests/ivf_residual_test.cpp builds them with g++ (tests/ivf_residual_ref.py is the same in numpy).
//
// A code of list l is the 8-bit PQ code of (vector - centroids[l]).  For a query xq and a valid list l:
//   r           = xq - centroids[l]                            one float32 subtraction per component
//   entry(m, c) = ivs::pq_entry(r, codebooks, dsub, m, c)      components in order
//   distance    = sum over m of entry(m, code[m])              in m order
// so the table belongs to (query, list), not to the query: it is built in front of every probed list whose clamped range is not
// empty.  Everything else -- the probe row, the clamp, the key, the insert by rank, the cut and its merge, the label, the slot, the
// hit, the place and the write bound -- is ivf_scan_ref.h / ivf_range_ref.h, unchanged.
#pragma once
#include <stdint.h>

#include "ivf_range_ref.h"
#include "ivf_scan_ref.h"

namespace vidc {
namespace ivx {

// the residual of a query against a list's centroid; r: d floats
VIDC_HD inline void residual(const float *xq, const float *centroid, uint32_t d, float *r) {
    for (uint32_t i = 0; i < d; i++) r[i] = xq[i] - centroid[i];
}
// the table of (query, list); r: d floats of scratch, table: M * 256 floats
inline void list_table(const float *xq, const float *centroids, uint32_t l, uint32_t d, uint32_t M, const float *codebooks, float *r,
                       float *table) {
    residual(xq, centroids + (uint64_t)l * d, d, r);
    for (uint32_t e = 0; e < M * 256u; e++) table[e] = ivs::pq_entry(r, codebooks, d / M, e >> 8, e & 255u);
}
inline void prepare_row(uint64_t nlist, uint32_t nprobe, const int64_t *probes, int32_t *row) {
    for (uint32_t j = 0; j < nprobe; j++) row[j] = ivs::probe_list(probes[j], nlist);
    for (uint32_t j = 0; j < nprobe; j++)
        if (ivs::probe_repeats(row, j)) row[j] = -1;
}

// ---- the serial scan of one (query, piece).  row: nprobe words of scratch; r: d floats; table: M * 256 floats; pool / tmp: k words
// each; cand: TRIP words.  -> pool holds the k best keys of the piece, EMPTY padded; ivs::merge_serial joins the pieces.
inline void scan_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, uint32_t d, uint32_t M,
                        const float *codebooks, const float *centroids, const float *xq, uint32_t nprobe, const int64_t *probes, uint32_t k,
                        uint32_t S, uint32_t s, int32_t *row, float *r, float *table, uint64_t *pool, uint64_t *tmp, uint64_t *cand,
                        ivs::Stats *st) {
    prepare_row(nlist, nprobe, probes, row);
    for (uint32_t i = 0; i < k; i++) pool[i] = ivs::EMPTY;
    st->lists = st->codes = 0;
    for (uint32_t j = ivs::piece_begin(nprobe, S, s); j < ivs::piece_begin(nprobe, S, s + 1); j++) {
        if (row[j] < 0) continue;
        const ivs::Range g = ivs::list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
        st->lists++;
        st->codes += (uint32_t)(g.b - g.a);
        if (g.a < g.b) list_table(xq, centroids, (uint32_t)row[j], d, M, codebooks, r, table);  // (an empty list builds nothing)
        for (uint64_t p0 = g.a; p0 < g.b; p0 += ivs::TRIP) {
            uint32_t C = 0;
            for (uint64_t p = p0; p < g.b && p < p0 + ivs::TRIP; p++) {
                const uint64_t key = ivs::key_make(ivr::code_distance(ivs::PQ8, codes + p * M, d, M, xq, table), (uint32_t)p);
                if (!ivs::key_dropped(key, pool[k - 1])) cand[C++] = key;
            }
            if (C) ivs::insert_trip(pool, tmp, k, cand, C);
        }
    }
}

// ---- the serial range count / fill of one (query, piece): the slots, hits and places of ivf_range_ref.h over the per-list table.
// counts: the nprobe hit counts of THIS query's slots; the piece writes every one of its own, the others are left alone
inline void count_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, uint32_t d, uint32_t M,
                         const float *codebooks, const float *centroids, const float *xq, uint32_t nprobe, const int64_t *probes,
                         float radius, uint32_t S, uint32_t s, int32_t *row, float *r, float *table, uint32_t *counts) {
    prepare_row(nlist, nprobe, probes, row);
    for (uint32_t j = ivs::piece_begin(nprobe, S, s); j < ivs::piece_begin(nprobe, S, s + 1); j++) {
        uint32_t hits = 0;
        if (row[j] >= 0) {
            const ivs::Range g = ivs::list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
            if (g.a < g.b) list_table(xq, centroids, (uint32_t)row[j], d, M, codebooks, r, table);
            for (uint64_t p = g.a; p < g.b; p++)
                hits += ivr::is_hit(ivr::code_distance(ivs::PQ8, codes + p * M, d, M, xq, table), radius) ? 1u : 0u;
        }
        counts[j] = hits;
    }
}

// lims: the nprobe + 1 slot limits of THIS query (slot_lims + q * nprobe); D / labels: the call's output arrays of `capacity` entries
inline void fill_serial(uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint8_t *codes, uint32_t d, uint32_t M,
                        const float *codebooks, const float *centroids, const float *xq, uint32_t nprobe, const int64_t *probes,
                        float radius, uint32_t S, uint32_t s, int32_t *row, float *r, float *table, const uint64_t *lims, uint64_t capacity,
                        float *D, int64_t *labels) {
    prepare_row(nlist, nprobe, probes, row);
    for (uint32_t j = ivs::piece_begin(nprobe, S, s); j < ivs::piece_begin(nprobe, S, s + 1); j++) {
        if (row[j] < 0) continue;
        const ivs::Range g = ivs::list_range(offsets[row[j]], offsets[(uint64_t)row[j] + 1], ntotal);
        if (g.a < g.b) list_table(xq, centroids, (uint32_t)row[j], d, M, codebooks, r, table);
        uint32_t running = 0;
        for (uint64_t p0 = g.a; p0 < g.b; p0 += ivs::TRIP) {
            uint32_t below = 0;
            for (uint64_t p = p0; p < g.b && p < p0 + ivs::TRIP; p++) {
                const float dist = ivr::code_distance(ivs::PQ8, codes + p * M, d, M, xq, table);
                if (!ivr::is_hit(dist, radius)) continue;
                const uint64_t place = ivr::hit_place(lims[j], running, below++);
                if (ivr::place_written(place, lims[j + 1], capacity)) {
                    D[place] = dist;
                    labels[place] = ivs::key_label(offsets, nlist, ivs::key_make(dist, (uint32_t)p));
                }
            }
            running += below;
        }
    }
}

}  // namespace ivx
}  // namespace vidc
