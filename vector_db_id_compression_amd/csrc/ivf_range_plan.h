// ivf_range_plan.h -- what the host decides for vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev before any device work: the
// argument checks, the LDS of one wavefront, the resident wavefronts, the cut S of a probe row, the scratch, and the (G, V, W) of the
// distance trip.  Host only, no HIP runtime: ivf_range.hip includes it and tests/ivf_range_test.cpp builds it with g++.  The count
// and the fill of one search make the same plan from the same arguments: both passes then see bit-identical distances.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_range_ref.h"
#include "ivf_scan_plan.h"

namespace vidc {
namespace ivr {

// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work).  The limits are the scan's, k apart (there is
// none), and one more: nq * nprobe + 1 slot limits are scanned with 32-bit indexes.
struct Args {
    uint64_t nlist;
    const void *offsets;
    uint64_t ntotal;
    const void *codes;
    int kind;
    uint32_t d, M;
    const void *codebooks;
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
    const void *slot_lims;
};
inline const char *check_common(const Args &a) {
    const ivs::Args s = {a.nlist, a.offsets, a.ntotal, a.codes, a.kind, a.d, a.M, a.codebooks, a.nq, a.xq, a.nprobe, a.probes, 1, &a, &a};
    if (const char *msg = ivs::check_args(s)) return msg;
    if (a.nq >= (0xffffffffull + a.nprobe - 1) / a.nprobe) return "nq * nprobe must be below 2^32 - 1";
    if (a.nq && !a.slot_lims) return "NULL slot limits";
    return nullptr;
}
inline const char *check_count(const Args &a) { return check_common(a); }
inline const char *check_fill(const Args &a, uint64_t capacity, const void *D, const void *labels) {
    if (const char *msg = check_common(a)) return msg;
    if (capacity && (!D || !labels)) return "NULL distance or label array with capacity > 0";
    return nullptr;
}

// dynamic LDS of a range wavefront: no pools.  FLAT: the trip's distances, the probe row, the query vector.  PQ8: the query vector
// (read while the table is built), the probe row, the M x 256 table.  Every part is a multiple of 16 bytes.
inline size_t head_bytes(int kind, uint32_t d) { return kind == ivs::PQ8 ? ivs::round16((size_t)d * 4) : (size_t)ivs::TRIP * 4; }
inline size_t row_bytes(uint32_t nprobe) { return ivs::round16((size_t)nprobe * 4); }
inline size_t lds_bytes(int kind, uint32_t nprobe, uint32_t d, uint32_t M) {
    const size_t behind = kind == ivs::PQ8 ? (size_t)M * 256 * 4 : ivs::round16((size_t)d * 4);
    return head_bytes(kind, d) + row_bytes(nprobe) + behind;
}
// (PQ8 at the limits: 8192 + 4096 + 65536 = 77824 bytes, two wavefronts per compute unit; M = 16, d = 128, nprobe = 16:
// 512 + 64 + 16384 = 16960 bytes, nine; FLAT d = 32, nprobe = 16: 256 + 64 + 128 = 448 bytes)

// context scratch: the nq * nprobe uint32 hit counts (every one is written by exactly one wavefront: no memset), and the tile sums
// of device_exscan beyond 8192 slots.  Nothing grows with the number of results.
inline uint64_t count_bytes(uint64_t nq, uint32_t nprobe) { return nq * nprobe * 4; }

struct Plan {
    size_t lds;
    uint32_t resident, S, nslots, W;
    uint64_t items, nslot_lims;
    gs::Group grp;  // FLAT: G lanes per vector, V components per load
};
inline Plan make_plan(uint32_t num_cu, int kind, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uintptr_t codes, uintptr_t xq) {
    Plan p;
    p.lds = lds_bytes(kind, nprobe, d, M);
    p.resident = ivs::resident_slots(num_cu, p.lds);
    p.S = ivs::pieces(nq, nprobe, p.resident);  // the scan's cut: pieces own disjoint slots, so nothing is merged
    p.items = nq * p.S;
    p.nslots = ivs::slots(p.items, p.resident);
    p.nslot_lims = nq * nprobe + 1;
    p.W = kind == ivs::PQ8 ? ivs::code_load_bytes(M, codes) : 0;
    p.grp = gs::group(d, ((codes | xq) & 15u) == 0);
    return p;
}

}  // namespace ivr
}  // namespace vidc
