// rows_update.h -- what the three vidc_*_update_rows_dev calls share (include/vidc.h, "update rows"): the argument checks, the slot
// table, and the host-side statement of which row of the updated matrix R' comes from where.  Included by several translation units:
// everything here has internal linkage.
//
// R' has N_new rows.  slot[v] = 1 + the LARGEST batch index i with d_nodes[i] == v (the last mention wins: the maximum does not depend
// on the order in which the atomics land, so the result is the same on every run); 0 = no mention.  Row v of R' is
//     slot[v] != 0              batch row slot[v] - 1
//     slot[v] == 0, v <  N_old  old row v
//     slot[v] == 0, v >= N_old  the empty row
// A negative node is skipped; a node >= N_new is skipped and counted.
#pragma once
#include <stdint.h>

// ---- host-side statement (plain C++: also compiled alone by tests/rows_update_plan_test.cpp)
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define VIDC_RU_HD __host__ __device__
#else
#define VIDC_RU_HD
#endif
namespace vidc {
enum RowsUpdSource : uint32_t { RU_OLD = 0, RU_BATCH = 1, RU_EMPTY = 2 };
// where row v of R' comes from, given slot[v]
VIDC_RU_HD inline RowsUpdSource rows_upd_source(uint32_t slot_v, uint64_t v, uint64_t N_old) {
    return slot_v ? RU_BATCH : (v < N_old ? RU_OLD : RU_EMPTY);
}
// the slot table of a batch, as the kernel builds it (reference for the stand-alone test and for reading the kernel): slot has N_new
// entries; -> the number of nodes >= N_new
inline uint64_t rows_upd_slots_host(const int64_t *nodes, uint64_t m, uint64_t N_new, uint32_t *slot) {
    uint64_t invalid = 0;
    for (uint64_t v = 0; v < N_new; v++) slot[v] = 0;
    for (uint64_t i = 0; i < m; i++) {
        const int64_t v = nodes[i];
        if (v < 0) continue;
        if ((uint64_t)v >= N_new) { invalid++; continue; }
        const uint32_t s = (uint32_t)i + 1u;
        if (s > slot[v]) slot[v] = s;
    }
    return invalid;
}
// the sizes the calls accept: VIDC_OK (0) or VIDC_ERR_INVALID (-1)
inline int rows_upd_sizes_ok(uint64_t m, uint64_t N_old, uint64_t N_new) {
    return (m < 0xffffffffull && N_new >= N_old && N_new < 0xffffffffull) ? 0 : -1;
}
// words of a fixed-stride record of LWn low + HWn high words that come from a record of LWo + HWo words: word w of the new record is
// old word rows_upd_restride(w, ...), or zero when that is ~0u.  (Low words first, then high words; a record that is kept fits the new
// geometry, so the words that are dropped hold zeros.)
VIDC_RU_HD inline uint32_t rows_upd_restride(uint32_t w, uint32_t LWn, uint32_t LWo, uint32_t HWo) {
    if (w < LWn) return w < LWo ? w : ~0u;
    const uint32_t h = w - LWn;
    return h < HWo ? LWo + h : ~0u;
}
}  // namespace vidc

#ifdef __HIPCC__
#include "common.h"
#include "requests.h"
#include "wave.h"

namespace vidc {
namespace {

// slot[v] = max(slot[v], i + 1) over the batch (slot zeroed by the host); nodes >= N_new are counted as req_count_invalid does
__global__ void __launch_bounds__(256) k_rows_upd_slots(const int64_t *__restrict__ nodes, uint64_t m, uint64_t N_new, uint32_t *__restrict__ slot,
                                                        unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < m; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + dev::lane_id();
        const int64_t v = i < m ? nodes[i] : -1;
        const bool ok = v >= 0 && (uint64_t)v < N_new;
        if (ok) atomicMax(&slot[v], (uint32_t)i + 1u);
        req_count_invalid(i < m && v >= 0 && !ok, invalid);
    }
}

// the argument checks of the three calls, before any device work
template <typename Obj>
inline int rows_upd_check(const char *what, const ::vidc_ctx *ctx, const Obj *obj, Obj **out, uint64_t m, const int64_t *d_nodes,
                          const int32_t *d_rows, uint64_t N_old, uint64_t N_new) {
    if (!ctx || !obj || !out || (m && (!d_nodes || !d_rows))) {
        set_error("%s update_rows: NULL context, object, out or array", what);
        return VIDC_ERR_INVALID;
    }
    if (rows_upd_sizes_ok(m, N_old, N_new) != 0) {
        set_error("%s update_rows: m = %llu, N_new = %llu (the object holds %llu rows): m and N_new stay below 2^32 - 1, N_new >= N_old", what,
                  (unsigned long long)m, (unsigned long long)N_new, (unsigned long long)N_old);
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}

// the slot table of a call in `s_slot` (N_new entries, at least one allocated); enqueue only
inline int rows_upd_slots(::vidc_ctx *ctx, uint64_t m, const int64_t *d_nodes, uint64_t N_new, Scratch &s_slot, uint64_t *d_invalid) {
    VIDC_TRY(s_slot.get(ctx, (N_new ? N_new : 1) * 4));
    VIDC_HIP(hipMemsetAsync(s_slot.p, 0, (N_new ? N_new : 1) * 4, ctx->stream));
    if (m) {
        hipLaunchKernelGGL(k_rows_upd_slots, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, N_new, s_slot.as<uint32_t>(),
                           (unsigned long long *)d_invalid);
        VIDC_HIP(hipGetLastError());
    }
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
#endif  // __HIPCC__
