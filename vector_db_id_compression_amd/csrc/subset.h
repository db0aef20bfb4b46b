// subset.h -- the predicate mark and the per-list range arithmetic shared by the vidc_*_subset_dev calls: a subset type and two
// arguments (subset_plan.h) name the entries of an existing object that a new object over the same lists takes, order kept.
//
//   types 0 and 1 (ID_RANGE, ID_MOD) look at the ids: a wavefront per chunk of RM_UNIT decoded elements (the chunk tables of
//      app_chunks) evaluates the predicate, writes the kill byte (1 - taken) the remove's compaction reads, the caller's `taken` byte
//      and the chunk's kill count (k_sub_mark_id); the exclusive scan of the kill counts, k_rm_new_off and k_rm_compact place the
//      taken entries as a remove places its survivors.
//   types 2 .. 4 (ELEMENT_RANGE, INVLIST_FRACTION, INVLIST) look at positions: one thread per list computes [i1, i2) from the offsets
//      alone (k_sub_bounds), a scan of the new sizes gives the new offsets, and a wavefront per chunk copies old_l[i1:i2] to its place
//      and writes the `taken` bytes from the bounds (k_sub_slice).  Nothing is marked.
// No atomic decides a position: the output is the same on every run.  What crosses PCIe: the size of the subset (8 bytes).  Included
// by several translation units: everything has internal linkage.
#pragma once
#include "remove.h"
#include "subset_plan.h"

namespace vidc {
namespace {

// Mark, a wavefront per chunk: segment s of `dec` (seg_off) is list seg_list[s] (NULL: list s).  kill[position in dec] = 1 - taken;
// taken_obj (optional) gets the taken byte at obj_off[l] + position in the list; chunk_kill[c] = entries of chunk c that are not taken.
__global__ void __launch_bounds__(256) k_sub_mark_id(const uint64_t *__restrict__ dec, const uint64_t *__restrict__ seg_off,
                                                     const uint32_t *__restrict__ seg_list, const Chunk *__restrict__ items,
                                                     const uint64_t *__restrict__ n_items, int type, uint64_t a1, uint64_t a2, uint32_t mod_kind,
                                                     uint8_t *__restrict__ kill, uint8_t *__restrict__ taken_obj,
                                                     const uint64_t *__restrict__ obj_off, uint32_t *__restrict__ chunk_kill) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < RM_UNIT ? n - ch.start : RM_UNIT);
        const uint64_t l = seg_list ? seg_list[ch.list] : ch.list;
        const uint64_t *s = dec + base + ch.start;
        uint8_t *k = kill + base + ch.start;
        uint8_t *t = taken_obj ? taken_obj + obj_off[l] + ch.start : nullptr;
        uint32_t kills = 0;
        for (uint32_t j0 = 0; j0 < nc; j0 += 64u) {  // (j0, nc: wavefront-uniform)
            const uint32_t j = j0 + lane;
            const bool in = j < nc;
            const bool take = in && subset_takes_id(type, a1, a2, mod_kind, s[j]);
            if (in) {
                k[j] = take ? 0 : 1;
                if (t) t[j] = take ? 1 : 0;
            }
            kills += dev::popc64(__ballot(in && !take));
        }
        if (lane == 0) chunk_kill[c] = kills;
    }
}

// Bounds, a thread per list: lo[l] = i1, sizes[l] = i2 - i1 of subset_bounds on the object's offsets (T = off[nlist] > 0); cls[l]
// (optional) = the list's ROC class and pflag[l] = 1 for a partial list, whose exclusive scan numbers the lists that are re-encoded.
__global__ void __launch_bounds__(256) k_sub_bounds(const uint64_t *__restrict__ off, uint64_t nlist, int type, uint64_t a1, uint64_t a2,
                                                    uint32_t *__restrict__ lo, uint32_t *__restrict__ sizes, uint32_t *__restrict__ cls,
                                                    uint32_t *__restrict__ pflag) {
    const uint64_t T = off[nlist];
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o0 = off[l], o1 = off[l + 1];
        uint64_t i1, i2;
        subset_bounds(type, a1, a2, T, l, o0, o1, i1, i2);
        lo[l] = (uint32_t)i1;
        sizes[l] = (uint32_t)(i2 - i1);
        if (cls) {
            const uint32_t c = subset_roc_class(o1 - o0, i2 - i1);
            cls[l] = c;
            pflag[l] = c == SUBC_PARTIAL ? 1u : 0u;
        }
    }
}

// Slice, a wavefront per chunk: segment s (seg_off) is list l = seg_list[s] (NULL: list s); its entries lo[l] <= j < lo[l] + sizes[l]
// are the subset.  dec != NULL: they go to out + dst_off[s], order kept.  taken != NULL: taken[obj_off[l] + j] = 1 inside the range, 0
// outside, for every j of the segment.
__global__ void __launch_bounds__(256) k_sub_slice(const uint64_t *__restrict__ dec, const uint64_t *__restrict__ seg_off,
                                                   const uint32_t *__restrict__ seg_list, const uint32_t *__restrict__ lo,
                                                   const uint32_t *__restrict__ sizes, const Chunk *__restrict__ items,
                                                   const uint64_t *__restrict__ n_items, const uint64_t *__restrict__ dst_off,
                                                   uint64_t *__restrict__ out, uint8_t *__restrict__ taken, const uint64_t *__restrict__ obj_off) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < RM_UNIT ? n - ch.start : RM_UNIT);
        const uint64_t l = seg_list ? seg_list[ch.list] : ch.list;
        const uint64_t i1 = lo[l], i2 = i1 + sizes[l];
        const uint64_t *s = dec ? dec + base : nullptr;
        uint64_t *d = dec ? out + dst_off[ch.list] : nullptr;
        uint8_t *t = taken ? taken + obj_off[l] : nullptr;
        for (uint32_t j0 = lane; j0 < nc; j0 += 64u) {
            const uint64_t j = ch.start + j0;  // position in the list: j < n
            const bool take = i1 <= j && j < i2;
            if (take && d) d[j - i1] = s[j];
            if (t) t[j] = take ? 1 : 0;
        }
    }
}

// the host-side argument checks every subset makes before any device work; *out = NULL from here on
template <typename Obj>
inline int subset_check(const char *what, const ::vidc_ctx *ctx, const Obj *obj, Obj **out, int type, uint64_t a1, uint64_t a2) {
    if (out) *out = nullptr;
    const bool any_null = !ctx || !obj || !out;
    switch (subset_refusal(any_null, type, a1, a2, any_null ? 0 : obj->ntotal)) {  // (the object is read for its ntotal alone)
    case SUB_OK: return VIDC_OK;
    case SUB_NULL: set_error("%s subset: NULL context, object or out", what); break;
    case SUB_TYPE: set_error("%s subset: subset_type %d outside 0 .. 4", what, type); break;
    default:
        set_error("%s subset: type %d does not take a1 = %llu, a2 = %llu (1: a2 < a1; 2: a1 <= a2 <= ntotal; 3: a2 < a1 < 2^32)", what, type,
                  (unsigned long long)a1, (unsigned long long)a2);
    }
    return VIDC_ERR_INVALID;
}

// The id mark on a decoded CSR: nseg segments (d_seg_off, `total` > 0 elements in d_dec; segment s is list d_seg_list[s], NULL: list
// s).  d_kill: total bytes, every one written.  Afterwards m.new_off (nseg + 1, device) are the offsets of the taken entries and
// m.ks / the chunk table are what remove_compact places them by.  Enqueue only.
inline int subset_mark(::vidc_ctx *ctx, int type, uint64_t a1, uint64_t a2, const uint64_t *d_dec, const uint64_t *d_seg_off,
                       const uint32_t *d_seg_list, uint64_t nseg, uint64_t total, uint8_t *d_kill, uint8_t *d_taken_obj, const uint64_t *d_obj_off,
                       RemoveMarked &m) {
    VIDC_TRY(app_chunks(ctx, d_seg_off, nseg, total, m.ch));
    const uint64_t nk = m.ch.bound + 1;  // (entries behind the last chunk stay zero: the scan runs over the bound)
    VIDC_TRY(m.s_kill.get(ctx, nk * 4));
    VIDC_TRY(m.s_ks.get(ctx, (nk + 1) * 8));
    VIDC_TRY(m.s_new.get(ctx, (nseg + 1) * 8));
    m.ks = m.s_ks.as<uint64_t>();
    m.new_off = m.s_new.as<uint64_t>();
    VIDC_HIP(hipMemsetAsync(m.s_kill.p, 0, nk * 4, ctx->stream));
    hipLaunchKernelGGL(k_sub_mark_id, app_chunk_grid(ctx, m.ch.bound), dim3(256), 0, ctx->stream, d_dec, d_seg_off, d_seg_list, m.ch.items,
                       m.ch.n_items, type, a1, a2, subset_mod_kind(type == SUB_ID_MOD ? a1 : 1), d_kill, d_taken_obj, d_obj_off,
                       m.s_kill.as<uint32_t>());
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(device_exscan(ctx, m.s_kill.as<uint32_t>(), (uint32_t)nk, m.s_ks.as<uint64_t>(), m.s_tmp));
    hipLaunchKernelGGL(k_rm_new_off, req_grid(ctx, nseg + 1), dim3(256), 0, ctx->stream, d_seg_off, nseg, (const uint64_t *)m.ch.s_off.as<uint64_t>(),
                       m.ks, m.new_off);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// Subset by rebuild (packed bits, Elias-Fano): the object is decoded into scratch and marked and compacted (types 0, 1) or sliced
// (types 2 .. 4); the caller hands (new_off, ntotal_new, s_out) to the codec's own device-offsets encoder.  decode_all(d_out).  Ends
// with the call's read-back of the subset's size: synchronises.  kernel_ms: the kernels so far (the decode included).
struct SubsetRebuilt {
    RemoveMarked marked;
    AppChunks ch;
    Scratch s_old, s_out, s_kill, s_new, s_lo, s_tmp;
    Pinned h_back;
    uint64_t ntotal_new = 0;
    uint64_t *new_off = nullptr;
    double kernel_ms = 0;
};
template <typename DecodeAll>
inline int subset_rebuild(::vidc_ctx *ctx, uint64_t nlist, uint64_t ntotal_old, const uint64_t *d_old_off, int type, uint64_t a1, uint64_t a2,
                          uint8_t *d_taken, SubsetRebuilt &m, DecodeAll &&decode_all) {
    VIDC_TRY(m.h_back.get(ctx, 64));
    if (!ntotal_old) {  // nothing to decode: every list stays empty
        VIDC_TRY(m.s_new.get(ctx, (nlist + 1) * 8));
        VIDC_TRY(m.s_out.get(ctx, 8));
        m.new_off = m.s_new.as<uint64_t>();
        VIDC_HIP(hipMemsetAsync(m.new_off, 0, (nlist + 1) * 8, ctx->stream));
        VIDC_HIP(vidc_stream_wait(ctx->stream));
        m.ntotal_new = 0;
        return VIDC_OK;
    }
    VIDC_TRY(m.s_old.get(ctx, ntotal_old * 8));
    VIDC_TRY(m.s_out.get(ctx, ntotal_old * 8));
    VIDC_TRY(decode_all(m.s_old.as<uint64_t>()));
    m.kernel_ms = ctx->last_kernel_ms;
    EventTimer tm = EventTimer::started(ctx);
    if (subset_by_id(type)) {
        VIDC_TRY(m.s_kill.get(ctx, ntotal_old));
        VIDC_TRY(subset_mark(ctx, type, a1, a2, m.s_old.as<uint64_t>(), d_old_off, nullptr, nlist, ntotal_old, m.s_kill.as<uint8_t>(), d_taken, d_old_off,
                             m.marked));
        m.new_off = m.marked.new_off;
        VIDC_TRY(remove_compact(ctx, m.marked, m.s_old.as<uint64_t>(), d_old_off, m.s_kill.as<uint8_t>(), m.new_off, nullptr, m.s_out.as<uint64_t>()));
    } else {
        VIDC_TRY(m.s_lo.get(ctx, 2 * (nlist + 1) * 4));  // lo | sizes
        VIDC_TRY(m.s_new.get(ctx, (nlist + 1) * 8));
        uint32_t *lo = m.s_lo.as<uint32_t>(), *sizes = lo + nlist + 1;
        m.new_off = m.s_new.as<uint64_t>();
        hipLaunchKernelGGL(k_sub_bounds, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, d_old_off, nlist, type, a1, a2, lo, sizes, (uint32_t *)nullptr,
                           (uint32_t *)nullptr);
        VIDC_HIP(hipGetLastError());
        VIDC_TRY(device_exscan(ctx, sizes, (uint32_t)nlist, m.new_off, m.s_tmp));
        VIDC_TRY(app_chunks(ctx, d_old_off, nlist, ntotal_old, m.ch));
        hipLaunchKernelGGL(k_sub_slice, app_chunk_grid(ctx, m.ch.bound), dim3(256), 0, ctx->stream, (const uint64_t *)m.s_old.as<uint64_t>(), d_old_off,
                           (const uint32_t *)nullptr, (const uint32_t *)lo, (const uint32_t *)sizes, m.ch.items, m.ch.n_items,
                           (const uint64_t *)m.new_off, m.s_out.as<uint64_t>(), d_taken, d_old_off);
        VIDC_HIP(hipGetLastError());
    }
    (void)tm.mark();
    uint64_t *h = m.h_back.as<uint64_t>();
    VIDC_HIP(hipMemcpyAsync(h, m.new_off + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    m.kernel_ms += tm.elapsed();
    m.ntotal_new = h[0];
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
