// merge.h -- what the vidc_*_merge_dev calls share: two objects over the same lists become one, list l of `b` behind list l of `a`
// with add_id added on the way (Faiss's InvertedLists::merge_from).  No sort: both sides are grouped by list already.
//
//   1. offsets: new_off[l] = a_off[l] + b_off[l], and split[l] = new_off[l] + |a_l|, where b's part of list l starts.
//   2. placement: two segmented copies of the decoded lists into the merged CSR, a wavefront per chunk of APP_COPY_UNIT elements through
//      the append's chunk table (app_chunks): a's lists by k_app_copy, b's by k_mrg_copy_add -- app_copy_chunk's body with a 64-bit add,
//      16-byte accesses where source and destination share their alignment.  The same kernel reduces the largest id of b (before the
//      shift), which the domain checks read back: 8 bytes, the only read-back of a rebuild.
//   3. d_src: for every position of the new object's decode_all order, where the entry came from: p >= 0 = position p of a's
//      decode_all order, ~p = position p of b's.  Input-order containers: arithmetic on the three offset arrays (k_mrg_src_plain);
//      re-ordering containers: through the new object's permutation (k_mrg_src_perm).
//   4. ROC: the lists are classified on the device (merge_plan.h), the re-encoded ones compacted (k_mrg_roc_classify, a scan,
//      k_mrg_roc_touched).
// Included by several translation units: everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "append.h"
#include "host_call.h"
#include "merge_plan.h"

namespace vidc {
namespace {

// new_off[l] = a_off[l] + b_off[l] for l = 0 .. nlist; split[l] = where b's part of the merged list l starts, for l < nlist
__global__ void __launch_bounds__(256) k_mrg_offsets(const uint64_t *__restrict__ a_off, const uint64_t *__restrict__ b_off, uint64_t nlist,
                                                     uint64_t *__restrict__ new_off, uint64_t *__restrict__ split) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        new_off[l] = a_off[l] + b_off[l];
        if (l < nlist) split[l] = a_off[l + 1] + b_off[l];
    }
}

__device__ __forceinline__ uint64_t mrg_wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor((unsigned long long)v, o, 64);
        v = v > w ? v : w;
    }
    return v;
}

// One chunk of a segmented copy with a shift, by one wavefront: d[j] = s[j] + add for j < nc, nc <= APP_COPY_UNIT.  app_copy_chunk's
// shape: two elements per 16-byte access where the two runs share their alignment mod 16, behind a head and in front of a tail of at
// most one element each; single elements otherwise.  -> this lane's largest s[j] (0 if it read none)
__device__ __forceinline__ uint64_t mrg_copy_add_chunk(const uint64_t *__restrict__ s, uint64_t *__restrict__ d, uint32_t nc, uint32_t lane,
                                                       uint64_t add) {
    uint64_t mx = 0;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0u) {
        uint32_t head = (uint32_t)(((16u - ((uintptr_t)d & 15u)) & 15u) / 8u);
        head = head < nc ? head : nc;
        if (lane < head) {
            const uint64_t x = s[lane];
            mx = x;
            d[lane] = x + add;
        }
        const uint32_t nv = (nc - head) / 2u;
        const ulonglong2 *sv = (const ulonglong2 *)(s + head);
        ulonglong2 *dv = (ulonglong2 *)(d + head);
        for (uint32_t j = lane; j < nv; j += 64u) {
            ulonglong2 x = sv[j];
            mx = mx > x.x ? mx : x.x;
            mx = mx > x.y ? mx : x.y;
            x.x += add;
            x.y += add;
            dv[j] = x;
        }
        for (uint32_t j = head + nv * 2u + lane; j < nc; j += 64u) {
            const uint64_t x = s[j];
            mx = mx > x ? mx : x;
            d[j] = x + add;
        }
    } else {
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t x = s[j];
            mx = mx > x ? mx : x;
            d[j] = x + add;
        }
    }
    return mx;
}

// Segment s (length src_off[s + 1] - src_off[s], at src + src_off[s]) goes to dst + dst_start[s] with `add` added to every element.
// items: the chunk table of src_off.  *max_src (zeroed by the caller) = the largest source element: a maximum does not depend on
// the order of its operands.
__global__ void __launch_bounds__(256) k_mrg_copy_add(const uint64_t *__restrict__ src, const uint64_t *__restrict__ src_off,
                                                      const uint64_t *__restrict__ dst_start, uint64_t *__restrict__ dst, uint64_t add,
                                                      const Chunk *__restrict__ items, const uint64_t *__restrict__ n_items,
                                                      unsigned long long *max_src) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    uint64_t mx = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = src_off[ch.list], n = src_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        const uint64_t m = mrg_copy_add_chunk(src + base + ch.start, dst + dst_start[ch.list] + ch.start, nc, lane, add);
        mx = mx > m ? mx : m;
    }
    mx = mrg_wave_max_u64(mx);  // (the loop above is wavefront-uniform: every lane is here)
    if (lane == 0 && mx) atomicMax(max_src, (unsigned long long)mx);
}

// d_src of a container that keeps input order.  items: the chunk table of new_off.
__global__ void __launch_bounds__(256) k_mrg_src_plain(const uint64_t *__restrict__ a_off, const uint64_t *__restrict__ b_off,
                                                       const uint64_t *__restrict__ new_off, const Chunk *__restrict__ items,
                                                       const uint64_t *__restrict__ n_items, int64_t *__restrict__ d_src) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t l = ch.list, base = new_off[l], n = new_off[l + 1] - base, a0 = a_off[l], a_n = a_off[l + 1] - a0, b0 = b_off[l];
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t q = ch.start + j;
            d_src[base + q] = q < a_n ? (int64_t)(a0 + q) : ~(int64_t)(b0 + q - a_n);
        }
    }
}

// d_src of a container that re-orders a list, from the permutation over the positions of M_l: the permutation of list l is at
// perm + perm_off[l] (pslot == NULL: the new object's own), or at perm + perm_off[pslot[l] - 1], or the identity where pslot[l] == 0
// (the ROC splice: only the re-encoded lists have one).  items: the chunk table of new_off.
__global__ void __launch_bounds__(256) k_mrg_src_perm(const uint32_t *__restrict__ perm, const uint64_t *__restrict__ perm_off,
                                                      const uint32_t *__restrict__ pslot, const uint64_t *__restrict__ a_off,
                                                      const uint64_t *__restrict__ b_off, const uint64_t *__restrict__ new_off,
                                                      const Chunk *__restrict__ items, const uint64_t *__restrict__ n_items,
                                                      int64_t *__restrict__ d_src) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t l = ch.list, base = new_off[l], n = new_off[l + 1] - base, a0 = a_off[l], a_n = a_off[l + 1] - a0, b0 = b_off[l];
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        const uint32_t sl = pslot ? pslot[l] : (uint32_t)l + 1u;
        const uint32_t *p = sl ? perm + perm_off[sl - 1u] + ch.start : nullptr;
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t q = ch.start + j, in_pos = p ? (uint64_t)p[j] : q;
            d_src[base + q] = in_pos < a_n ? (int64_t)(a0 + in_pos) : ~(int64_t)(b0 + in_pos - a_n);
        }
    }
}

// ROC: cls[l] = merge_roc_class; for a list that is re-encoded flag[l] = 1, mark[l] = its merged size and bmark[l] = |b_l| (what the
// scans turn into its place in the staging CSR of the merged lists and in the staging of b's decoded lists), 0 otherwise
__global__ void __launch_bounds__(256) k_mrg_roc_classify(const uint64_t *__restrict__ a_off, const uint64_t *__restrict__ b_off, uint64_t nlist,
                                                          bool shifted, uint32_t *__restrict__ cls, uint32_t *__restrict__ flag,
                                                          uint32_t *__restrict__ mark, uint32_t *__restrict__ bmark) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a_n = a_off[l + 1] - a_off[l], b_n = b_off[l + 1] - b_off[l];
        const uint32_t c = merge_roc_class(a_n, b_n, shifted);
        const bool enc = c == MRG_ENCODE;
        cls[l] = c;
        flag[l] = enc ? 1u : 0u;
        mark[l] = enc ? (uint32_t)(a_n + b_n) : 0u;  // (ntotal(a) + ntotal(b) < 2^32 - 1: checked by the caller)
        bmark[l] = enc ? (uint32_t)b_n : 0u;
    }
}
// touched[tpos[l]] = l and msize[tpos[l]] = merged size for every re-encoded list, ascending; for every list slot[l] = tpos[l] + 1 or
// 0 (what the permutation kernels select by) and dst_start[l] = where b's part of the list starts in the staging CSR
__global__ void __launch_bounds__(256) k_mrg_roc_touched(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ tpos,
                                                         const uint32_t *__restrict__ mark, const uint64_t *__restrict__ stage_off,
                                                         const uint64_t *__restrict__ a_off, uint64_t nlist, uint32_t *__restrict__ touched,
                                                         uint32_t *__restrict__ msize, uint32_t *__restrict__ slot,
                                                         uint64_t *__restrict__ dst_start) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const bool t = flag[l] != 0u;
        slot[l] = t ? (uint32_t)tpos[l] + 1u : 0u;
        dst_start[l] = stage_off[l] + (a_off[l + 1] - a_off[l]);
        if (t) {
            touched[tpos[l]] = (uint32_t)l;
            msize[tpos[l]] = mark[l];
        }
    }
}

// the host-side argument checks every merge makes before any device work; *out = NULL from here on.  Obj: nlist, ntotal, device.
template <typename Obj>
inline int merge_check(const ::vidc_ctx *ctx, const Obj *a, const Obj *b, Obj **out) {
    if (out) *out = nullptr;
    const bool any_null = !ctx || !a || !b || !out;
    switch (merge_refusal(any_null, any_null ? 0 : a->nlist, any_null ? 0 : b->nlist, any_null ? 0 : ctx->device, any_null ? 0 : a->device,
                          any_null ? 0 : b->device, any_null ? 0 : a->ntotal, any_null ? 0 : b->ntotal)) {
        case MRG_OK: return VIDC_OK;
        case MRG_NULL: set_error("merge: NULL context, object or out"); break;
        case MRG_NLIST:
            set_error("merge: the objects hold %llu and %llu lists", (unsigned long long)a->nlist, (unsigned long long)b->nlist);
            break;
        case MRG_DEVICE:
            set_error("merge: the objects live on devices %d and %d, the context on device %d", a->device, b->device, ctx->device);
            break;
        case MRG_NTOTAL: set_error("merge: the merged object would hold 2^32 - 1 ids or more"); break;
    }
    return VIDC_ERR_INVALID;
}

// Merge by rebuild (packed bits, Elias-Fano, wavelet tree): both objects are decoded into scratch (once when they are the same
// object), placed (steps 1-2 of the header) and handed to the codec's own device-offsets encoder by the caller.  dec_a(d_out),
// dec_b(d_out): the objects' decode_all.  Synchronises; max_b = the largest id of b before the shift (0 without ids).
struct MergeRebuilt {
    Scratch s_a, s_b, s_merged, s_off, s_max;
    Pinned h_back;
    uint64_t ntotal_new = 0, max_b = 0;
    const uint64_t *new_off = nullptr, *split = nullptr;
    double kernel_ms = 0;
};
template <typename DecA, typename DecB>
inline int merge_rebuild(::vidc_ctx *ctx, uint64_t nlist, uint64_t na, uint64_t nb, const uint64_t *d_a_off, const uint64_t *d_b_off,
                         uint64_t add_id, bool same, MergeRebuilt &m, DecA &&dec_a, DecB &&dec_b) {
    m.ntotal_new = na + nb;
    VIDC_TRY(m.s_merged.get(ctx, (m.ntotal_new ? m.ntotal_new : 1) * 8));
    VIDC_TRY(m.s_off.get(ctx, 2 * (nlist + 1) * 8));
    VIDC_TRY(m.s_max.get(ctx, 8));
    VIDC_TRY(m.h_back.get(ctx, 64));
    uint64_t *new_off = m.s_off.as<uint64_t>(), *split = new_off + nlist + 1;
    m.new_off = new_off;
    m.split = split;
    const uint64_t *ids_b = nullptr;
    if (na) {
        VIDC_TRY(m.s_a.get(ctx, na * 8));
        VIDC_TRY(dec_a(m.s_a.as<uint64_t>()));
        m.kernel_ms += ctx->last_kernel_ms;
    }
    if (nb && same) ids_b = m.s_a.as<uint64_t>();
    else if (nb) {
        VIDC_TRY(m.s_b.get(ctx, nb * 8));
        VIDC_TRY(dec_b(m.s_b.as<uint64_t>()));
        m.kernel_ms += ctx->last_kernel_ms;
        ids_b = m.s_b.as<uint64_t>();
    }
    AppChunks ch_a, ch_b;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    hipLaunchKernelGGL(k_mrg_offsets, req_grid(ctx, nlist + 1), dim3(256), 0, ctx->stream, d_a_off, d_b_off, nlist, new_off, split);
    VIDC_HIP(hipGetLastError());
    if (na) {
        VIDC_TRY(app_chunks(ctx, d_a_off, nlist, na, ch_a));
        hipLaunchKernelGGL(k_app_copy<uint64_t>, app_chunk_grid(ctx, ch_a.bound), dim3(256), 0, ctx->stream,
                           (const uint64_t *)m.s_a.as<uint64_t>(), d_a_off, (const uint64_t *)nullptr, (const uint64_t *)nullptr,
                           (const uint32_t *)nullptr, (const uint64_t *)new_off, m.s_merged.as<uint64_t>(), ch_a.items, ch_a.n_items);
        VIDC_HIP(hipGetLastError());
    }
    uint64_t *h = m.h_back.as<uint64_t>();
    h[0] = 0;
    if (nb) {
        VIDC_HIP(hipMemsetAsync(m.s_max.p, 0, 8, ctx->stream));
        VIDC_TRY(app_chunks(ctx, d_b_off, nlist, nb, ch_b));
        hipLaunchKernelGGL(k_mrg_copy_add, app_chunk_grid(ctx, ch_b.bound), dim3(256), 0, ctx->stream, ids_b, d_b_off, (const uint64_t *)split,
                           m.s_merged.as<uint64_t>(), add_id, ch_b.items, ch_b.n_items, m.s_max.as<unsigned long long>());
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(hipMemcpyAsync(h, m.s_max.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    VIDC_HIP(t.mark());
    guard.disarm();
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    m.kernel_ms += t.elapsed();
    m.max_b = h[0];
    return VIDC_OK;
}

// d_src (step 3 of the header) over the new object's offsets; perm == NULL: the input-order form.  Synchronises.
inline int merge_write_src(::vidc_ctx *ctx, uint64_t nlist, uint64_t ntotal_new, const uint64_t *d_a_off, const uint64_t *d_b_off,
                           const uint64_t *d_new_off, const uint32_t *d_perm, const uint64_t *d_perm_off, const uint32_t *d_pslot,
                           int64_t *d_src, double &kernel_ms) {
    if (!d_src || !ntotal_new) return VIDC_OK;
    AppChunks ch;
    StreamGuard guard(ctx);
    VIDC_TRY(app_chunks(ctx, d_new_off, nlist, ntotal_new, ch));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    if (d_perm)
        hipLaunchKernelGGL(k_mrg_src_perm, app_chunk_grid(ctx, ch.bound), dim3(256), 0, ctx->stream, d_perm, d_perm_off, d_pslot, d_a_off, d_b_off,
                           d_new_off, ch.items, ch.n_items, d_src);
    else
        hipLaunchKernelGGL(k_mrg_src_plain, app_chunk_grid(ctx, ch.bound), dim3(256), 0, ctx->stream, d_a_off, d_b_off, d_new_off, ch.items,
                           ch.n_items, d_src);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(t.mark());
    guard.disarm();
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    kernel_ms += t.elapsed();
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
