// append.h -- the merge shared by the vidc_*_append_dev calls: a batch of (list number, id) pairs, device-resident, is placed behind
// the lists of an existing object, in batch order inside every list.
//
//   1. keys: key[i] = list number of pair i, or nlist for a pair that is skipped (negative: "not assigned", uncounted; >= nlist: counted
//      in *d_invalid).
//   2. a stable LSD radix sort of (key, i) by key, 8 bits per pass, ceil(bit_width(nlist) / 8) passes.  One wavefront owns a tile of
//      APP_TILE consecutive pairs and walks it 64 pairs at a time, so the order inside a digit is the batch order: the sorted pairs of
//      list l are its batch entries in ascending i.  No atomics decide a position: the result is the same on every run.
//   3. bounds: add_off[l] = first sorted position whose key is >= l (a binary search per list): the batch entries of list l are the
//      sorted positions add_off[l] .. add_off[l + 1], and new_off[l] = old_off[l] + add_off[l] are the offsets of the merged lists --
//      the exclusive scan of |old_l| + add_cnt[l] without a second scan.
//   4. the old lists are copied to their new places by chunk (a wavefront per APP_COPY_UNIT elements, 16-byte accesses where source and
//      destination share their alignment), the batch ids are placed behind them.
// What crosses PCIe: the number of valid pairs (8 bytes).  Included by several translation units: everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunks.h"
#include "common.h"
#include "requests.h"
#include "scan.h"
#include "wave.h"

namespace vidc {
namespace {

constexpr uint32_t APP_TILE = 1024;       // pairs per wavefront of a sort pass
constexpr uint32_t APP_COPY_UNIT = 1024;  // elements per wavefront of a segmented copy

__global__ void __launch_bounds__(256) k_app_keys(const int64_t *__restrict__ list_nos, uint64_t n, uint64_t nlist, uint32_t *__restrict__ keys,
                                                  unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + dev::lane_id();
        const int64_t l = i < n ? list_nos[i] : -1;
        const bool ok = l >= 0 && (uint64_t)l < nlist;
        if (i < n) keys[i] = ok ? (uint32_t)l : (uint32_t)nlist;
        req_count_invalid(l >= 0 && !ok, invalid);
    }
}

// hist[d * ntiles + tile] = pairs of the tile whose digit is d
__global__ void __launch_bounds__(64) k_app_hist(const uint32_t *__restrict__ keys, uint32_t n, uint32_t shift, uint32_t ntiles,
                                                 uint32_t *__restrict__ hist) {
    __shared__ uint32_t cnt[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (uint32_t d = lane; d < 256u; d += 64u) cnt[d] = 0u;
        __syncthreads();
        const uint32_t base = tile * APP_TILE;
        for (uint32_t r = 0; r < APP_TILE; r += 64u) {
            const uint32_t i = base + r + lane;
            if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & 255u], 1u);
        }
        __syncthreads();
        for (uint32_t d = lane; d < 256u; d += 64u) hist[d * ntiles + tile] = cnt[d];
        __syncthreads();
    }
}

// stable scatter of one pass: a pair goes to scan[digit][tile] + (pairs of the tile in front of it with the same digit)
__global__ void __launch_bounds__(64) k_app_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint32_t shift,
                                                    uint32_t ntiles, const uint64_t *__restrict__ scan, uint32_t *__restrict__ keys_out,
                                                    uint32_t *__restrict__ vals_out) {
    __shared__ uint32_t cnt[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (uint32_t d = lane; d < 256u; d += 64u) cnt[d] = (uint32_t)scan[d * ntiles + tile];
        __syncthreads();
        const uint32_t base = tile * APP_TILE;
        for (uint32_t r = 0; r < APP_TILE && base + r < n; r += 64u) {
            const uint32_t i = base + r + lane;
            const bool in = i < n;
            const uint32_t key = in ? keys[i] : 0u;
            const uint32_t val = in ? (vals ? vals[i] : i) : 0u;
            const uint32_t d = (key >> shift) & 255u;
            uint64_t peers = __ballot(in);  // lanes of this round with the same digit
#pragma unroll
            for (uint32_t b = 0; b < 8u; b++) {
                const bool bit = (d >> b) & 1u;
                const uint64_t m = __ballot(in && bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t before = dev::mbcnt(peers);
            const uint32_t start = in ? cnt[d] : 0u;
            __syncthreads();
            if (in) {
                keys_out[start + before] = key;
                vals_out[start + before] = val;
                if (before + 1u == dev::popc64(peers)) cnt[d] = start + before + 1u;  // (the last lane of the digit)
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// add_off[l] = first sorted position with key >= l, new_off[l] = old_off[l] + add_off[l], l = 0 .. nlist
__global__ void __launch_bounds__(256) k_app_bounds(const uint32_t *__restrict__ keys, uint32_t n, const uint64_t *__restrict__ old_off, uint64_t nlist,
                                                    uint64_t *__restrict__ add_off, uint64_t *__restrict__ new_off) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)keys[mid] < l) lo = mid + 1u; else hi = mid;
        }
        add_off[l] = lo;
        new_off[l] = old_off[l] + lo;
    }
}

// the batch ids behind the old ones: sorted position p = entry (p - add_off[l]) of list l = keys[p]; dst_off[l]: where the merged
// list starts in `merged`.  labels (optional): -1 for a skipped pair and, when `plain`, list << 32 | (|old_l| + rank) for the others
// (the containers that keep input order).
__global__ void __launch_bounds__(256) k_app_place(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint64_t nlist,
                                                   const uint64_t *__restrict__ old_off, const uint64_t *__restrict__ add_off,
                                                   const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ ids, uint64_t *__restrict__ merged,
                                                   int64_t *__restrict__ labels, bool plain) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t l = keys[p];
        const uint32_t i = vals[p];
        if (l >= nlist) {
            if (labels) labels[i] = -1;
            continue;
        }
        const uint64_t at = old_off[l + 1] - old_off[l] + (p - add_off[l]);
        merged[dst_off[l] + at] = ids[i];
        if (labels && plain) labels[i] = (int64_t)((l << 32) | at);
    }
}

// chunks of APP_COPY_UNIT elements per segment (len_off: offsets whose differences are the segment lengths)
__global__ void k_app_count_chunks(const uint64_t *len_off, uint32_t nseg, uint32_t *cnt) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += gridDim.x * blockDim.x)
        cnt[s] = (uint32_t)((len_off[s + 1] - len_off[s] + APP_COPY_UNIT - 1) / APP_COPY_UNIT);
}

// Segmented copy, a wavefront per chunk: segment s (length src_off[s + 1] - src_off[s]) goes to dst + dst_off[s].  Its source is
// src + src_off[s], or -- when slot[s] != 0 -- alt + alt_off[slot[s] - 1].
template <typename T>
__global__ void __launch_bounds__(256) k_app_copy(const T *__restrict__ src, const uint64_t *__restrict__ src_off, const T *__restrict__ alt,
                                                  const uint64_t *__restrict__ alt_off, const uint32_t *__restrict__ slot,
                                                  const uint64_t *__restrict__ dst_off, T *__restrict__ dst, const Chunk *__restrict__ items,
                                                  const uint64_t *__restrict__ n_items) {
    constexpr uint32_t VEC = 16u / sizeof(T);
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t n = src_off[ch.list + 1] - src_off[ch.list];
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        const uint32_t sl = slot ? slot[ch.list] : 0u;
        const T *s = (sl ? alt + alt_off[sl - 1u] : src + src_off[ch.list]) + ch.start;
        T *d = dst + dst_off[ch.list] + ch.start;
        if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0u) {
            uint32_t head = (uint32_t)(((16u - ((uintptr_t)d & 15u)) & 15u) / sizeof(T));
            head = head < nc ? head : nc;
            if (lane < head) d[lane] = s[lane];
            const uint32_t nv = (nc - head) / VEC;
            const uint4 *sv = (const uint4 *)(s + head);
            uint4 *dv = (uint4 *)(d + head);
            for (uint32_t j = lane; j < nv; j += 64u) dv[j] = sv[j];
            for (uint32_t j = head + nv * VEC + lane; j < nc; j += 64u) d[j] = s[j];
        } else {
            for (uint32_t j = lane; j < nc; j += 64u) d[j] = s[j];
        }
    }
}

// One chunk of a segmented copy, by one wavefront: d[0 .. nc) = s[0 .. nc), nc <= APP_COPY_UNIT.  16-byte accesses where the two runs
// share their alignment mod 16, behind a head of less than 16 bytes and in front of a tail of less than 16; accesses of one element
// otherwise.  k_app_copy's chunk body as a function, for the kernels that choose a segment's source differently (the ROC splice's word
// copy, roc.hip).  k_app_copy keeps its own text: moving it here re-allocates the registers of its 8-byte instantiation, and the code
// objects of the append and the remove stay what they were, instruction for instruction.
template <typename T>
__device__ __forceinline__ void app_copy_chunk(const T *__restrict__ s, T *__restrict__ d, uint32_t nc, uint32_t lane) {
    constexpr uint32_t VEC = 16u / sizeof(T);
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0u) {
        uint32_t head = (uint32_t)(((16u - ((uintptr_t)d & 15u)) & 15u) / sizeof(T));
        head = head < nc ? head : nc;
        if (lane < head) d[lane] = s[lane];
        const uint32_t nv = (nc - head) / VEC;
        const uint4 *sv = (const uint4 *)(s + head);
        uint4 *dv = (uint4 *)(d + head);
        for (uint32_t j = lane; j < nv; j += 64u) dv[j] = sv[j];
        for (uint32_t j = head + nv * VEC + lane; j < nc; j += 64u) d[j] = s[j];
    } else {
        for (uint32_t j = lane; j < nc; j += 64u) d[j] = s[j];
    }
}

// Labels of the containers that re-order a list (Elias-Fano: ascending, ROC: sampling order) from the permutation of the new
// object: segment s holds the merged list seg_list[s] (NULL: list s) at perm + seg_off[s]; perm value j >= |old_l| is batch entry
// j - |old_l| of that list, pair vals[add_off[l] + j - |old_l|] of the batch.  A wavefront per chunk; untouched lists are skipped.
__global__ void __launch_bounds__(256) k_app_labels_perm(const uint32_t *__restrict__ perm, const uint64_t *__restrict__ seg_off,
                                                         const uint32_t *__restrict__ seg_list, const uint64_t *__restrict__ old_off,
                                                         const uint64_t *__restrict__ add_off, const uint32_t *__restrict__ vals,
                                                         const Chunk *__restrict__ items, const uint64_t *__restrict__ n_items,
                                                         int64_t *__restrict__ labels) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t l = seg_list ? seg_list[ch.list] : ch.list;
        const uint64_t a0 = add_off[l];
        if (add_off[l + 1] == a0) continue;
        const uint64_t old_n = old_off[l + 1] - old_off[l], base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t q = ch.start + j, in_pos = perm[base + q];
            if (in_pos >= old_n) labels[vals[a0 + in_pos - old_n]] = (int64_t)((l << 32) | q);
        }
    }
}

inline dim3 app_chunk_grid(const ::vidc_ctx *c, uint64_t bound) {
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((bound + 3) / 4, (uint64_t)c->num_cu * 16)));
}

// the chunk table of nseg segments: items[0 .. item_off[nseg]), built on the device; bound: what the caller knows the count cannot exceed
struct AppChunks {
    Scratch s_cnt, s_off, s_items, s_tmp;
    const Chunk *items = nullptr;
    const uint64_t *n_items = nullptr;
    uint64_t bound = 0;
};
inline int app_chunks(::vidc_ctx *ctx, const uint64_t *d_len_off, uint64_t nseg, uint64_t total_elems, AppChunks &c) {
    c.bound = total_elems / APP_COPY_UNIT + nseg;
    VIDC_TRY(c.s_cnt.get(ctx, (nseg + 1) * 4));
    VIDC_TRY(c.s_off.get(ctx, (nseg + 1) * 8));
    VIDC_TRY(c.s_items.get(ctx, (c.bound + 1) * sizeof(Chunk)));
    if (nseg) {
        hipLaunchKernelGGL(k_app_count_chunks, req_grid(ctx, nseg), dim3(256), 0, ctx->stream, d_len_off, (uint32_t)nseg, c.s_cnt.as<uint32_t>());
        VIDC_TRY(device_exscan(ctx, c.s_cnt.as<uint32_t>(), (uint32_t)nseg, c.s_off.as<uint64_t>(), c.s_tmp));
        launch_fill_items(ctx->stream, c.s_off.as<uint64_t>(), (uint32_t)nseg, APP_COPY_UNIT, c.s_items.as<Chunk>(), c.bound, (uint32_t)ctx->num_cu);
        VIDC_HIP(hipGetLastError());
    } else {
        VIDC_HIP(hipMemsetAsync(c.s_off.p, 0, 8, ctx->stream));
    }
    c.items = c.s_items.as<Chunk>();
    c.n_items = c.s_off.as<uint64_t>() + nseg;
    return VIDC_OK;
}

// the batch, sorted by list: keys / vals (n_add each; key nlist = skipped), add_off / new_off (nlist + 1 each, device), n_valid (host)
struct AppendBatch {
    Scratch s_sort, s_hist, s_scan, s_tmp, s_off;
    Pinned h_back;
    uint64_t n_add = 0, nlist = 0, n_valid = 0;
    const uint32_t *keys = nullptr, *vals = nullptr;
    uint64_t *add_off = nullptr, *new_off = nullptr;
};

// the host-side argument checks every append makes before any device work; *out = NULL from here on
template <typename Obj>
inline int append_check(const ::vidc_ctx *ctx, const Obj *obj, Obj **out, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids) {
    if (out) *out = nullptr;
    if (!ctx || !obj || !out || (n_add && (!d_list_nos || !d_ids))) {
        set_error("append: NULL context, object, out or array");
        return VIDC_ERR_INVALID;
    }
    if (n_add >= 0xffffffffull) { set_error("append: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    return VIDC_OK;
}

// The stable LSD sort of n pairs (n > 0): two key and two value buffers of n words each, and where the sort stands -- kin / vin are the
// keys and the pair numbers in the current order (vin == NULL: the identity, nothing sorted yet).
struct AppSort {
    uint32_t n = 0;
    uint32_t *kb[2] = {nullptr, nullptr}, *vb[2] = {nullptr, nullptr};
    const uint32_t *kin = nullptr, *vin = nullptr;
};
inline int app_sort_scratch(::vidc_ctx *ctx, const AppSort &s, Scratch &s_hist, Scratch &s_scan) {
    const uint32_t ntiles = (s.n + APP_TILE - 1u) / APP_TILE;
    VIDC_TRY(s_hist.get(ctx, (size_t)ntiles * 256 * 4));
    VIDC_TRY(s_scan.get(ctx, ((size_t)ntiles * 256 + 1) * 8));
    return VIDC_OK;
}
// One phase: gather(kdst, vin) enqueues the kernel that writes the phase's 32-bit keys in the current order (position p holds the key of
// pair vin[p]), then `bits` key bits are sorted, 8 per pass, at least one pass.  The order of earlier phases survives inside equal keys:
// phases run from the least significant key to the most significant one.
template <typename Gather>
inline int app_sort_phase(::vidc_ctx *ctx, AppSort &s, uint32_t bits, Scratch &s_hist, Scratch &s_scan, Scratch &s_tmp, Gather &&gather) {
    const uint32_t n = s.n, ntiles = (n + APP_TILE - 1u) / APP_TILE;
    gather(s.kb[0], s.vin);
    VIDC_HIP(hipGetLastError());
    s.kin = s.kb[0];
    uint32_t *kout = s.kb[1], *vout = s.vin == s.vb[0] ? s.vb[1] : s.vb[0];
    const dim3 grid(std::min<uint32_t>(ntiles, (uint32_t)ctx->num_cu * 32u));
    for (uint32_t shift = 0; shift == 0 || shift < bits; shift += 8u) {
        hipLaunchKernelGGL(k_app_hist, grid, dim3(64), 0, ctx->stream, s.kin, n, shift, ntiles, s_hist.as<uint32_t>());
        VIDC_TRY(device_exscan(ctx, s_hist.as<uint32_t>(), ntiles * 256u, s_scan.as<uint64_t>(), s_tmp));
        hipLaunchKernelGGL(k_app_scatter, grid, dim3(64), 0, ctx->stream, s.kin, s.vin, n, shift, ntiles, s_scan.as<uint64_t>(), kout, vout);
        VIDC_HIP(hipGetLastError());
        s.kin = kout;
        s.vin = vout;
        kout = kout == s.kb[1] ? s.kb[0] : s.kb[1];
        vout = vout == s.vb[0] ? s.vb[1] : s.vb[0];
    }
    return VIDC_OK;
}

// steps 1-3 (header).  Ends with the call's read-back of the valid pair count: synchronises.
inline int append_sort_batch(::vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_old_off, uint64_t n_add, const int64_t *d_list_nos,
                             uint64_t *d_invalid, AppendBatch &b) {
    b.n_add = n_add;
    b.nlist = nlist;
    const uint32_t n = (uint32_t)n_add;
    VIDC_TRY(b.s_sort.get(ctx, ((size_t)n * 4 + 4) * 4));
    VIDC_TRY(b.s_off.get(ctx, 2 * (nlist + 1) * 8));
    VIDC_TRY(b.h_back.get(ctx, 64));
    AppSort s;
    s.n = n;
    s.kb[0] = b.s_sort.as<uint32_t>(); s.kb[1] = s.kb[0] + n; s.vb[0] = s.kb[1] + n; s.vb[1] = s.vb[0] + n;
    s.kin = s.kb[0];
    b.add_off = b.s_off.as<uint64_t>();
    b.new_off = b.add_off + nlist + 1;
    if (n) {
        VIDC_TRY(app_sort_scratch(ctx, s, b.s_hist, b.s_scan));
        uint32_t bits = 0;
        while (bits < 32u && (nlist >> bits)) bits++;  // keys are 0 .. nlist
        VIDC_TRY(app_sort_phase(ctx, s, bits, b.s_hist, b.s_scan, b.s_tmp, [&](uint32_t *kdst, const uint32_t *) {
            hipLaunchKernelGGL(k_app_keys, req_grid(ctx, n), dim3(256), 0, ctx->stream, d_list_nos, n_add, nlist, kdst, (unsigned long long *)d_invalid);
        }));
    }
    b.keys = s.kin;
    b.vals = s.vin;
    hipLaunchKernelGGL(k_app_bounds, req_grid(ctx, nlist + 1), dim3(256), 0, ctx->stream, b.keys, n, d_old_off, nlist, b.add_off, b.new_off);
    VIDC_HIP(hipGetLastError());
    uint64_t *h = b.h_back.as<uint64_t>();
    VIDC_HIP(hipMemcpyAsync(h, b.add_off + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    b.n_valid = h[0];
    return VIDC_OK;
}

// Append by rebuild (packed bits, Elias-Fano, wavelet tree): the old object is decoded into scratch, merged with the batch (step 4)
// and handed to the codec's own device-offsets encoder.  decode_all(d_out), encode(d_new_off, ntotal_new, d_merged).  labels:
// plain_labels says whether the merge writes them (input-order containers) or only the -1 of the skipped pairs.
struct AppendMerged {
    AppendBatch batch;
    Scratch s_old, s_merged;
    uint64_t ntotal_new = 0;
};
template <typename DecodeAll>
inline int append_merge(::vidc_ctx *ctx, uint64_t nlist, uint64_t ntotal_old, const uint64_t *d_old_off, uint64_t n_add,
                        const int64_t *d_list_nos, const uint64_t *d_ids, int64_t *d_labels, uint64_t *d_invalid, bool plain_labels,
                        AppendMerged &m, DecodeAll &&decode_all) {
    VIDC_TRY(append_sort_batch(ctx, nlist, d_old_off, n_add, d_list_nos, d_invalid, m.batch));
    m.ntotal_new = ntotal_old + m.batch.n_valid;
    VIDC_TRY(m.s_merged.get(ctx, (m.ntotal_new ? m.ntotal_new : 1) * 8));
    if (ntotal_old) {
        VIDC_TRY(m.s_old.get(ctx, ntotal_old * 8));
        VIDC_TRY(decode_all(m.s_old.as<uint64_t>()));
        AppChunks ch;
        VIDC_TRY(app_chunks(ctx, d_old_off, nlist, ntotal_old, ch));
        hipLaunchKernelGGL(k_app_copy<uint64_t>, app_chunk_grid(ctx, ch.bound), dim3(256), 0, ctx->stream, m.s_old.as<uint64_t>(), d_old_off,
                           (const uint64_t *)nullptr, (const uint64_t *)nullptr, (const uint32_t *)nullptr, m.batch.new_off,
                           m.s_merged.as<uint64_t>(), ch.items, ch.n_items);
        VIDC_HIP(hipGetLastError());
        if (n_add)
            hipLaunchKernelGGL(k_app_place, req_grid(ctx, n_add), dim3(256), 0, ctx->stream, m.batch.keys, m.batch.vals, (uint32_t)n_add, nlist,
                               d_old_off, m.batch.add_off, m.batch.new_off, d_ids, m.s_merged.as<uint64_t>(), d_labels, plain_labels);
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(vidc_stream_wait(ctx->stream));  // (the chunk table goes back to the context's cache)
        return VIDC_OK;
    }
    if (n_add) {
        hipLaunchKernelGGL(k_app_place, req_grid(ctx, n_add), dim3(256), 0, ctx->stream, m.batch.keys, m.batch.vals, (uint32_t)n_add, nlist,
                           d_old_off, m.batch.add_off, m.batch.new_off, d_ids, m.s_merged.as<uint64_t>(), d_labels, plain_labels);
        VIDC_HIP(hipGetLastError());
    }
    return VIDC_OK;
}

// labels of a re-ordering container from the permutation of its new object (k_app_labels_perm); synchronises
inline int append_labels_from_perm(::vidc_ctx *ctx, const AppendBatch &b, const uint32_t *d_perm, const uint64_t *d_seg_off, const uint32_t *d_seg_list,
                                   uint64_t nseg, uint64_t total, const uint64_t *d_old_off, int64_t *d_labels) {
    if (!d_labels || !b.n_valid) return VIDC_OK;
    AppChunks ch;
    VIDC_TRY(app_chunks(ctx, d_seg_off, nseg, total, ch));
    hipLaunchKernelGGL(k_app_labels_perm, app_chunk_grid(ctx, ch.bound), dim3(256), 0, ctx->stream, d_perm, d_seg_off, d_seg_list, d_old_off,
                       (const uint64_t *)b.add_off, b.vals, ch.items, ch.n_items, d_labels);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
