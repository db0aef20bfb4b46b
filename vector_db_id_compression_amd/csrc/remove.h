// remove.h -- the membership test and the stream compaction shared by the vidc_*_remove_dev calls: a batch of (list number, id) pairs,
// device-resident, names the entries that leave the lists of an existing object.
//
//   1. the batch is sorted by (list, id) with the stable LSD sorter of append.h (app_sort_phase): the low half of the id, the high
//      half where the object can hold ids >= 2^32, then the list key.  A pair that cannot match -- a skipped list number, or an id the
//      object cannot hold (id >> id_bits != 0: counted as missing) -- gets the key behind the last list and sorts out of every run.
//      In any-list mode (no list numbers) the batch is the run of one virtual list 0.
//   2. bounds (k_app_bounds): run_off[l] .. run_off[l + 1] is list l's run, ascending by id; sid[] holds the sorted ids themselves.
//   3. mark: a wavefront per chunk of RM_UNIT decoded elements (the chunk tables of app_chunks) -- every element binary-searches its
//      list's run, writes its `removed` byte and sets hit[] of the first equal run position; the chunk keeps its kill count.
//   4. missing: run position p is missing iff hit[first position of its value in its run] == 0.  Found bytes (optional, for the
//      sharded remove's join): the same flag per pair, sent back to batch order through the sorter's pair numbers.
//   5. compact: the destination of a survivor is (exclusive scan of the chunk kill counts) + (ballot prefix inside the wavefront);
//      new_off[s] = seg_off[s] - kills in front of segment s.  No atomic decides a position: the output is the same on every run.
// What crosses PCIe: the survivor count (8 bytes).  Included by several translation units: everything has internal linkage.
#pragma once
#include "append.h"
#include "host_call.h"

namespace vidc {
namespace {

constexpr uint32_t RM_UNIT = APP_COPY_UNIT;  // decoded elements per wavefront of the mark and of the compaction
enum : uint32_t { RM_KEY_ID_LO = 0, RM_KEY_ID_HI = 1, RM_KEY_LIST = 2 };

// keys[p] = the 32-bit key of the pair at sorted position p (pair vals[p]; vals == NULL: pair p).  RM_KEY_LIST makes the key as
// k_app_keys does (nl = number of lists; list_nos == NULL: every pair is of list 0), counts the list numbers >= nl in *invalid and
// the valid pairs whose id does not fit id_bits in *missing.
__global__ void __launch_bounds__(256) k_rm_keys(uint32_t mode, const int64_t *__restrict__ list_nos, const uint64_t *__restrict__ ids,
                                                 const uint32_t *__restrict__ vals, uint64_t n, uint64_t nl, uint32_t id_bits,
                                                 uint32_t *__restrict__ keys, unsigned long long *invalid, unsigned long long *missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); p0 < n; p0 += stride) {  // (p0: wavefront-uniform)
        const uint64_t p = p0 + dev::lane_id();
        const bool in = p < n;
        const uint64_t i = in ? (vals ? (uint64_t)vals[p] : p) : 0u;
        const uint64_t id = in ? ids[i] : 0u;
        if (mode != RM_KEY_LIST) {
            if (in) keys[p] = mode == RM_KEY_ID_LO ? (uint32_t)id : (uint32_t)(id >> 32);
            continue;
        }
        const int64_t l = in ? (list_nos ? list_nos[i] : 0) : -1;
        const bool ok = l >= 0 && (uint64_t)l < nl;
        const bool wide = ok && id_bits < 64u && (id >> id_bits) != 0u;
        if (in) keys[p] = ok && !wide ? (uint32_t)l : (uint32_t)nl;
        req_count_invalid(l >= 0 && !ok, invalid);
        req_count_invalid(wide, missing);
    }
}

// sid[p] = ids[vals[p]]: what the binary searches probe
__global__ void __launch_bounds__(256) k_rm_sorted_ids(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ vals, uint32_t n,
                                                       uint64_t *__restrict__ sid) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) sid[p] = ids[vals[p]];
}

// first position of [lo, hi) whose id is >= id
__device__ __forceinline__ uint32_t rm_lower_bound(const uint64_t *__restrict__ sid, uint32_t lo, uint32_t hi, uint64_t id) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sid[mid] < id) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// Mark, a wavefront per chunk: segment s of `dec` (seg_off) is list seg_list[s] (NULL: list s); its run is run_off[l] .. run_off[l + 1]
// (any != 0: run_off[0] .. run_off[1]).  removed[position in dec] = 0 / 1; removed_obj (optional) gets the same byte at
// obj_off[l] + position in the list; chunk_kill[c] = removed elements of chunk c.  An empty run is not searched.
__global__ void __launch_bounds__(256) k_rm_mark(const uint64_t *__restrict__ dec, const uint64_t *__restrict__ seg_off,
                                                 const uint32_t *__restrict__ seg_list, const uint64_t *__restrict__ run_off, uint32_t any,
                                                 const uint64_t *__restrict__ sid, const Chunk *__restrict__ items,
                                                 const uint64_t *__restrict__ n_items, uint8_t *__restrict__ removed,
                                                 uint8_t *__restrict__ removed_obj, const uint64_t *__restrict__ obj_off, uint32_t *hit,
                                                 uint32_t *__restrict__ chunk_kill) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < RM_UNIT ? n - ch.start : RM_UNIT);
        const uint64_t l = seg_list ? seg_list[ch.list] : ch.list, run = any ? 0u : l;
        const uint32_t r0 = (uint32_t)run_off[run], r1 = (uint32_t)run_off[run + 1];
        uint32_t kills = 0;
        for (uint32_t j0 = 0; j0 < nc; j0 += 64u) {  // (j0, nc: wavefront-uniform)
            const uint32_t j = j0 + lane;
            const bool in = j < nc;
            bool found = false;
            if (in && r1 > r0) {
                const uint64_t id = dec[base + ch.start + j];
                const uint32_t at = rm_lower_bound(sid, r0, r1, id);
                found = at < r1 && sid[at] == id;
                if (found) __hip_atomic_store(&hit[at], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (in) {
                removed[base + ch.start + j] = found ? 1 : 0;
                if (removed_obj) removed_obj[obj_off[l] + ch.start + j] = found ? 1 : 0;
            }
            kills += dev::popc64(__ballot(found));
        }
        if (lane == 0) chunk_kill[c] = kills;
    }
}

// *missing += sorted positions p of a run (keys[p] < nl) whose value no element hit
__global__ void __launch_bounds__(256) k_rm_missing(const uint32_t *__restrict__ keys, uint32_t n, uint64_t nl, const uint64_t *__restrict__ run_off,
                                                    const uint64_t *__restrict__ sid, const uint32_t *__restrict__ hit,
                                                    unsigned long long *missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); p0 < n; p0 += stride) {  // (p0: wavefront-uniform)
        const uint64_t p = p0 + dev::lane_id();
        bool miss = false;
        if (p < n && (uint64_t)keys[p] < nl) {
            const uint32_t first = rm_lower_bound(sid, (uint32_t)run_off[keys[p]], (uint32_t)p, sid[p]);
            miss = hit[first] == 0u;
        }
        req_count_invalid(miss, missing);
    }
}

// found[vals[p]] = 1 iff sorted position p belongs to a run (keys[p] < nl) and some element hit its value: one byte per pair, in batch
// order, every byte written (vals is a permutation of 0 .. n - 1).  Skipped pairs and too-wide ids carry the key nl: 0.
__global__ void __launch_bounds__(256) k_rm_pair_found(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint64_t nl,
                                                       const uint64_t *__restrict__ run_off, const uint64_t *__restrict__ sid,
                                                       const uint32_t *__restrict__ hit, uint8_t *__restrict__ found) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        uint32_t f = 0;
        if ((uint64_t)keys[p] < nl) f = hit[rm_lower_bound(sid, (uint32_t)run_off[keys[p]], (uint32_t)p, sid[p])];
        found[vals[p]] = f ? 1 : 0;
    }
}

// new_off[s] = seg_off[s] - seg_off[0] - (kills in front of segment s), s = 0 .. nseg: item_off is the chunk table's offset array,
// ks the exclusive scan of chunk_kill
__global__ void __launch_bounds__(256) k_rm_new_off(const uint64_t *__restrict__ seg_off, uint64_t nseg, const uint64_t *__restrict__ item_off,
                                                    const uint64_t *__restrict__ ks, uint64_t *__restrict__ new_off) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= nseg; s += (uint64_t)gridDim.x * blockDim.x)
        new_off[s] = seg_off[s] - seg_off[0] - ks[item_off[s]];
}

// Compact, a wavefront per chunk: the survivors of segment s go to out + dst_off[s], order kept.  take (optional): segments with
// take[s] == 0 are left out.
__global__ void __launch_bounds__(256) k_rm_compact(const uint64_t *__restrict__ dec, const uint64_t *__restrict__ seg_off,
                                                    const uint8_t *__restrict__ removed, const Chunk *__restrict__ items,
                                                    const uint64_t *__restrict__ n_items, const uint64_t *__restrict__ item_off,
                                                    const uint64_t *__restrict__ ks, const uint64_t *__restrict__ dst_off,
                                                    const uint32_t *__restrict__ take, uint64_t *__restrict__ out) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        if (take && !take[ch.list]) continue;
        const uint64_t base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < RM_UNIT ? n - ch.start : RM_UNIT);
        const uint64_t before = ks[c] - ks[item_off[ch.list]];  // kills of the segment in front of this chunk
        uint64_t *d = out + dst_off[ch.list] + (ch.start - before);
        const uint64_t *s = dec + base + ch.start;
        const uint8_t *rm = removed + base + ch.start;
        uint32_t kept = 0;
        for (uint32_t j0 = 0; j0 < nc; j0 += 64u) {  // (j0, nc: wavefront-uniform)
            const uint32_t j = j0 + lane;
            const bool keep = j < nc && rm[j] == 0;
            const uint64_t b = __ballot(keep);
            if (keep) d[kept + dev::mbcnt(b)] = s[j];
            kept += dev::popc64(b);
        }
    }
}

// the host-side argument checks every remove makes before any device work; *out = NULL from here on
template <typename Obj>
inline int remove_check(const ::vidc_ctx *ctx, const Obj *obj, Obj **out, uint64_t n_rm, const uint64_t *d_ids) {
    if (out) *out = nullptr;
    if (!ctx || !obj || !out || (n_rm && !d_ids)) {
        set_error("remove: NULL context, object, out or id array");
        return VIDC_ERR_INVALID;
    }
    if (n_rm >= 0xffffffffull) { set_error("remove: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    return VIDC_OK;
}

// the batch, sorted by (list, id): keys / sid (n each), run_off (nl + 1, device); nl = nlist, or 1 in any-list mode
struct RemoveBatch {
    Scratch s_sort, s_hist, s_scan, s_tmp, s_off, s_sid, s_hit, s_zero;
    uint32_t n = 0, any = 0;
    uint64_t nl = 0;
    const uint32_t *keys = nullptr, *vals = nullptr;  // vals[p]: the pair at sorted position p
    const uint64_t *run_off = nullptr, *sid = nullptr;
    uint32_t *hit = nullptr;
};

// steps 1-2 (header).  id_bits: the width of the ids the object can hold.  Enqueue only.
inline int remove_sort_batch(::vidc_ctx *ctx, uint64_t nlist, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids, uint32_t id_bits,
                             uint64_t *d_missing, uint64_t *d_invalid, RemoveBatch &b) {
    const uint32_t n = (uint32_t)n_rm;
    b.n = n;
    b.any = d_list_nos ? 0u : 1u;
    b.nl = d_list_nos ? nlist : 1u;
    VIDC_TRY(b.s_off.get(ctx, 2 * (b.nl + 1) * 8));  // run_off | what k_app_bounds adds its old offsets to
    VIDC_TRY(b.s_sid.get(ctx, ((size_t)n + 1) * 8));
    VIDC_TRY(b.s_hit.get(ctx, ((size_t)n + 1) * 4));
    uint64_t *run_off = b.s_off.as<uint64_t>();
    b.run_off = run_off;
    b.sid = b.s_sid.as<uint64_t>();
    b.hit = b.s_hit.as<uint32_t>();
    if (!n) {
        VIDC_HIP(hipMemsetAsync(run_off, 0, (b.nl + 1) * 8, ctx->stream));
        return VIDC_OK;
    }
    VIDC_HIP(hipMemsetAsync(b.hit, 0, (size_t)n * 4, ctx->stream));
    VIDC_TRY(b.s_sort.get(ctx, ((size_t)n * 4 + 4) * 4));
    AppSort s;
    s.n = n;
    s.kb[0] = b.s_sort.as<uint32_t>(); s.kb[1] = s.kb[0] + n; s.vb[0] = s.kb[1] + n; s.vb[1] = s.vb[0] + n;
    VIDC_TRY(app_sort_scratch(ctx, s, b.s_hist, b.s_scan));
    const dim3 grid = req_grid(ctx, n);
    auto gather = [&](uint32_t mode) {
        return [&, mode](uint32_t *kdst, const uint32_t *vin) {
            hipLaunchKernelGGL(k_rm_keys, grid, dim3(256), 0, ctx->stream, mode, d_list_nos, d_ids, vin, (uint64_t)n, b.nl, id_bits, kdst,
                               (unsigned long long *)d_invalid, (unsigned long long *)d_missing);
        };
    };
    if (id_bits) VIDC_TRY(app_sort_phase(ctx, s, std::min(id_bits, 32u), b.s_hist, b.s_scan, b.s_tmp, gather(RM_KEY_ID_LO)));
    if (id_bits > 32u) VIDC_TRY(app_sort_phase(ctx, s, id_bits - 32u, b.s_hist, b.s_scan, b.s_tmp, gather(RM_KEY_ID_HI)));
    uint32_t lbits = 0;
    while (lbits < 32u && (b.nl >> lbits)) lbits++;  // keys are 0 .. nl
    VIDC_TRY(app_sort_phase(ctx, s, lbits, b.s_hist, b.s_scan, b.s_tmp, gather(RM_KEY_LIST)));
    b.keys = s.kin;
    b.vals = s.vin;
    // (k_app_bounds also adds the run bounds to a set of old offsets: zeros here, the sums are not used)
    VIDC_TRY(b.s_zero.get(ctx, (b.nl + 1) * 8));
    VIDC_HIP(hipMemsetAsync(b.s_zero.p, 0, (b.nl + 1) * 8, ctx->stream));
    hipLaunchKernelGGL(k_app_bounds, req_grid(ctx, b.nl + 1), dim3(256), 0, ctx->stream, s.kin, n, (const uint64_t *)b.s_zero.as<uint64_t>(), b.nl,
                       run_off, run_off + b.nl + 1);
    hipLaunchKernelGGL(k_rm_sorted_ids, grid, dim3(256), 0, ctx->stream, d_ids, s.vin, n, b.s_sid.as<uint64_t>());
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// steps 3-5 on a decoded CSR: nseg segments (d_seg_off, total elements in d_dec; segment s is list d_seg_list[s], NULL: list s).
// d_removed: total bytes, every one written.  Afterwards new_off (nseg + 1, device) are the offsets of the survivors and ks / the
// chunk table are what remove_compact places them by.  Enqueue only; total > 0.
struct RemoveMarked {
    AppChunks ch;
    Scratch s_kill, s_ks, s_tmp, s_new;
    const uint64_t *ks = nullptr;
    uint64_t *new_off = nullptr;
};
inline int remove_mark(::vidc_ctx *ctx, const RemoveBatch &b, const uint64_t *d_dec, const uint64_t *d_seg_off, const uint32_t *d_seg_list,
                       uint64_t nseg, uint64_t total, uint8_t *d_removed, uint8_t *d_removed_obj, const uint64_t *d_obj_off,
                       uint64_t *d_missing, RemoveMarked &m) {
    VIDC_TRY(app_chunks(ctx, d_seg_off, nseg, total, m.ch));
    const uint64_t nk = m.ch.bound + 1;  // (entries behind the last chunk stay zero: the scan runs over the bound)
    VIDC_TRY(m.s_kill.get(ctx, nk * 4));
    VIDC_TRY(m.s_ks.get(ctx, (nk + 1) * 8));
    VIDC_TRY(m.s_new.get(ctx, (nseg + 1) * 8));
    m.ks = m.s_ks.as<uint64_t>();
    m.new_off = m.s_new.as<uint64_t>();
    VIDC_HIP(hipMemsetAsync(m.s_kill.p, 0, nk * 4, ctx->stream));
    hipLaunchKernelGGL(k_rm_mark, app_chunk_grid(ctx, m.ch.bound), dim3(256), 0, ctx->stream, d_dec, d_seg_off, d_seg_list, b.run_off, b.any, b.sid,
                       m.ch.items, m.ch.n_items, d_removed, d_removed_obj, d_obj_off, b.hit, m.s_kill.as<uint32_t>());
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(device_exscan(ctx, m.s_kill.as<uint32_t>(), (uint32_t)nk, m.s_ks.as<uint64_t>(), m.s_tmp));
    hipLaunchKernelGGL(k_rm_new_off, req_grid(ctx, nseg + 1), dim3(256), 0, ctx->stream, d_seg_off, nseg, (const uint64_t *)m.ch.s_off.as<uint64_t>(),
                       m.ks, m.new_off);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
// step 4: after every remove_mark of the call
inline int remove_count_missing(::vidc_ctx *ctx, const RemoveBatch &b, uint64_t *d_missing) {
    if (!d_missing || !b.n) return VIDC_OK;
    hipLaunchKernelGGL(k_rm_missing, req_grid(ctx, b.n), dim3(256), 0, ctx->stream, b.keys, b.n, b.nl, b.run_off, b.sid, (const uint32_t *)b.hit,
                       (unsigned long long *)d_missing);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
// the per-pair found bytes (d_pair_found: n bytes in batch order, NULL: nothing runs): where remove_count_missing runs
inline int remove_pair_found(::vidc_ctx *ctx, const RemoveBatch &b, uint8_t *d_pair_found) {
    if (!d_pair_found || !b.n) return VIDC_OK;
    hipLaunchKernelGGL(k_rm_pair_found, req_grid(ctx, b.n), dim3(256), 0, ctx->stream, b.keys, b.vals, b.n, b.nl, b.run_off, b.sid,
                       (const uint32_t *)b.hit, d_pair_found);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
inline int remove_compact(::vidc_ctx *ctx, const RemoveMarked &m, const uint64_t *d_dec, const uint64_t *d_seg_off, const uint8_t *d_removed,
                          const uint64_t *d_dst_off, const uint32_t *d_take, uint64_t *d_out) {
    hipLaunchKernelGGL(k_rm_compact, app_chunk_grid(ctx, m.ch.bound), dim3(256), 0, ctx->stream, d_dec, d_seg_off, d_removed, m.ch.items, m.ch.n_items,
                       (const uint64_t *)m.ch.s_off.as<uint64_t>(), m.ks, d_dst_off, d_take, d_out);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// Remove by rebuild (packed bits, Elias-Fano): the old object is decoded into scratch, marked and compacted; the caller hands
// (new_off, ntotal_new, survivors) to the codec's own device-offsets encoder.  decode_all(d_out).  Ends with the call's read-back
// of the survivor count: synchronises.  kernel_ms: the kernels so far (the decode included).
struct RemoveRebuilt {
    RemoveBatch batch;
    RemoveMarked marked;
    Scratch s_old, s_out, s_rm, s_new;
    Pinned h_back;
    uint64_t ntotal_new = 0;
    uint64_t *new_off = nullptr;
    double kernel_ms = 0;
};
template <typename DecodeAll>
inline int remove_rebuild(::vidc_ctx *ctx, uint64_t nlist, uint64_t ntotal_old, const uint64_t *d_old_off, uint64_t n_rm,
                          const int64_t *d_list_nos, const uint64_t *d_ids, uint32_t id_bits, uint8_t *d_removed, uint64_t *d_missing,
                          uint64_t *d_invalid, uint8_t *d_pair_found, RemoveRebuilt &m, DecodeAll &&decode_all) {
    VIDC_TRY(m.h_back.get(ctx, 64));
    EventTimer tm = EventTimer::started(ctx);
    VIDC_TRY(remove_sort_batch(ctx, nlist, n_rm, d_list_nos, d_ids, id_bits, d_missing, d_invalid, m.batch));
    if (!ntotal_old) {  // nothing to decode: every list stays empty, every pair of a run is missing
        VIDC_TRY(m.s_new.get(ctx, (nlist + 1) * 8));
        VIDC_TRY(m.s_out.get(ctx, 8));
        m.new_off = m.s_new.as<uint64_t>();
        VIDC_HIP(hipMemsetAsync(m.new_off, 0, (nlist + 1) * 8, ctx->stream));
        VIDC_TRY(remove_count_missing(ctx, m.batch, d_missing));
        VIDC_TRY(remove_pair_found(ctx, m.batch, d_pair_found));
        m.kernel_ms = tm.stop();
        VIDC_HIP(vidc_stream_wait(ctx->stream));
        m.ntotal_new = 0;
        return VIDC_OK;
    }
    m.kernel_ms = tm.stop();
    VIDC_TRY(m.s_old.get(ctx, ntotal_old * 8));
    VIDC_TRY(m.s_out.get(ctx, ntotal_old * 8));
    uint8_t *removed = d_removed;
    if (!removed) {
        VIDC_TRY(m.s_rm.get(ctx, ntotal_old));
        removed = m.s_rm.as<uint8_t>();
    }
    VIDC_TRY(decode_all(m.s_old.as<uint64_t>()));
    m.kernel_ms += ctx->last_kernel_ms;
    (void)tm.start();
    VIDC_TRY(remove_mark(ctx, m.batch, m.s_old.as<uint64_t>(), d_old_off, nullptr, nlist, ntotal_old, removed, nullptr, nullptr, d_missing, m.marked));
    VIDC_TRY(remove_count_missing(ctx, m.batch, d_missing));
    VIDC_TRY(remove_pair_found(ctx, m.batch, d_pair_found));
    m.new_off = m.marked.new_off;
    VIDC_TRY(remove_compact(ctx, m.marked, m.s_old.as<uint64_t>(), d_old_off, removed, m.new_off, nullptr, m.s_out.as<uint64_t>()));
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
