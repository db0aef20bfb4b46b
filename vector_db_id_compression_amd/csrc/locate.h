// locate.h -- the inverse of translate_labels for the containers that have to be decoded to be searched (packed bits, Elias-Fano,
// ROC; vidc_*_locate_dev): a batch of (list number, id) pairs, device-resident, is answered with the label list << 32 | offset of an
// entry equal to the id.  It is the membership test of remove.h with the place of the hit kept:
//
//   1-2. the batch is sorted by (list, id) and cut into runs exactly as a remove does it (remove_sort_batch, k_app_bounds): a pair
//      that cannot match carries the key behind the last list, an id the object cannot hold is counted as missing there.
//   3. mark (k_loc_mark): a wavefront per chunk of RM_UNIT decoded elements (the chunk tables of app_chunks) -- every element
//      binary-searches its list's run and, on equality, does a 64-bit atomicMin of its own label into first_pos[first equal run
//      position] (all-ones before).  Segments are decoded in ascending list order, so the order of the labels is the decoded order:
//      the minimum is the lowest list, then the lowest offset.  A minimum does not depend on the order its operands arrive in:
//      nothing timing-dependent decides a result, two wavefronts that race on one slot leave the same word whoever comes first.
//   4. labels (k_loc_labels): a thread per sorted position reads first_pos of the first position of its value in its run and writes
//      it to labels[pair number] -- batch order, every element written; -1 for no hit and for the pairs keyed behind the last
//      list.  The valid pairs without a hit are counted as missing here (k_rm_missing's rule: repeated pairs each count).
//
// The object is decoded into scratch (decode_all; ROC: the candidate lists a remove would decode) and not changed.  No kernel of the
// remove is touched.  Out of scope: segmented ROC objects, sharded containers and graph objects; a search inside the compressed
// Elias-Fano lists without decoding them (decode_all runs at memory rate); the Faiss adapter header; a direct map kept beside the
// object.  Included by several translation units: everything has internal linkage.
// (That search now exists beside this file: vidc_ef_rank_dev, ef_rank_ref.h and the rank kernels of ef.hip; locate does not use it.)
#pragma once
#include "remove.h"

namespace vidc {
namespace {

// Mark, a wavefront per chunk: segment s of `dec` (seg_off) is list seg_list[s] (NULL: list s); its run is run_off[l] .. run_off[l + 1]
// (any != 0: run_off[0] .. run_off[1]).  first_pos[first equal run position] = min(itself, l << 32 | position in the list).  An
// empty run is not searched.
__global__ void __launch_bounds__(256) k_loc_mark(const uint64_t *__restrict__ dec, const uint64_t *__restrict__ seg_off,
                                                  const uint32_t *__restrict__ seg_list, const uint64_t *__restrict__ run_off, uint32_t any,
                                                  const uint64_t *__restrict__ sid, const Chunk *__restrict__ items,
                                                  const uint64_t *__restrict__ n_items, unsigned long long *first_pos) {
    const uint64_t total = *n_items;
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = seg_off[ch.list], n = seg_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < RM_UNIT ? n - ch.start : RM_UNIT);
        const uint64_t l = seg_list ? seg_list[ch.list] : ch.list, run = any ? 0u : l;
        const uint32_t r0 = (uint32_t)run_off[run], r1 = (uint32_t)run_off[run + 1];
        if (r1 == r0) continue;
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t id = dec[base + ch.start + j];
            const uint32_t at = rm_lower_bound(sid, r0, r1, id);
            if (at < r1 && sid[at] == id) atomicMin(&first_pos[at], (unsigned long long)((l << 32) | (ch.start + j)));
        }
    }
}

// labels[vals[p]] = first_pos[first position of p's value in its run], or -1 (no hit; keys[p] == nl: skipped, invalid or too wide);
// *missing += the positions of a run without a hit.  vals is a permutation of 0 .. n - 1: every label is written once.
__global__ void __launch_bounds__(256) k_loc_labels(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n, uint64_t nl,
                                                    const uint64_t *__restrict__ run_off, const uint64_t *__restrict__ sid,
                                                    const unsigned long long *__restrict__ first_pos, int64_t *__restrict__ labels,
                                                    unsigned long long *missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); p0 < n; p0 += stride) {  // (p0: wavefront-uniform)
        const uint64_t p = p0 + dev::lane_id();
        bool miss = false;
        if (p < n) {
            int64_t lab = -1;
            if ((uint64_t)keys[p] < nl) {
                lab = (int64_t)first_pos[rm_lower_bound(sid, (uint32_t)run_off[keys[p]], (uint32_t)p, sid[p])];  // (all-ones: -1)
                miss = lab < 0;
            }
            labels[vals[p]] = lab;
        }
        req_count_invalid(miss, missing);
    }
}

// the host-side argument checks every locate makes before any device work
inline int locate_check(const ::vidc_ctx *ctx, const void *obj, uint64_t n, const uint64_t *d_ids, const int64_t *d_labels) {
    if (!ctx || !obj || (n && (!d_ids || !d_labels))) {
        set_error("locate: NULL context, object, id or label array");
        return VIDC_ERR_INVALID;
    }
    if (n >= 0xffffffffull) { set_error("locate: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    return VIDC_OK;
}

// the sorted batch and its first_pos words (n, all-ones).  n > 0.  Enqueue only.
struct LocateBatch {
    RemoveBatch batch;
    Scratch s_first;
    unsigned long long *first_pos = nullptr;
};
inline int locate_sort_batch(::vidc_ctx *ctx, uint64_t nlist, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, uint32_t id_bits,
                             uint64_t *d_missing, uint64_t *d_invalid, LocateBatch &b) {
    VIDC_TRY(remove_sort_batch(ctx, nlist, n, d_list_nos, d_ids, id_bits, d_missing, d_invalid, b.batch));
    VIDC_TRY(b.s_first.get(ctx, (size_t)n * 8));
    b.first_pos = b.s_first.as<unsigned long long>();
    VIDC_HIP(hipMemsetAsync(b.first_pos, 0xff, (size_t)n * 8, ctx->stream));
    return VIDC_OK;
}
// step 3 on a decoded CSR: nseg segments in ascending list order (d_seg_off, total elements in d_dec; segment s is list d_seg_list[s],
// NULL: list s).  ch: the call's chunk table (alive until the stream has run).  Enqueue only; total > 0.
inline int locate_mark(::vidc_ctx *ctx, const LocateBatch &b, const uint64_t *d_dec, const uint64_t *d_seg_off, const uint32_t *d_seg_list,
                       uint64_t nseg, uint64_t total, AppChunks &ch) {
    VIDC_TRY(app_chunks(ctx, d_seg_off, nseg, total, ch));
    hipLaunchKernelGGL(k_loc_mark, app_chunk_grid(ctx, ch.bound), dim3(256), 0, ctx->stream, d_dec, d_seg_off, d_seg_list, b.batch.run_off,
                       b.batch.any, b.batch.sid, ch.items, ch.n_items, b.first_pos);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
// step 4: after the call's locate_mark
inline int locate_labels(::vidc_ctx *ctx, const LocateBatch &b, int64_t *d_labels, uint64_t *d_missing) {
    hipLaunchKernelGGL(k_loc_labels, req_grid(ctx, b.batch.n), dim3(256), 0, ctx->stream, b.batch.keys, b.batch.vals, b.batch.n, b.batch.nl,
                       b.batch.run_off, b.batch.sid, (const unsigned long long *)b.first_pos, d_labels, (unsigned long long *)d_missing);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// Locate in a container that is decoded as a whole (packed bits, Elias-Fano): decode_all(d_out) into scratch, the mark, the labels.
// n > 0.  No read-back; the call waits for its last kernel (the scratch blocks go back to the context's cache) and leaves the sum of
// its kernels' times in ctx->last_kernel_ms.
template <typename DecodeAll>
inline int locate_decoded(::vidc_ctx *ctx, uint64_t nlist, uint64_t ntotal, const uint64_t *d_off, uint64_t n, const int64_t *d_list_nos,
                          const uint64_t *d_ids, uint32_t id_bits, int64_t *d_labels, uint64_t *d_missing, uint64_t *d_invalid,
                          DecodeAll &&decode_all) {
    LocateBatch b;
    AppChunks ch;
    Scratch s_dec;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    EventTimer tm = EventTimer::started(ctx);
    VIDC_TRY(locate_sort_batch(ctx, nlist, n, d_list_nos, d_ids, id_bits, d_missing, d_invalid, b));
    double kernel_ms = 0;
    if (ntotal) {
        kernel_ms = tm.stop();
        VIDC_TRY(s_dec.get(ctx, ntotal * 8));
        VIDC_TRY(decode_all(s_dec.as<uint64_t>()));
        kernel_ms += ctx->last_kernel_ms;
        (void)tm.start();
        VIDC_TRY(locate_mark(ctx, b, s_dec.as<uint64_t>(), d_off, nullptr, nlist, ntotal, ch));
    }
    VIDC_TRY(locate_labels(ctx, b, d_labels, d_missing));
    ctx->last_kernel_ms = kernel_ms + tm.stop();
    guard.disarm();
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
