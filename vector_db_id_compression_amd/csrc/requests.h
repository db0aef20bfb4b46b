// requests.h -- device-resident requests (vidc_*_translate_labels_dev, vidc_*_decode_rows_dev / vidc_compact_rows_decode_dev):
// the label / node checks of the host-array calls, done on the device.  A label is Faiss's lo_build(list_no, offset) =
// list_no << 32 | offset; a negative label or node is "no result" (-1 out, not counted), one outside the object is invalid (-1 out,
// counted).  Included by several translation units: everything here has internal linkage.
#pragma once
#include "common.h"
#include "wave.h"

namespace vidc {
namespace {

// *cnt += invalid labels of the wavefront: one ballot, and one atomic from the first active lane of a wavefront that saw any
// (an all-valid request does no atomics).  Every active lane of the wavefront must call it.
__device__ __forceinline__ void req_count_invalid(bool bad, unsigned long long *cnt) {
    const uint64_t b = __ballot(bad);
    if (b && cnt && dev::lane_id() == dev::ff1(__ballot(true))) atomicAdd(cnt, (unsigned long long)dev::popc64(b));
}

// label -> (list, offset); false for a negative label.  The list still has to be checked against nlist before anything is loaded.
__device__ __forceinline__ bool req_label(int64_t lab, uint64_t &list, uint64_t &off) {
    list = (uint64_t)lab >> 32;
    off = (uint64_t)lab & 0xffffffffull;
    return lab >= 0;
}

// sanitize pass of a row request: out[i] = nodes[i], or 0 for a node outside [0, N) (the row decoders then stay inside the object;
// req_rows_fixup overwrites those rows).  N > 0.
template <typename I>
__global__ void __launch_bounds__(256) k_req_nodes_sanitize(const int64_t *__restrict__ nodes, uint64_t m, uint64_t N, I *__restrict__ out,
                                                            unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < m; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + dev::lane_id();
        const int64_t v = i < m ? nodes[i] : 0;
        const bool ok = v >= 0 && (uint64_t)v < N;
        if (i < m) out[i] = ok ? (I)v : (I)0;
        req_count_invalid(i < m && v >= 0 && !ok, invalid);
    }
}

// *dst += *v (a count the host found, added in stream order)
__global__ void k_req_add(const unsigned long long *v, unsigned long long *dst) {
    if (threadIdx.x == 0 && *v) atomicAdd(dst, *v);
}

// fix-up pass of a row request: the row of every node outside [0, N) becomes K times -1, its count 0
__global__ void __launch_bounds__(256) k_req_rows_fixup(const int64_t *__restrict__ nodes, uint64_t m, uint64_t N, uint32_t K,
                                                        int32_t *__restrict__ out, uint32_t *__restrict__ counts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        const int64_t v = nodes[i];
        if (v >= 0 && (uint64_t)v < N) continue;
        for (uint32_t j = 0; j < K; j++) out[i * K + j] = -1;
        if (counts) counts[i] = 0;
    }
}

inline dim3 req_grid(const ::vidc_ctx *c, uint64_t n, uint32_t per_block = 256) {
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, (uint64_t)c->num_cu * 32)));
}

// the host-side argument checks every request call makes before any device work
inline int req_check_rows(const ::vidc_ctx *ctx, const void *obj, uint64_t m, const int64_t *d_nodes, const int32_t *d_out) {
    if (!ctx || !obj || (m && (!d_nodes || !d_out))) {
        set_error("rows request: NULL context, object or array");
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}
inline int req_check_labels(const ::vidc_ctx *ctx, const void *obj, uint64_t n, const int64_t *d_labels, const int64_t *d_ids) {
    if (!ctx || !obj || (n && (!d_labels || !d_ids))) {
        set_error("translate_labels: NULL context, object or array");
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}

// Rows of a request that runs on the device (compact rows, Elias-Fano arena rows, ROC's lean lane path): nodes sanitized into the
// context's request block (u64 or u32 per node, behind it m counts when the caller passed none and the decoder wants them), the
// codec's own decoder (decode(d_nodes, d_counts)), the fix-up pass.  Enqueue only.
template <typename I, typename Decode>
inline int req_rows_on_device(::vidc_ctx *ctx, uint64_t N, uint64_t m, const int64_t *d_nodes, uint32_t K, int32_t *d_out,
                              uint32_t *d_counts, uint64_t *d_invalid, bool need_counts, Decode &&decode) {
    void *blk = nullptr;
    const size_t nb = (m * sizeof(I) + 15) & ~(size_t)15;
    VIDC_TRY(req_scratch(ctx, nb + (need_counts && !d_counts ? m * 4 : 0), &blk));
    I *s_nodes = (I *)blk;
    uint32_t *cnt = d_counts ? d_counts : (need_counts ? (uint32_t *)((char *)blk + nb) : nullptr);
    hipLaunchKernelGGL(k_req_nodes_sanitize<I>, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, N, s_nodes,
                       (unsigned long long *)d_invalid);
    VIDC_HIP(hipGetLastError());
    if (N) VIDC_TRY(decode((const I *)s_nodes, cnt));  // (N == 0: no row to decode, every node is negative or invalid)
    hipLaunchKernelGGL(k_req_rows_fixup, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, N, K, d_out, d_counts);
    VIDC_HIP(hipGetLastError());
    return req_done(ctx);
}

// Rows of a request that takes the host-array path: the nodes cross PCIe once (D2H), nodes outside [0, N) become the request's first
// valid node on the host (a row that was asked for anyway: it fits K whenever the request can be served at all -- node 0 need not),
// the host-array call decodes (decode(host_nodes, host_counts)), the counts go back up, the fix-up pass rewrites the invalid rows.
// Synchronises.
template <typename Decode>
inline int req_rows_via_host(::vidc_ctx *ctx, uint64_t N, uint64_t m, const int64_t *d_nodes, uint32_t K, int32_t *d_out,
                             uint32_t *d_counts, uint64_t *d_invalid, Decode &&decode) {
    Pinned h;
    VIDC_TRY(h.get(ctx, m * 12 + 8));
    uint64_t *hn = h.as<uint64_t>();
    uint64_t &bad = hn[m];
    uint32_t *hc = (uint32_t *)(hn + m + 1);
    VIDC_HIP(hipMemcpyAsync(hn, d_nodes, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    bad = 0;
    uint64_t stand_in = ~0ull;  // the first valid node of the request
    for (uint64_t i = 0; i < m && stand_in == ~0ull; i++)
        if ((int64_t)hn[i] >= 0 && hn[i] < N) stand_in = hn[i];
    for (uint64_t i = 0; i < m; i++) {
        const int64_t v = (int64_t)hn[i];
        if (v >= 0 && (uint64_t)v >= N) bad++;
        hn[i] = v >= 0 && (uint64_t)v < N ? (uint64_t)v : stand_in;
    }
    if (stand_in != ~0ull) VIDC_TRY(decode((const uint64_t *)hn, d_counts ? hc : nullptr));  // (else: no row to decode)
    if (d_counts) VIDC_HIP(hipMemcpyAsync(d_counts, hc, m * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_req_rows_fixup, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, N, K, d_out, d_counts);
    VIDC_HIP(hipGetLastError());
    if (bad && d_invalid) {
        // (the count is added on the device, in stream order with the caller's other uses of *d_invalid)
        void *blk = nullptr;
        VIDC_TRY(req_scratch(ctx, 8, &blk));
        VIDC_HIP(hipMemcpyAsync(blk, &bad, 8, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_req_add, dim3(1), dim3(64), 0, ctx->stream, (const unsigned long long *)blk, (unsigned long long *)d_invalid);
        VIDC_HIP(hipGetLastError());
        VIDC_TRY(req_done(ctx));
    }
    VIDC_HIP(vidc_stream_wait(ctx->stream));  // (the pinned block goes back to the context's cache)
    return VIDC_OK;
}

}  // namespace
}  // namespace vidc
