// dev_offsets.h -- the entry of a device-resident offsets array (the vidc_*_encode_dev / vidc_wt_build_dev calls).
//
// k_offsets_ingest copies the caller's offsets[nlist+1] into the object's own array, validates them and reduces the per-list
// figures the host path takes from its pass over host offsets (lengths_pass): summed bytes / words / chunks of a codec, the
// longest list, the first bad list.  The last workgroup to finish (release increment, acquire by the last) writes the summary
// into pinned host memory, read by the host after the call's wait.
//
// Bad offsets (offsets[0] != 0, a decrease, offsets[nlist] != ntotal, a list over the codec's limit) never reach a later kernel:
// the last workgroup replaces the object's copy by an even split of [0, ntotal) -- a valid CSR of the same (nlist, ntotal), so
// every buffer sized from (nlist, ntotal) bounds still holds what the later kernels write -- and the call returns the error
// after its wait.  Kernels that take a count from res[] check res[DOFF_BAD] first (the counts of bad offsets are meaningless).
//
// The accumulators live in a context-owned block (doff_block): zeroed once when it is created, and cleared again by the last
// workgroup after it has copied them into the result words res[] that the call's later kernels read -- no memset per call.  Calls
// on one context are ordered (each ends with a wait), so one block serves them all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace vidc {

enum : uint32_t { DOFF_BYTES = 0, DOFF_WORDS, DOFF_CHUNKS, DOFF_MAX, DOFF_BAD, DOFF_KINDS, DOFF_COUNTER, DOFF_NACC = 8 };
enum : uint32_t { DOFF_KIND_INVALID = 1u, DOFF_KIND_LIMIT = 2u };

// 64 bytes, written by the last workgroup (pinned host memory)
struct DevOffSummary {
    uint64_t bytes;   // sum ceil(n * bits / 8)
    uint64_t words;   // sum ceil(n * bits / 64) + 1
    uint64_t chunks;  // sum ceil(n / 2^chunk_shift)
    uint64_t max_n;   // longest list
    uint64_t bad;     // 0, or ~(first bad list)
    uint64_t kinds;   // DOFF_KIND_* of every bad list
    uint64_t done;    // 1 once written
    uint64_t pad;
};
static_assert(sizeof(DevOffSummary) == 64, "one 64-byte summary");

// grid of the ingest: a workgroup of 256 threads per 2048 offsets, at most 128.  (Every workgroup ends with an agent-scope release,
// a write-back of its L2: with one workgroup per 256 offsets the ingest of 65 536 lists took ~22 us, with this grid ~11 us --
// rocprofv3 kernel traces, the second one in profiles/r07_dev_offsets_trace.txt.)
inline uint32_t doff_grid(uint64_t nlist) {
    const uint64_t g = (nlist + 1 + 2047) / 2048;
    return (uint32_t)(g < 128 ? g : 128);
}

namespace dev {

__device__ __forceinline__ uint64_t doff_wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t doff_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t x = __shfl_xor(v, o, 64);
        v = x > v ? x : v;
    }
    return v;
}

namespace {  // (one copy per translation unit that launches it)

// acc: DOFF_NACC device words, zero at the launch (and again at the end); res: DOFF_NACC words receiving the totals.
// limit: longest list the codec takes (longer: DOFF_KIND_LIMIT).
__global__ void __launch_bounds__(256) k_offsets_ingest(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint64_t nlist,
                                                        uint64_t ntotal, uint32_t chunk_shift, uint32_t bits, uint64_t limit,
                                                        unsigned long long *acc, unsigned long long *res, DevOffSummary *out) {
    __shared__ uint64_t red[4][4];
    __shared__ uint32_t last_s;
    __shared__ uint64_t bad_s;
    const uint32_t t = threadIdx.x;
    uint64_t s_bytes = 0, s_words = 0, s_chunks = 0, s_max = 0, bad_key = ~0ull;
    uint32_t kinds = 0;
    const uint64_t cmask = (1ull << chunk_shift) - 1ull;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + t; i <= nlist; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t a = src[i];
        dst[i] = a;
        uint32_t k = 0;
        uint64_t list = i;
        if (i == 0 && a != 0) k |= DOFF_KIND_INVALID;
        if (i < nlist) {
            const uint64_t b = src[i + 1];
            const uint64_t n = b - a;
            if (b < a) k |= DOFF_KIND_INVALID;
            else {
                if (n > limit) k |= DOFF_KIND_LIMIT;
                s_bytes += (n * bits + 7) >> 3;
                s_words += ((n * bits + 63) >> 6) + 1;
                s_chunks += (n + cmask) >> chunk_shift;
                s_max = n > s_max ? n : s_max;
            }
        } else {  // i == nlist: the total
            if (a != ntotal) k |= DOFF_KIND_INVALID;
            list = nlist ? nlist - 1 : 0;
        }
        if (k) {
            kinds |= k;
            bad_key = list < bad_key ? list : bad_key;
        }
    }
    const uint32_t w = t >> 6;
    s_bytes = doff_wave_sum(s_bytes);
    s_words = doff_wave_sum(s_words);
    s_chunks = doff_wave_sum(s_chunks);
    s_max = doff_wave_max(s_max);
    if ((t & 63u) == 0) { red[w][0] = s_bytes; red[w][1] = s_words; red[w][2] = s_chunks; red[w][3] = s_max; }
    if (kinds) {  // (rare: bad offsets)
        atomicOr(&acc[DOFF_KINDS], (unsigned long long)kinds);
        atomicMax(&acc[DOFF_BAD], (unsigned long long)~bad_key);
    }
    __syncthreads();
    if (t == 0) {
        uint64_t b = 0, wd = 0, c = 0, m = 0;
        for (int j = 0; j < 4; j++) {
            b += red[j][0]; wd += red[j][1]; c += red[j][2];
            m = red[j][3] > m ? red[j][3] : m;
        }
        atomicAdd(&acc[DOFF_BYTES], (unsigned long long)b);
        atomicAdd(&acc[DOFF_WORDS], (unsigned long long)wd);
        atomicAdd(&acc[DOFF_CHUNKS], (unsigned long long)c);
        atomicMax(&acc[DOFF_MAX], (unsigned long long)m);
    }
    __syncthreads();  // (the bad-list atomics of every thread are ahead of thread 0's release below)
    if (t == 0) {
        const unsigned long long prev =
            __hip_atomic_fetch_add(&acc[DOFF_COUNTER], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = prev == (unsigned long long)gridDim.x - 1ull;
        last_s = last ? 1u : 0u;
        if (last) {
            DevOffSummary s;
            s.bytes = __hip_atomic_load(&acc[DOFF_BYTES], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.words = __hip_atomic_load(&acc[DOFF_WORDS], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.chunks = __hip_atomic_load(&acc[DOFF_CHUNKS], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.max_n = __hip_atomic_load(&acc[DOFF_MAX], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.bad = __hip_atomic_load(&acc[DOFF_BAD], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.kinds = __hip_atomic_load(&acc[DOFF_KINDS], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            s.done = 1;
            s.pad = 0;
            bad_s = s.bad;
            *out = s;
            res[DOFF_BYTES] = s.bytes; res[DOFF_WORDS] = s.words; res[DOFF_CHUNKS] = s.chunks; res[DOFF_MAX] = s.max_n;
            res[DOFF_BAD] = s.bad; res[DOFF_KINDS] = s.kinds;
            for (int j = 0; j < (int)DOFF_NACC; j++) __hip_atomic_store(&acc[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            bad_s = 0;
        }
    }
    __syncthreads();
    if (last_s && bad_s) {  // even split: offsets[i] = min(i * ceil(ntotal / nlist), ntotal), offsets[nlist] = ntotal
        const uint64_t q = nlist ? (ntotal + nlist - 1) / nlist : 0;
        for (uint64_t i = t; i <= nlist; i += 256u) {
            const uint64_t v = i == nlist ? ntotal : (i * q < ntotal ? i * q : ntotal);
            __hip_atomic_store(&dst[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

}  // namespace dev

// the context's accumulator block: [DOFF_NACC accumulators | DOFF_NACC results], created (and zeroed) on first use
inline int doff_block(::vidc_ctx *ctx, unsigned long long **acc) {
    if (!ctx->d_doff) {
        unsigned long long *p = nullptr;
        VIDC_HIP(hipMalloc((void **)&p, 2 * DOFF_NACC * 8));
        if (hipMemset(p, 0, 2 * DOFF_NACC * 8) != hipSuccess) { (void)hipFree(p); set_error("doff_block: memset failed"); return VIDC_ERR_HIP; }
        ctx->d_doff = p;
    }
    *acc = ctx->d_doff;
    return VIDC_OK;
}

// the status of a summary (VIDC_OK for good offsets), with a message that names the first bad list.  limit_status: what a list
// over the codec's limit returns (the host path's code for it).
inline int doff_status(const DevOffSummary &s, const char *codec, int limit_status) {
    if (!s.bad) return VIDC_OK;
    const unsigned long long l = (unsigned long long)~s.bad;
    if (s.kinds & DOFF_KIND_INVALID) {
        set_error("%s: bad device offsets at list %llu (offsets[0] must be 0, offsets monotone, offsets[nlist] == ntotal)", codec, l);
        return VIDC_ERR_INVALID;
    }
    set_error("%s: list %llu is longer than the codec takes", codec, l);
    return limit_status;
}

}  // namespace vidc
