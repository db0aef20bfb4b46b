// ivf_merge.h -- the S-way merge of a cut IVF scan (ivf_scan.hip, ivf_residual.hip, ivf_pqbits.hip, ivf_aq.hip): the kernel every
// scan unit launches behind its scan when a probe row was cut into S > 1 pieces, and the host tail those units share: the carve of
// the run scratch, the LDS cap of a launch, the scan's launch with the merge behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "ivf_scan_plan.h"
#include "ivf_scan_ref.h"
#include "requests.h"
#include "wave.h"

namespace vidc {
namespace dev {

// a wavefront per query: the S sorted runs of its pieces -> D, labels, stats.  A key's place is its index in its own run plus the
// keys below it in every other run (keys of a query are distinct); the places behind the last key are padded.
static __global__ void __launch_bounds__(64) k_ivf_merge(const uint64_t *__restrict__ runs, const uint32_t *__restrict__ run_stats, uint64_t nq,
                                                         uint32_t S, uint32_t k, const uint64_t *__restrict__ off, uint64_t nlist,
                                                         float *__restrict__ D, int64_t *__restrict__ labels, uint32_t *__restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint64_t r[];  // S * k keys
    const uint32_t lane = lane_id(), n = S * k;
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        for (uint32_t e = lane; e < n; e += 64) r[e] = runs[q * n + e];
        __syncthreads();
        uint32_t total = 0;
        for (uint32_t s = 0; s < S; s++) total += ivs::lower_bound(r + s * k, k, ivs::EMPTY);
        total = total < k ? total : k;
        for (uint32_t e = lane; e < n; e += 64) {
            const uint64_t key = r[e];
            if (key == ivs::EMPTY) continue;
            const uint32_t place = ivs::merge_place(r, S, k, e / k, e % k);
            if (ivs::place_kept(place, k)) {
                D[q * k + place] = ivs::key_dist(key);
                labels[q * k + place] = ivs::key_label(off, nlist, key);
            }
        }
        for (uint32_t i = total + lane; i < k; i += 64) {
            D[q * k + i] = __builtin_inff();
            labels[q * k + i] = -1;
        }
        if (stats && lane == 0) {
            uint32_t nl = 0, nc = 0;
            for (uint32_t s = 0; s < S; s++) {
                nl += run_stats[(q * S + s) * 2];
                nc += run_stats[(q * S + s) * 2 + 1];
            }
            stats[q * 2] = nl;
            stats[q * 2 + 1] = nc;
        }
        __syncthreads();  // (the next query rewrites the runs)
    }
}

}  // namespace dev

// The host tail of a scan entry point.  A: the kernel's argument struct, whose nlist, off, nq, S, k, runs, run_stats, D, labels and
// stats carry those names in every unit; P: the unit's plan (nslots, lds, S, merge_lds).

// the runs of a cut call and their counters, carved out of one scratch block: [nq, S, k] keys, then [nq, S, 2] counters
template <typename A>
void ivf_carve_runs(A &a, const Scratch &s, uint64_t nq, uint32_t S, uint32_t k) {
    a.runs = S > 1 ? s.as<uint64_t>() : nullptr;
    a.run_stats = S > 1 ? (uint32_t *)(s.as<uint64_t>() + ivs::scratch_keys(nq, S, k)) : nullptr;
}

// dynamic LDS above the default cap of a launch (tables of about 48 sub-quantisers and more, long probe rows): raised per kernel
template <typename A>
int ivf_lds_cap(void (*fn)(A), size_t lds) {
    if (lds > 64u * 1024u) VIDC_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return VIDC_OK;
}

// the scan kernel, a wavefront per slot, and behind it the merge of a cut call, both on the context's stream
template <typename A, typename P>
int ivf_launch_scan(vidc_ctx *ctx, void (*fn)(A), const P &p, const A &a) {
    hipLaunchKernelGGL(fn, dim3(p.nslots), dim3(64), p.lds, ctx->stream, a);
    VIDC_HIP(hipGetLastError());
    if (p.S > 1) {
        hipLaunchKernelGGL(dev::k_ivf_merge, req_grid(ctx, a.nq, 1), dim3(64), p.merge_lds, ctx->stream, (const uint64_t *)a.runs,
                           (const uint32_t *)a.run_stats, a.nq, p.S, a.k, a.off, a.nlist, a.D, a.labels, a.stats);
        VIDC_HIP(hipGetLastError());
    }
    return VIDC_OK;
}

}  // namespace vidc
