// ivf_merge.h -- the S-way merge of a cut IVF scan (ivf_scan.hip: k_ivf_scan, ivf_residual.hip: k_ivf_scan_residual): the kernel both
// translation units launch behind their scan when a probe row was cut into S > 1 pieces.  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_scan_ref.h"
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
}  // namespace vidc
