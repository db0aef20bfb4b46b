// ivf_probe_select.h -- one trip of the selection of vidc_ivf_probe_dev: up to 64 keys, one per lane, into a sorted pool of k keys in
// LDS.  The step is that of the scan kernels (drop by ballot, insert by rank), whose workgroup-barrier form is ivf_insert_trip
// (csrc/ivf_scan_steps.h), and the rules are those of csrc/ivf_scan_ref.h: key_dropped, lower_bound, place_kept.  k_ivf_probe runs
// it over the distance tile of a query, k_ivf_probe_merge over the S runs of one.
// Device only.  The caller's wavefront owns pool, other and ckey; nothing here meets another wavefront, so the LDS is ordered by
// wave_lds_sync and the function may be called where the wavefronts of a workgroup have diverged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_scan_ref.h"
#include "wave.h"

namespace vidc {
namespace dev {

// key: this lane's candidate, or ivs::EMPTY.  The keys of a query are distinct (a key ends in its list number).  pool: k ascending
// keys, EMPTY padded; other: k keys of room; ckey: 64 keys of room.  -> true: the union's first k keys are in `other` now (the
// caller swaps the two); false: every key was dropped.  Every loop has a wavefront-uniform trip count.
__device__ __forceinline__ bool probe_select_trip(uint64_t key, const uint64_t *pool, uint64_t *other, uint64_t *ckey, uint32_t k, uint32_t lane) {
    const bool keep = key != ivs::EMPTY && !ivs::key_dropped(key, pool[k - 1u]);
    const uint64_t keepm = __ballot(keep);
    const uint32_t C = popc64(keepm);
    if (C == 0) return false;
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
    uint32_t below = 0;
    for (uint64_t m = keepm; m; m &= m - 1ull) below += ivs::key_less(rl64(klo, khi, ff1(m)), key) ? 1u : 0u;
    uint32_t pb = 0;
    if (keep) {
        ckey[below] = key;  // the survivors in ascending order
        pb = ivs::lower_bound(pool, k, key);
    }
    wave_lds_sync();
    for (uint32_t t = 0; t < k; t += 64) {
        const uint32_t i = t + lane;
        if (i < k) {
            const uint64_t pk = pool[i];
            const uint32_t place = i + ivs::lower_bound(ckey, C, pk);
            if (ivs::place_kept(place, k)) other[place] = pk;
        }
    }
    if (keep && ivs::place_kept(pb + below, k)) other[pb + below] = key;
    wave_lds_sync();
    return true;
}

}  // namespace dev
}  // namespace vidc
