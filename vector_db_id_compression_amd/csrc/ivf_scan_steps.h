// ivf_scan_steps.h -- the three steps every IVF list kernel takes in the same words (ivf_scan.hip, ivf_range.hip, ivf_residual.hip,
// ivf_pqbits.hip, ivf_aq.hip): the head of an item, the insert of a trip's survivors, the result write of an item.  Device only, one
// wavefront per workgroup.  The rules they apply (probe row, drop test, insert by rank, label of a position) are
// csrc/ivf_scan_ref.h; the duplicate rule over the whole row, the strict drop test and "labels decide ties" are what make a result
// independent of the cut S, and they are stated here once.  Nothing here knows which code kind it serves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ivf_scan_ref.h"
#include "wave.h"

namespace vidc {
namespace dev {

// the head of an item: the query vector (d floats) and the probe row (nprobe entries) of query q go to LDS; the row is mapped to
// list numbers (-1: no list) and de-duplicated in place over the WHOLE row, 64 entries a pass: lane j compares its entry with every
// entry in front of it (uniform trip count), and a pass clears the later mentions among its 64 entries, so every pass behind it
// still finds the first one.  The piece of a cut item is taken afterwards.  Ends behind a barrier.
__device__ __forceinline__ void ivf_item_head(const float *xq, const int64_t *probes, uint64_t nlist, uint64_t q, uint32_t d, uint32_t nprobe,
                                              uint32_t lane, float *qv, int32_t *row) {
    for (uint32_t i = lane; i < d; i += 64) qv[i] = xq[q * d + i];
    for (uint32_t j = lane; j < nprobe; j += 64) row[j] = ivs::probe_list(probes[q * nprobe + j], nlist);
    __syncthreads();
    for (uint32_t j0 = 0; j0 < nprobe; j0 += 64) {
        const uint32_t j = j0 + lane, end = j0 + 64u < nprobe ? j0 + 64u : nprobe;
        const int32_t mine = j < nprobe ? row[j] : -1;
        bool dup = false;
        for (uint32_t i = 0; i < end; i++) dup = dup || (i < j && row[i] == mine);
        __syncthreads();
        if (dup && mine >= 0) row[j] = -1;
        __syncthreads();
    }
}

// the insert of a trip: key is this lane's candidate where valid.  pool: k ascending keys, EMPTY padded; other: k keys of room;
// ckey: 64 keys of room.  A candidate whose key is not below the pool's last key is dropped by a ballot; the survivors are ranked
// among themselves by lane reads, against the pool by binary search, and every element is stored at its place in `other`.
// -> true: the first k keys of the union are being written to `other`: the caller swaps the two and closes the trip with a barrier
// before anything reads the pool; false: every key was dropped, nothing was written and no barrier was passed.
// ivf_probe_select.h holds the same step for wavefronts that have diverged (wave_lds_sync).
__device__ __forceinline__ bool ivf_insert_trip(uint64_t key, bool valid, const uint64_t *pool, uint64_t *other, uint64_t *ckey, uint32_t k,
                                                uint32_t lane) {
    const bool keep = valid && !ivs::key_dropped(key, pool[k - 1u]);
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
    __syncthreads();
    for (uint32_t t = 0; t < k; t += 64) {
        const uint32_t i = t + lane;
        if (i < k) {
            const uint64_t pk = pool[i];
            const uint32_t place = i + ivs::lower_bound(ckey, C, pk);
            if (ivs::place_kept(place, k)) other[place] = pk;
        }
    }
    if (keep && ivs::place_kept(pb + below, k)) other[pb + below] = key;
    return true;
}

// the result write of an item (query q, item = q * S + piece) from its pool of k keys.  S == 1: the wavefront writes D, the labels
// and the two counters of stats (NULL: none) itself.  S > 1: its k keys and two counters go to the run of the item, which
// k_ivf_merge (ivf_merge.h) reads.  No barrier: the caller's closing one stands behind it.
__device__ __forceinline__ void ivf_write_item(const uint64_t *pool, uint32_t k, uint32_t lane, uint64_t q, uint64_t item, uint32_t S,
                                               const uint64_t *off, uint64_t nlist, uint32_t nlists, uint32_t ncodes, float *D, int64_t *labels,
                                               uint32_t *stats, uint64_t *runs, uint32_t *run_stats) {
    if (S == 1) {
        for (uint32_t i = lane; i < k; i += 64) {
            const uint64_t ki = pool[i];
            D[q * k + i] = ki == ivs::EMPTY ? __builtin_inff() : ivs::key_dist(ki);
            labels[q * k + i] = ki == ivs::EMPTY ? -1 : ivs::key_label(off, nlist, ki);
        }
        if (stats && lane == 0) {
            stats[q * 2] = nlists;
            stats[q * 2 + 1] = ncodes;
        }
    } else {
        for (uint32_t i = lane; i < k; i += 64) runs[item * k + i] = pool[i];
        if (lane == 0) {
            run_stats[item * 2] = nlists;
            run_stats[item * 2 + 1] = ncodes;
        }
    }
}

}  // namespace dev
}  // namespace vidc
