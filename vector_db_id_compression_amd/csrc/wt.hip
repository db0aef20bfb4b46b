// wt.hip -- wavelet tree over the sequence list_nos[id] (CompressedIDInvertedListsWaveletTree,
// custom_invlists_impl.cpp:346-397): id = select(offset + 1, list_no)  (:377-379).
//
// The reference delegates to sdsl::wt_int (not in the reference tree, "parity unpinned" for its size and
// internal layout); what is reproduced here is the data structure itself and the select semantics:
//   L = max(1, bit_width(nlist - 1)) levels; level l holds one bit per id (bit L-1-l of the symbol) in the order
//   obtained by stable-sorting the ids by the top l bits of their symbol (pointerless / levelwise layout);
//   every level has a rank directory (ones before each 512-bit block).
// select walks the levels bottom-up with one rank and one select per level.  Everything is built and
// queried on the GPU: thread-per-word bit gathering, a workgroup scan for the rank directory, and a
// rank-driven stable partition to derive the next level's order.
//
// wt_type = 1 (sdsl::wt_int<rrr_vector<63>>, custom_invlists_impl.h:104-113): every level is stored RRR-coded and the
// plain bits are dropped after the build -- 63-bit blocks, each a 6-bit class (its popcount c) and a
// ceil(log2 C(63, c))-bit offset (the block's index among the 63-bit words with c ones, combinatorial number
// system), plus one (offset-stream pointer, ones-before) sample per 32 blocks.  rank / access decode ONE block
// (sample -> add the classes of the blocks before it -> unrank the offset); select is a binary search over the
// samples, a scan over <= 32 classes and one block decode.  The bit order inside sdsl's structure is not pinned
// (sdsl is absent here); the structure, its parameters (block 63, sample rate 32) and what it answers are.
#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>

#include "append.h"
#include "merge.h"
#include "bits.h"
#include "common.h"
#include "dev_offsets.h"
#include "host_call.h"
#include "requests.h"
#include "scan.h"
#include "wt_plan.h"

using namespace vidc;
using namespace vidc::dev;

struct vidc_wt {
    int device = 0;
    uint64_t ntotal = 0, nlist = 0;
    uint32_t L = 0;
    int wt_type = 0;
    uint64_t words_per_level = 0, blocks_per_level = 0;
    uint64_t size_bytes = 0;
    mutable std::vector<uint64_t> offsets;  // host copy of the symbol start positions C[s]: for objects built from device offsets
    mutable bool offsets_host = true;       // filled on first use (wt_ensure_offsets, under mu)
    mutable std::mutex mu;
    DevBuf<uint64_t> d_bits;            // L * words_per_level                      (wt_type 0)
    DevBuf<uint32_t> d_rank;            // L * (blocks_per_level + 1): ones before each 512-bit block
    DevBuf<uint64_t> d_C;               // nlist + 1
    // wt_type 1: RRR-63 levels
    uint64_t rrr_nblk = 0, rrr_nsamp = 0, rrr_cls_wpl = 0;
    std::vector<uint64_t> rrr_off_base;  // [L + 1] first word of every level's offset stream
    std::vector<uint64_t> rrr_off_bits;  // [L] bits of every level's offset stream (host only: the image's off_bits)
    DevBuf<uint32_t> d_cls;             // L * rrr_cls_wpl: packed 6-bit classes
    DevBuf<uint64_t> d_offs;            // offset streams, level after level
    DevBuf<uint32_t> d_ptr, d_rs;       // L * (rrr_nsamp + 1): bit position in the offset stream / ones before block 32 s
    // Query acceleration (both types; like the batch records of an Elias-Fano object it is not part of the reported size):
    // ones before the start of every node of every level -- level l has 2^l nodes, entry (l, p) at wt_nrank_base(l) + p,
    // entry (l, 2^l) = the level's total --, what every step of a select / decode walk asked the level's rank structure for.
    DevBuf<uint32_t> d_nrank;
    // two entries per node of every level (k_wt_node_ranks_from_C): what the build and the bulk decode add an element's rank to
    DevBuf<uint32_t> d_dstab;
    DevBuf<uint64_t> d_binom;           // C(n, k), n, k < 64 (row n at 64 n); behind it (d_binom + 4096) the 64 offset widths as bytes
};

namespace {

// list_nos[id] = list number; validates the reference's asserts (ids ascending inside a list, < ntotal).
// A workgroup takes 4096 consecutive positions: two searches of the whole offset table find the lists of its first and last position,
// every position then searches only between them; the symbol goes out with a plain store and k_wt_check_syms looks for slots nobody
// wrote (ntotal ids below ntotal without a gap are a permutation).  Round 5: a 16-step search per id and an atomic exchange per
// id -- 0.69 ms for 16.8 M ids.
__global__ void __launch_bounds__(256) k_wt_scatter_syms(const uint64_t *__restrict__ ids, const uint64_t *__restrict__ offsets, uint32_t nlist,
                                                         uint64_t ntotal, uint32_t *__restrict__ syms, uint32_t *err) {
    __shared__ uint32_t lo_s, hi_s;
    bool bad = false;
    for (uint64_t base = (uint64_t)blockIdx.x * 4096u; base < ntotal; base += (uint64_t)gridDim.x * 4096u) {
        const uint64_t end = base + 4096u < ntotal ? base + 4096u : ntotal;
        if (threadIdx.x == 0) lo_s = find_list(offsets, nlist, base);
        if (threadIdx.x == 64) hi_s = find_list(offsets, nlist, end - 1);
        __syncthreads();
        const uint32_t llo = lo_s, lhi = hi_s;
        for (uint64_t g = base + threadIdx.x; g < end; g += 256u) {
            uint32_t lo = llo, hi = lhi + 1u;  // invariant: offsets[lo] <= g < offsets[hi]
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (offsets[mid] <= g) lo = mid; else hi = mid;
            }
            const uint64_t id = ids[g];
            bool b = id >= ntotal;
            if (g > offsets[lo]) b |= ids[g - 1] >= id;  // assert(ids_data[i] > prev_id), :359
            if (!b) syms[id] = lo;
            bad |= b;
        }
        __syncthreads();
    }
    if (bad) atomicOr(err, 1u);
}
// a slot nobody wrote = an id that is missing = another one present twice
__global__ void k_wt_check_syms(const uint32_t *syms, uint64_t ntotal, uint32_t *err) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ntotal; i += (uint64_t)gridDim.x * blockDim.x) bad |= syms[i] == 0xffffffffu;
    if (bad) atomicOr(err, 2u);
}

// ---- the same in two streaming passes (round 6, second half; 2^18 <= ntotal <= 2^24 ids, <= 2^18 lists).  The direct scatter writes 4 bytes
// at 16.8 M random places: 32-byte partial writes, 0.48 ms at 92 % of its wavefronts' cycles waiting (profiles/r06_pmc_wt.json).  Here the
// (id, list) pairs are first PARTITIONED by id >> 14 into <= 1024 buckets -- 256 workgroups over consecutive positions, per-workgroup
// histograms, no global atomic (rule 3) -- as one packed dword each (14 low id bits | list number; the list of a position from the list starts marked in a tile's LDS image and a scan,
// not from a search per position), then one workgroup
// per bucket places its pairs in a 64 KiB LDS image of the bucket's 16 384 ids and writes the image out with 16-byte stores; a slot nobody
// wrote is found on the way (k_wt_check_syms and the 0xff fill of the array are not needed).
// (VIDC_WTP_*, wtp_chunk: wt_plan.h)
__global__ void __launch_bounds__(256) k_wt_part_hist(const uint64_t *__restrict__ ids, uint64_t ntotal, uint32_t *__restrict__ part) {
    __shared__ uint32_t h[VIDC_WTP_MAXB];
    for (uint32_t k = threadIdx.x; k < VIDC_WTP_MAXB; k += 256u) h[k] = 0u;
    __syncthreads();
    const uint64_t chunk = wtp_chunk(ntotal), lo = blockIdx.x * chunk, hi = lo + chunk < ntotal ? lo + chunk : ntotal;
    for (uint64_t g0 = lo; g0 < hi; g0 += 1024u) {
        uint64_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t g = g0 + (uint32_t)j * 256u + threadIdx.x;
            v[j] = g < hi ? ids[g] : ~0ull;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (v[j] < ntotal) atomicAdd(&h[v[j] >> VIDC_WTP_BSH], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < VIDC_WTP_MAXB; k += 256u) part[blockIdx.x * VIDC_WTP_MAXB + k] = h[k];
}
// thread = bucket: its per-workgroup counts 128 at a time in registers -> exclusive prefix over the workgroups in place, the bucket's total to tot
// (64 threads per workgroup: 2048 memory instructions per wavefront go through ONE CU's address unit, so sixteen CUs share them)
__global__ void __launch_bounds__(64) k_wt_part_scan(uint32_t *part, uint32_t *tot) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < VIDC_WTP_NBLK; b0 += 128u) {
        uint32_t c[128];
#pragma unroll
        for (uint32_t b = 0; b < 128u; b++) c[b] = part[(b0 + b) * VIDC_WTP_MAXB + k];
        asm volatile("" ::: "memory");  // (all 128 loads in flight before the first add: scheduled in groups of ~32 they were 32 round trips)
#pragma unroll
        for (uint32_t b = 0; b < 128u; b++) {
            const uint32_t t = c[b];
            c[b] = run;
            run += t;
        }
#pragma unroll
        for (uint32_t b = 0; b < 128u; b++) part[(b0 + b) * VIDC_WTP_MAXB + k] = c[b];
    }
    tot[k] = run;
}
__global__ void __launch_bounds__(256) k_wt_part_scatter(const uint64_t *__restrict__ ids, const uint64_t *__restrict__ offsets, uint32_t nlist,
                                                         uint64_t ntotal, const uint32_t *__restrict__ part, const uint32_t *__restrict__ tot,
                                                         uint32_t *__restrict__ bstart, uint32_t *__restrict__ pairs, uint32_t *err) {
    __shared__ uint32_t cur[VIDC_WTP_MAXB];
    __shared__ uint32_t tsum[256];
    __shared__ uint32_t lidx[4096 + 256];       // per position of a tile: list starts marked, then the number of the position's list
    __shared__ uint32_t lo_s, hi_s;
    uint32_t bs4[4];  // starts of this thread's four buckets
    {   // bucket starts = exclusive scan of the 1024 totals: four per thread + a scan over the threads
        uint32_t t4[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { t4[j] = tot[threadIdx.x * 4u + (uint32_t)j]; s += t4[j]; }
        tsum[threadIdx.x] = s;
        __syncthreads();
        for (uint32_t o = 1; o < 256u; o <<= 1) {
            const uint32_t v = threadIdx.x >= o ? tsum[threadIdx.x - o] : 0u;
            __syncthreads();
            tsum[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t run = tsum[threadIdx.x] - s;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t k = threadIdx.x * 4u + (uint32_t)j;
            bs4[j] = run;
            if (blockIdx.x == 0) bstart[k] = run;
            run += t4[j];
        }
        if (blockIdx.x == 0 && threadIdx.x == 255u) bstart[VIDC_WTP_MAXB] = run;
    }
    bool bad = false;
    // chunks blockIdx.x, blockIdx.x + gridDim.x, ... (the launch has one workgroup per chunk; fewer, each walking several chunks -- so that
    // fewer of the 64-byte bucket runs are open at once and their lines fill up in the L2 -- measured no faster: 143 / 221 us with 512 / 256)
    for (uint32_t cb = blockIdx.x; cb < VIDC_WTP_NBLK; cb += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t k = threadIdx.x * 4u + (uint32_t)j;
        cur[k] = bs4[j] + part[cb * VIDC_WTP_MAXB + k];
    }
    __syncthreads();
    const uint64_t chunk = wtp_chunk(ntotal), c_lo = cb * chunk, c_hi = c_lo + chunk < ntotal ? c_lo + chunk : ntotal;
    for (uint64_t base = c_lo; base < c_hi; base += 4096u) {
        const uint64_t end = base + 4096u < c_hi ? base + 4096u : c_hi;
        // the tile's 16 ids per thread (and the id in front of each: the order check) are requested before anything waits
        uint64_t idv[16], prv[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t g = base + (uint32_t)j * 256u + threadIdx.x;
            idv[j] = g < end ? ids[g] : ~0ull;
            prv[j] = (g < end && g) ? ids[g - 1] : 0ull;
        }
        if (threadIdx.x == 0) lo_s = find_list(offsets, nlist, base);
        if (threadIdx.x == 64) hi_s = find_list(offsets, nlist, end - 1);
#pragma unroll
        for (int j = 0; j < 17; j++) lidx[(uint32_t)j * 256u + threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t llo = lo_s, lhi = hi_s, nl = lhi - llo + 1u;  // lists llo .. lhi
        const bool first_starts = offsets[llo] == base;  // (the tile's first position opens list llo: no id in front of it to compare with)
        // list of a position = llo + the number of lists llo + 1 .. lhi that start at or in front of it: every such list marks its start
        // (all of them lie inside the tile), a scan over the tile's 4096 positions does the rest -- no search per position (a binary search
        // in LDS per position, a chain of dependent reads sixteen times in a row per thread, was most of this kernel's 0.2 ms)
        for (uint32_t k = 1u + threadIdx.x; k < nl; k += 256u) {
            const uint32_t rel = (uint32_t)(offsets[llo + k] - base);
            atomicAdd(&lidx[rel + (rel >> 4)], 1u);  // (entry p at p + p / 16: thread t's sixteen entries of the scan below are conflict-free)
        }
        __syncthreads();
        {
            uint32_t f[16], sum = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) { f[j] = lidx[threadIdx.x * 17u + (uint32_t)j]; sum += f[j]; }
            uint32_t incl = sum;
            const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= (uint32_t)o) incl += u;
            }
            if (lane == 63u) tsum[wave] = incl;
            __syncthreads();
            uint32_t run = incl - sum;
            for (uint32_t w2 = 0; w2 < wave; w2++) run += tsum[w2];
#pragma unroll
            for (int j = 0; j < 16; j++) {
                run += f[j];
                lidx[threadIdx.x * 17u + (uint32_t)j] = run | (f[j] ? 0x80000000u : 0u);  // bit 31: a list starts here
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t rel = (uint32_t)j * 256u + threadIdx.x;
            const uint64_t g = base + rel;
            if (g >= end) continue;
            const uint32_t v = lidx[rel + (rel >> 4)];
            const uint64_t id = idv[j];
            if (id < ntotal) {  // (counted by k_wt_part_hist: takes its slot whatever else is wrong with it)
                if (!(v >> 31) && !(rel == 0u && first_starts)) bad |= prv[j] >= id;  // assert(ids_data[i] > prev_id), :359 (not for the first id of a list)
                const uint32_t slot = atomicAdd(&cur[id >> VIDC_WTP_BSH], 1u);
                pairs[slot] = ((uint32_t)id & (VIDC_WTP_BUCKET - 1u)) | ((llo + (v & 0x7fffffffu)) << VIDC_WTP_BSH);
            } else {
                bad = true;
            }
        }
        __syncthreads();
    }
    }
    if (bad) atomicOr(err, 1u);
}
__global__ void __launch_bounds__(256) k_wt_part_place(const uint32_t *__restrict__ pairs, const uint32_t *__restrict__ bstart, uint64_t ntotal,
                                                       uint32_t *__restrict__ syms, uint32_t *err) {
    extern __shared__ __attribute__((aligned(16))) uint32_t img[];  // VIDC_WTP_BUCKET dwords
    for (uint32_t i = threadIdx.x; i < VIDC_WTP_BUCKET / 4u; i += 256u) ((uint4 *)img)[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    __syncthreads();
    const uint32_t j0 = bstart[blockIdx.x], j1 = bstart[blockIdx.x + 1u];
    for (uint32_t j = j0 + threadIdx.x; j < j1; j += 1024u) {
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = j + (uint32_t)q * 256u < j1 ? pairs[j + (uint32_t)q * 256u] : ~0u;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (j + (uint32_t)q * 256u < j1) img[v[q] & (VIDC_WTP_BUCKET - 1u)] = v[q] >> VIDC_WTP_BSH;
    }
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x << VIDC_WTP_BSH;
    const uint32_t cnt = ntotal - first < VIDC_WTP_BUCKET ? (uint32_t)(ntotal - first) : VIDC_WTP_BUCKET;
    bool bad = false;
    for (uint32_t i = threadIdx.x * 4u; i < cnt; i += 1024u) {
        const uint4 v = *(const uint4 *)(img + i);
        if (i + 4u <= cnt) {
            bad |= v.x == ~0u || v.y == ~0u || v.z == ~0u || v.w == ~0u;
            *(uint4 *)(syms + first + i) = v;  // (the array and the bucket's first id are 16-byte aligned)
        } else {
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
            for (uint32_t q = 0; i + q < cnt; q++) { bad |= e[q] == ~0u; syms[first + i + q] = e[q]; }
        }
    }
    if (bad) atomicOr(err, 2u);  // a slot nobody wrote = an id that is missing = another one present twice
}

// ---- one level of the tree in ONE pass over its symbols (round 6).  Before: four launches per level -- a thread per 64-bit word gathering 64
// symbols 4 bytes at a time, a SINGLE workgroup scanning the whole rank directory, a node-rank kernel, and a partition whose every element
// asked the fresh rank directory three times -- 0.4 ms per level on 16.8 M ids, 6.4 ms for the 16 levels of a 65 536-list tree.
// Now a tile of 4096 consecutive positions per workgroup: the symbols come in coalesced, a wavefront's ballot IS the bit-vector word of its
// 64 positions, the ones before the tile come from a chained scan over the tiles (decoupled look-back: a tile publishes its own count, then
// its inclusive prefix; a successor adds counts until it meets a prefix; tiles take their numbers from a counter in start order, so every
// wait ends), and an element's slot in the next level follows from its rank and from tables that need only the symbol start table C: the
// ones before every node start (k_wt_node_ranks_from_C, all levels in one launch before the first pass).
// (VIDC_WT_EPT elements per thread, tiles of VIDC_WT_TILE positions: wt_plan.h)
struct WtScanState {  // per tile: bit 63 = inclusive prefix, bit 62 = the tile's own count; 0 = nothing yet.  [ntiles] | ticket
    unsigned long long v;
};
// nrank[(level, p)] = ones before the start of node p of the level (p = 0 .. 2^level; entry 2^level = the level's ones): the elements of the
// right children of the nodes before p, i.e. sums of symbol counts.  One workgroup per level.
// dstab[2 (level, p) + b] (build only): what an element of node p with bit b adds its zero-rank / one-rank to for its slot in the next level:
// slot = b ? (node start + zeros of the node - ones before the node) + ones before the element
//          : (ones before the node) + zeros before the element        -- ONE table entry per element instead of four (two C, two nrank).
// VIDC_WT_NR_G workgroups per level: workgroup g owns a run of nodes, adds up the right children of every node in FRONT of its run itself
// (coalesced, independent loads: redundant work, 128 loads per thread at most for a 65 536-list tree) and then scans its run 256 nodes
// per trip.  One workgroup per level -- 64 trips for the last level, or a run of 128 nodes per thread with every access 2 KiB from its
// neighbour's -- kept the whole last level on ONE CU's address unit: 92-98 us whatever the loop looked like.
__global__ void __launch_bounds__(256) k_wt_node_ranks_from_C(const uint64_t *__restrict__ C, uint32_t nlist, uint32_t L, uint32_t *__restrict__ nrank,
                                                              uint32_t *__restrict__ dstab) {
    __shared__ uint64_t wsum[4];
    const uint32_t level = blockIdx.x / VIDC_WT_NR_G, g = blockIdx.x % VIDC_WT_NR_G, shn = L - level;  // a node of this level spans 2^shn symbols
    uint32_t *out = nrank + wt_nrank_base(level);
    uint32_t *dst = dstab + 2 * wt_nrank_base(level);
    const uint64_t nodes = 1ull << level;
    const uint64_t B = ((nodes + VIDC_WT_NR_G - 1u) / VIDC_WT_NR_G + 255u) & ~255ull;
    const uint64_t first = g * B, last = first + B < nodes ? first + B : nodes;
    if (first >= nodes) return;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    auto csym = [&](uint64_t sym) -> uint64_t { return C[sym > nlist ? nlist : sym]; };
    auto block_sum = [&](uint64_t v) -> uint64_t {  // every thread gets the sum over the workgroup
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if (lane == 0) wsum[wave] = v;
        __syncthreads();
        return wsum[0] + wsum[1] + wsum[2] + wsum[3];
    };
    uint64_t acc = 0;  // right children of the nodes in front of the run
    for (uint64_t q0 = 0; q0 < first; q0 += 1024u) {
        uint64_t m[4], h[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t q = q0 + (uint32_t)j * 256u + t;
            m[j] = q < first ? csym((2 * q + 1) << (shn - 1)) : 0;
            h[j] = q < first ? csym((2 * q + 2) << (shn - 1)) : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) acc += h[j] - m[j];
    }
    uint64_t carry = block_sum(acc);
    for (uint64_t p0 = first; p0 < last; p0 += 256u) {
        const uint64_t p = p0 + t;
        const bool in = p < last;
        const uint64_t ns = in ? csym(p << shn) : 0, mid = in ? csym((2 * p + 1) << (shn - 1)) : 0, hi = in ? csym((p + 1) << shn) : 0;
        const uint64_t rs = hi - mid;  // size of the node's right child
        uint64_t incl = rs;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t u = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += u;
        }
        __syncthreads();
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w2 = 0; w2 < wave; w2++) before += wsum[w2];
        if (in) {
            const uint64_t r_ns = before + incl - rs, zeros = mid - ns;
            out[p] = (uint32_t)r_ns;
            dst[2 * p] = (uint32_t)r_ns;
            dst[2 * p + 1] = (uint32_t)(ns + zeros - r_ns);
        }
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
    if (last == nodes && t == 0) out[nodes] = (uint32_t)carry;
}

// syms_in: the level's order.  bits / rank: the level's bit vector (nwords words, zero padded) and its directory of ones before every
// 512-bit block (nblocks + 1 entries).  syms_out (nullptr on the last level): the next level's order.  state: zeroed, ntiles + 1 entries.
__global__ void __launch_bounds__(256) k_wt_level(const uint32_t *__restrict__ syms_in, uint32_t *__restrict__ syms_out, uint64_t ntotal,
                                                  uint32_t nlist, uint32_t L, uint32_t level,
                                                  const uint32_t *__restrict__ dstab_l, uint64_t *__restrict__ bits, uint64_t nwords,
                                                  uint32_t *__restrict__ rank, uint64_t nblocks, unsigned long long *state, uint32_t ntiles) {
    __shared__ uint64_t words[VIDC_WT_EPT * 4];
    __shared__ uint32_t wpre[VIDC_WT_EPT * 4 + 1];  // ones before every word of the tile
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t tile_s;
    __shared__ unsigned long long before_s;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if (t == 0) tile_s = (uint32_t)atomicAdd(&state[ntiles], 1ull);
    __syncthreads();
    const uint32_t tile = tile_s;
    const uint64_t base = (uint64_t)tile * VIDC_WT_TILE;
    const uint32_t bsh = L - 1u - level;  // the symbol bit this level stores
    uint32_t sym[VIDC_WT_EPT];
    uint32_t inword[VIDC_WT_EPT / 4];  // ones before the element inside its word (< 64): four per register
    uint64_t mybits = 0;
    // (every load of the tile is issued before the first ballot: a predicated load inside the ballot loop made the compiler wait for each
    // of the 64 loads in turn -- 63 us of a level's 100 were this loop)
#pragma unroll
    for (int j = 0; j < (int)VIDC_WT_EPT; j++) {
        const uint64_t i = base + (uint64_t)j * 256u + t;
        sym[j] = syms_in[i < ntotal ? i : ntotal - 1u];
    }
#pragma unroll
    for (int j = 0; j < (int)VIDC_WT_EPT; j++) {
        const uint64_t i = base + (uint64_t)j * 256u + t;
        const bool b = i < ntotal && ((sym[j] >> bsh) & 1u);
        const uint64_t m = __ballot(b);
        const uint32_t iw = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if ((j & 3) == 0) inword[j >> 2] = iw; else inword[j >> 2] |= iw << (8 * (j & 3));
        mybits |= b ? 1ull << j : 0ull;
        if (lane == 0) words[j * 4 + wave] = m;
    }
    __syncthreads();
    // ones before every word of the tile (256 words: a thread each, scan inside the wavefronts, then across the four)
    {
        const uint32_t c = (uint32_t)__builtin_popcountll(words[t]);
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o, 64);
            if (lane >= (uint32_t)o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t wbefore = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) wbefore += k < wave ? wsum[k] : 0u;
        wpre[t] = wbefore + incl - c;
        if (t == 255) wpre[256] = wbefore + incl;
        // the bit-vector words of the tile: one coalesced store
        const uint64_t w = (uint64_t)tile * (VIDC_WT_EPT * 4) + t;
        if (w < nwords) bits[w] = words[t];
    }
    __syncthreads();
    const uint32_t tile_ones = wpre[VIDC_WT_EPT * 4];
    // chained scan: publish the tile's count, look back for the ones before the tile, publish the inclusive prefix.  The look-back reads 256
    // predecessors per round trip (one per thread): the first tiles of a launch all start together and none of them holds a prefix
    // yet, so the tile numbered k makes k / 256 rounds -- with 64 per round the 2048 resident tiles of a 16.8 M-id level finished their
    // look-backs at 2 us x k / 64, and the level took 100 us for 30 us of traffic.
    {
        __shared__ unsigned long long w_all[4], w_upto[4];
        __shared__ uint32_t w_stop[4], done_s;
        if (t == 0) {
            atomicExch(&state[tile], (1ull << 62) | tile_ones);
            before_s = 0;
            done_s = tile == 0u ? 1u : 0u;
        }
        __syncthreads();
        int64_t k0 = (int64_t)tile - 1;
        while (!done_s) {
            const int64_t k = k0 - (int64_t)t;
            unsigned long long x = 0;
            if (k >= 0) {
                do { x = __hip_atomic_load(&state[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (!(x >> 62));
            }
            const uint64_t pm = __ballot(k >= 0 && (x >> 63));  // predecessors that hold an inclusive prefix
            const uint32_t stop = pm ? (uint32_t)__builtin_ctzll(pm) : 64u;  // the nearest of this wavefront's
            const unsigned long long v = k >= 0 ? (x & ((1ull << 62) - 1ull)) : 0ull;
            unsigned long long all = v, upto = lane <= stop ? v : 0ull;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                all += __shfl_xor(all, o, 64);
                upto += __shfl_xor(upto, o, 64);
            }
            if (lane == 0) { w_all[wave] = all; w_upto[wave] = upto; w_stop[wave] = stop; }
            __syncthreads();
            if (t == 0) {
                unsigned long long acc = before_s;
                bool found = false;
                for (int w = 0; w < 4 && !found; w++) {  // wavefront w holds predecessors k0 - 64 w .. k0 - 64 w - 63
                    found = w_stop[w] < 64u;
                    acc += found ? w_upto[w] : w_all[w];
                }
                before_s = acc;
                if (found || k0 - 256 < 0) done_s = 1u;
            }
            __syncthreads();
            k0 -= 256;
        }
        if (t == 0) atomicExch(&state[tile], (1ull << 63) | (before_s + tile_ones));
    }
    const uint64_t before = before_s;
    // rank directory: ones before every 512-bit block (8 words) of the tile; the entry behind the last block = the level's ones
    if (t < VIDC_WT_EPT / 2) {
        const uint64_t blk = (uint64_t)tile * (VIDC_WT_EPT / 2) + t;
        if (blk < nblocks) rank[blk] = (uint32_t)(before + wpre[t * 8u]);
    }
    if (tile + 1u == ntiles && t == 0) rank[nblocks] = (uint32_t)(before + tile_ones);
    if (!syms_out) return;
    // the next level's order: zeros of a node keep their order in its left child, ones in its right child
    const uint32_t shn = L - level;  // a node of this level spans 2^shn symbols
#pragma unroll
    for (int j0 = 0; j0 < (int)VIDC_WT_EPT; j0 += 16) {
        uint32_t tb[16];  // sixteen table entries in flight, then sixteen stores
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            const int j = j0 + jj;
            const uint32_t p = shn >= 32u ? 0u : sym[j] >> shn;
            tb[jj] = dstab_l[2u * p + ((uint32_t)(mybits >> j) & 1u)];
        }
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            const int j = j0 + jj;
            const uint64_t i = base + (uint64_t)j * 256u + t;
            const uint32_t bit = (uint32_t)(mybits >> j) & 1u;
            const uint64_t r_i = before + wpre[j * 4 + wave] + ((inword[j >> 2] >> (8 * (j & 3))) & 0xffu);  // ones before the element
            const uint64_t dst = (uint64_t)tb[jj] + (bit ? r_i : i - r_i);
            if (i < ntotal) syms_out[dst] = sym[j];
        }
    }
}

__device__ __forceinline__ uint64_t rank1(const uint64_t *bits, const uint32_t *rank, uint64_t i) {
    const uint64_t blk = i / (64 * BLK_WORDS);
    uint64_t r = rank[blk];
    const uint64_t w_end = i >> 6;
    for (uint64_t w = blk * BLK_WORDS; w < w_end; w++) r += (uint64_t)__builtin_popcountll(bits[w]);
    const uint32_t rem = (uint32_t)(i & 63);
    if (rem) r += (uint64_t)__builtin_popcountll(bits[w_end] & ((1ull << rem) - 1ull));
    return r;
}

// position of the (j+1)-th bit equal to `one` (j 0-based); nblocks = number of 512-bit blocks
__device__ __forceinline__ uint64_t select_bit(const uint64_t *bits, const uint32_t *rank, uint64_t nblocks,
                                               uint64_t nwords, uint64_t j, bool one) {
    // largest block b with count_before(b) <= j
    uint64_t lo = 0, hi = nblocks;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t before = one ? rank[mid] : mid * 64 * BLK_WORDS - rank[mid];
        if (before <= j) lo = mid; else hi = mid;
    }
    uint64_t seen = one ? rank[lo] : lo * 64 * BLK_WORDS - rank[lo];
    for (uint64_t w = lo * BLK_WORDS; w < nwords; w++) {
        uint64_t word = one ? bits[w] : ~bits[w];
        const uint32_t c = (uint32_t)__builtin_popcountll(word);
        if (seen + c > j) {
            for (uint64_t k = j - seen; k; k--) word &= word - 1;
            return w * 64 + (uint64_t)__builtin_ctzll(word);
        }
        seen += c;
    }
    return ~0ull;
}


// ---------------------------------------------------------------------------------------------------------------
// bit-vector views: what the query kernels need from a level, over plain bits or over the RRR coding
struct BvPlain {
    const uint64_t *bits;
    const uint32_t *rank;
    uint64_t nblocks, nwords;
    __device__ __forceinline__ uint64_t rank_1(uint64_t i) const { return rank1(bits, rank, i); }
    __device__ __forceinline__ uint64_t rank_1_bit(uint64_t i, bool &bit) const {
        bit = (bits[i >> 6] >> (i & 63)) & 1ull;
        return rank1(bits, rank, i);
    }
    __device__ __forceinline__ uint64_t select(uint64_t j, bool one) const { return select_bit(bits, rank, nblocks, nwords, j, one); }
    // the same when the answer is known to lie in [p0, p1) (a node of the level): the directory search starts from the node's blocks
    __device__ __forceinline__ uint64_t select_in(uint64_t j, bool one, uint64_t p0, uint64_t p1) const {
        uint64_t lo = p0 / (64 * BLK_WORDS), hi = p1 / (64 * BLK_WORDS) + 1;
        if (hi > nblocks) hi = nblocks;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            const uint64_t before = one ? rank[mid] : mid * 64 * BLK_WORDS - rank[mid];
            if (before <= j) lo = mid; else hi = mid;
        }
        uint64_t seen = one ? rank[lo] : lo * 64 * BLK_WORDS - rank[lo];
        for (uint64_t w = lo * BLK_WORDS; w < nwords; w++) {
            uint64_t word = one ? bits[w] : ~bits[w];
            const uint32_t c = (uint32_t)__builtin_popcountll(word);
            if (seen + c > j) {
                for (uint64_t k = j - seen; k; k--) word &= word - 1;
                return w * 64 + (uint64_t)__builtin_ctzll(word);
            }
            seen += c;
        }
        return ~0ull;
    }
    static constexpr bool kRrr = false;
};
struct WtPlainView {
    static constexpr bool kRrrView = false;
    const uint64_t *bits;
    const uint32_t *rank;
    uint64_t wpl, bpl;
    __device__ __forceinline__ BvPlain level(uint32_t l) const {
        return BvPlain{bits + (uint64_t)l * wpl, rank + (uint64_t)l * (bpl + 1), bpl, wpl};
    }
};

struct RrrTab { uint8_t ow[64]; };  // offset width of class c: ceil(log2 C(63, c))

// index of the 63-bit word v (c ones) among the words with c ones: sum over its ones (ascending, i = 1..c) of C(p_i, i)
__device__ __forceinline__ uint64_t rrr_rank_word(uint64_t v, const uint64_t *binom) {
    uint64_t o = 0;
    uint32_t i = 1;
    while (v) {
        const uint32_t p = (uint32_t)__builtin_ctzll(v);
        o += binom[p * 64u + i];
        i++;
        v &= v - 1;
    }
    return o;
}
__device__ __forceinline__ uint64_t rrr_unrank_word(uint32_t c, uint64_t o, const uint64_t *binom) {
    if (c == 0) return 0;
    if (c == RRR_B) return (1ull << RRR_B) - 1ull;
    uint64_t v = 0;
    for (int p = (int)RRR_B - 1; c; p--) {
        const uint64_t b = binom[(uint32_t)p * 64u + c];  // words with c ones below position p
        if (o >= b) { v |= 1ull << p; o -= b; c--; }
    }
    return v;
}
// ones of the block (class c, offset o) below position rem, and the bit at rem: the unranking only has to walk the positions
// from the top down to rem (what is left of c afterwards sits below)
__device__ __forceinline__ uint32_t rrr_rank_below(uint32_t c, uint64_t o, uint32_t rem, bool &bit, const uint64_t *binom) {
    bit = false;
    if (c == 0) return 0;
    if (c == RRR_B) { bit = rem < RRR_B; return rem; }
    for (int p = (int)RRR_B - 1; p >= (int)rem && c; p--) {
        const uint64_t b = binom[(uint32_t)p * 64u + c];
        if (o >= b) {
            o -= b;
            c--;
            if ((uint32_t)p == rem) { bit = true; }
        }
    }
    return c;
}
struct BvRrr {
    const uint32_t *cls;
    const uint64_t *offs;
    const uint32_t *ptr, *rs;
    const uint64_t *binom;
    const uint8_t *ow;  // offset width by class (memory, not a by-value table: a dynamically indexed kernel argument goes to scratch)
    uint64_t nblk, nsamp, nbits;
    __device__ __forceinline__ uint32_t cls_at(uint64_t b) const {
        const uint64_t bp = 6 * b;
        uint32_t w = cls[bp >> 5] >> (bp & 31);
        if ((bp & 31) > 26) w |= cls[(bp >> 5) + 1] << (32 - (bp & 31));
        return w & 63u;
    }
    __device__ __forceinline__ uint64_t offset_at(uint64_t bp, uint32_t c) const {  // offset field of the block starting at bit bp
        const uint32_t wd = ow[c];
        uint64_t o = 0;
        if (wd) {
            o = offs[bp >> 6] >> (bp & 63);
            if ((bp & 63) + wd > 64) o |= offs[(bp >> 6) + 1] << (64 - (bp & 63));
            o &= (1ull << wd) - 1ull;
        }
        return o;
    }
    __device__ __forceinline__ uint64_t word_at(uint64_t bp, uint32_t c) const { return rrr_unrank_word(c, offset_at(bp, c), binom); }
    // position inside the block (class c, offset o, `len` existing bits) of its (k+1)-th bit equal to `one`: the unranking walks
    // the positions from the top and stops at the wanted bit (the k-th from below is the (count - 1 - k)-th from above) instead
    // of rebuilding the whole word and clearing k bits
    __device__ __forceinline__ uint32_t select_in_block(uint32_t c, uint64_t o, uint32_t k, bool one, uint32_t len) const {
        uint32_t t = (one ? c : len - c) - 1u - k;  // wanted bit, counted from the top among the existing bits of its kind
        for (int p = (int)RRR_B - 1; p >= 0; p--) {
            if (c == 0) return one ? 0u : (uint32_t)p - t - ((uint32_t)p >= len ? (uint32_t)p + 1u - len : 0u);  // only zeros below
            const uint64_t b = binom[(uint32_t)p * 64u + c];
            const bool bit = o >= b;
            if (bit) { o -= b; c--; }
            if ((uint32_t)p < len && bit == one) {
                if (t == 0) return (uint32_t)p;
                t--;
            }
        }
        return 0u;
    }
    __device__ __forceinline__ uint64_t rank_1_bit(uint64_t i, bool &bit) const {
        const uint64_t blk = i / RRR_B, s = blk / RRR_K;
        uint64_t r = rs[s], bp = ptr[s];
        for (uint64_t b = s * RRR_K; b < blk; b++) {
            const uint32_t c = cls_at(b);
            r += c;
            bp += ow[c];
        }
        const uint32_t rem = (uint32_t)(i - blk * RRR_B);
        bit = false;
        if (blk < nblk) {
            const uint32_t c = cls_at(blk);
            r += rrr_rank_below(c, offset_at(bp, c), rem, bit, binom);
        }
        return r;
    }
    __device__ __forceinline__ uint64_t rank_1(uint64_t i) const {
        bool b;
        return rank_1_bit(i, b);
    }
    __device__ __forceinline__ uint64_t before(uint64_t s, bool one) const {  // ones / zeros in blocks [0, 32 s)
        const uint64_t r = rs[s];
        if (one) return r;
        const uint64_t pos = s * RRR_K * RRR_B;
        return (pos < nbits ? pos : nbits) - r;
    }
    __device__ __forceinline__ uint64_t select(uint64_t j, bool one) const { return select_in(j, one, 0, nbits); }
    // (j+1)-th bit equal to `one`, known to lie in [p0, p1) (a node of the level).  The sample search starts from the node's
    // samples (a node of a deep level spans one or two), the 32 classes behind the sample -- 192 bits, word-aligned: sample s
    // starts at bit 6 * 32 s -- come with three independent 8-byte loads and are walked in registers, and the unranking stops at
    // the wanted bit.  The first version made up to 13 + 2 * 31 + 63 DEPENDENT loads per level (directory, one class and one
    // width per block, one binomial per position): 5 ms for a select on a 16-level tree, whatever the number of queries.
    __device__ __forceinline__ uint64_t select_in(uint64_t j, bool one, uint64_t p0, uint64_t p1) const {
        uint64_t lo = p0 / (RRR_K * RRR_B), hi = p1 / (RRR_K * RRR_B) + 1;
        if (hi > nsamp) hi = nsamp;
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (before(mid, one) <= j) lo = mid; else hi = mid;
        }
        uint64_t seen = before(lo, one), bp = ptr[lo];
        const uint2 *cw = (const uint2 *)(cls + 6 * lo);  // (cls_wpl has a pad word; the level's last sample may read into it)
        const uint2 q0 = cw[0], q1 = cw[1], q2 = cw[2];
        const uint32_t w[7] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, 0u};
        bool found = false;
        uint64_t fb = 0, fbp = 0, fseen = 0;
        uint32_t fc = 0, flen = 0;
#pragma unroll
        for (uint32_t k = 0; k < RRR_K; k++) {
            const uint64_t b = lo * RRR_K + k;
            const uint32_t bit0 = 6u * k, wi = bit0 >> 5, sh = bit0 & 31u;
            uint32_t c = w[wi] >> sh;
            if (sh > 26u) c |= w[wi + 1] << (32u - sh);
            c &= 63u;
            if (!found && b < nblk) {
                const uint64_t len = nbits - b * RRR_B < RRR_B ? nbits - b * RRR_B : RRR_B;  // bits of this block that exist
                const uint64_t cnt = one ? c : len - c;
                if (seen + cnt > j) { found = true; fb = b; fbp = bp; fseen = seen; fc = c; flen = (uint32_t)len; }
                else { seen += cnt; bp += ow[c]; }
            }
        }
        if (found) return fb * RRR_B + select_in_block(fc, offset_at(fbp, fc), (uint32_t)(j - fseen), one, flen);
        for (uint64_t b = (lo + 1) * RRR_K; b < nblk; b++) {  // (not reached while the samples are consistent)
            const uint32_t c = cls_at(b);
            const uint64_t len = nbits - b * RRR_B < RRR_B ? nbits - b * RRR_B : RRR_B;
            const uint64_t cnt = one ? c : len - c;
            if (seen + cnt > j) return b * RRR_B + select_in_block(c, offset_at(bp, c), (uint32_t)(j - seen), one, (uint32_t)len);
            seen += cnt;
            bp += ow[c];
        }
        return ~0ull;
    }
    static constexpr bool kRrr = true;
};
struct WtRrrView {
    static constexpr bool kRrrView = true;
    const uint32_t *cls;
    const uint64_t *offs;
    const uint32_t *ptr, *rs;
    const uint64_t *binom;
    uint64_t cls_wpl, nblk, nsamp, nbits;
    uint64_t off_base[32];
    __device__ __forceinline__ BvRrr level(uint32_t l) const {
        return BvRrr{cls + (uint64_t)l * cls_wpl, offs + off_base[l], ptr + (uint64_t)l * (nsamp + 1), rs + (uint64_t)l * (nsamp + 1),
                     binom, (const uint8_t *)(binom + 64 * 64), nblk, nsamp, nbits};
    }
};

// ---- RRR build kernels (one thread per 63-bit block of a level's plain bits)
__device__ __forceinline__ uint64_t rrr_get63(const uint64_t *bits, uint64_t b) {
    const uint64_t pos = b * RRR_B;
    uint64_t v = bits[pos >> 6] >> (pos & 63);
    if ((pos & 63) + RRR_B > 64) v |= bits[(pos >> 6) + 1] << (64 - (pos & 63));
    return v & ((1ull << RRR_B) - 1ull);
}
__global__ void k_rrr_classes(const uint64_t *bits, uint64_t nblk, RrrTab tab, uint32_t *cls, uint32_t *width) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += stride) {
        const uint32_t c = (uint32_t)__builtin_popcountll(rrr_get63(bits, b));
        width[b] = tab.ow[c];
        const uint64_t bp = 6 * b;
        atomicOr(&cls[bp >> 5], c << (bp & 31));
        if ((bp & 31) > 26) atomicOr(&cls[(bp >> 5) + 1], c >> (32 - (bp & 31)));
    }
}
__global__ void k_rrr_offsets(const uint64_t *bits, uint64_t nblk, RrrTab tab, const uint64_t *binom, const uint64_t *bitpos,
                              unsigned long long *offs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += stride) {
        const uint64_t v = rrr_get63(bits, b);
        const uint32_t wd = tab.ow[__builtin_popcountll(v)];
        if (!wd) continue;
        const uint64_t o = rrr_rank_word(v, binom), bp = bitpos[b];
        atomicOr(&offs[bp >> 6], (unsigned long long)(o << (bp & 63)));
        if ((bp & 63) + wd > 64) atomicOr(&offs[(bp >> 6) + 1], (unsigned long long)(o >> (64 - (bp & 63))));
    }
}
__global__ void k_rrr_samples(const uint64_t *bits, const uint32_t *rank, uint64_t nbits, uint64_t nblk, uint64_t nsamp,
                              const uint64_t *bitpos, uint32_t *ptr, uint32_t *rs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= nsamp; s += stride) {
        const uint64_t b = s * RRR_K < nblk ? s * RRR_K : nblk;
        const uint64_t pos = b * RRR_B < nbits ? b * RRR_B : nbits;
        ptr[s] = (uint32_t)bitpos[b];
        rs[s] = (uint32_t)rank1(bits, rank, pos);
    }
}

// Bulk decode of a compressed tree: a level is turned back into plain bits ONCE -- a thread per 63-bit block: the sample before
// it, the classes up to it, one unranking -- with the 512-bit rank directory the plain kernels use (a thread per entry, from
// the samples and classes), and the level's partition then runs on the plain view.  The per-element form unranked a block for
// each of the three ranks every element asks its level for: 16 M ids decoded in 23 ms, 11 x the plain tree.
__global__ void k_rrr_expand(BvRrr bv, unsigned long long *bits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < bv.nblk; b += stride) {
        const uint64_t s = b / RRR_K;
        uint64_t bp = bv.ptr[s];
        for (uint64_t k = s * RRR_K; k < b; k++) bp += bv.ow[bv.cls_at(k)];
        const uint32_t c = bv.cls_at(b);
        if (!c) continue;  // (the scratch is zeroed)
        const uint64_t v = bv.word_at(bp, c), pos = b * RRR_B;
        atomicOr(&bits[pos >> 6], (unsigned long long)(v << (pos & 63)));
        if ((pos & 63) + RRR_B > 64) atomicOr(&bits[(pos >> 6) + 1], (unsigned long long)(v >> (64 - (pos & 63))));
    }
}
__global__ void k_rrr_rankdir(BvRrr bv, uint64_t nblocks, uint32_t *rank) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= nblocks; j += stride) {
        const uint64_t pos = j * 64 * BLK_WORDS;
        rank[j] = (uint32_t)bv.rank_1(pos < bv.nbits ? pos : bv.nbits);
    }
}

// the tables an RRR view looks up once per position / per block, in LDS for the kernels that walk levels per query (the binomials
// are a dependent load per unranked position: ~30 of them per level and query)
template <class View>
__device__ __forceinline__ void wt_stage_tables(const View &vw, uint64_t *s_binom, uint8_t *s_ow) {
    if constexpr (View::kRrrView) {
        for (uint32_t i = threadIdx.x; i < 64u * 64u; i += blockDim.x) s_binom[i] = vw.binom[i];
        const uint8_t *ow = (const uint8_t *)(vw.binom + 64 * 64);
        for (uint32_t i = threadIdx.x; i < 64u; i += blockDim.x) s_ow[i] = ow[i];
        __syncthreads();
    }
}
template <class Bv>
__device__ __forceinline__ void wt_use_tables(Bv &bv, const uint64_t *s_binom, const uint8_t *s_ow) {
    if constexpr (Bv::kRrr) { bv.binom = s_binom; bv.ow = s_ow; }
}

// the walk of one select: position of the (pos+1)-th element of list c, from the root level down
template <class View>
__device__ __forceinline__ uint64_t wt_select_walk(const View &vw, const uint64_t *C, const uint32_t *__restrict__ nrank, uint32_t nlist,
                                                   uint32_t L, uint32_t c, uint64_t pos, const uint64_t *s_binom, const uint8_t *s_ow) {
    for (int level = (int)L - 1; level >= 0; level--) {
        const uint32_t sh = L - (uint32_t)level;
        const uint64_t p = sh >= 32 ? 0 : (uint64_t)(c >> sh);
        const uint64_t s_lo = sh >= 32 ? 0 : (p << sh);
        uint64_t s_hi = sh >= 32 ? nlist : ((p + 1) << sh);
        if (s_hi > nlist) s_hi = nlist;
        const uint64_t ns = C[s_lo], ne = C[s_hi];
        const bool bit = (c >> (L - 1u - (uint32_t)level)) & 1u;
        auto bv = vw.level((uint32_t)level);
        wt_use_tables(bv, s_binom, s_ow);
        const uint64_t r_ns = nrank[wt_nrank_base((uint32_t)level) + p];  // (== bv.rank_1(ns), from the build)
        const uint64_t before = bit ? r_ns : ns - r_ns;
        pos = bv.select_in(before + pos, bit, ns, ne) - ns;
    }
    return pos;
}

// one thread per query: id of the (k+1)-th element of list c.  LABELS (vidc_wt_translate_labels_dev): list_nos holds Faiss labels
// (int64 list << 32 | offset; offs unused), checked against C before the walk starts; -1 for a negative or invalid label, the invalid
// ones counted.  out may then be the labels array itself.
template <class View, bool LABELS = false>
__global__ void k_wt_select(View vw, const uint64_t *C, const uint32_t *__restrict__ nrank, uint32_t nlist, uint32_t L, uint64_t m,
                            const uint64_t *list_nos, const uint64_t *offs, int64_t *out, unsigned long long *invalid = nullptr) {
    __shared__ uint64_t s_binom[View::kRrrView ? 64 * 64 : 1];
    __shared__ uint8_t s_ow[64];
    wt_stage_tables(vw, s_binom, s_ow);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if constexpr (LABELS) {
        for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); q0 < m; q0 += stride) {  // (q0: wavefront-uniform)
            const uint64_t q = q0 + (threadIdx.x & 63u);
            uint64_t l = 0, o = 0;
            const bool nonneg = req_label(q < m ? (int64_t)list_nos[q] : -1, l, o);
            const bool ok = nonneg && l < nlist && o < C[l + 1] - C[l];
            req_count_invalid(nonneg && !ok, invalid);
            if (ok) out[q] = (int64_t)wt_select_walk(vw, C, nrank, nlist, L, (uint32_t)l, o, s_binom, s_ow);
            else if (q < m) out[q] = -1;
        }
    } else {
        for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += stride)
            out[q] = (int64_t)wt_select_walk(vw, C, nrank, nlist, L, (uint32_t)list_nos[q], offs[q], s_binom, s_ow);
    }
}

// Locate (vidc_wt_locate_dev), one thread per pair: wt_select_walk the other way.  Id i is position i of the root; at every level the
// bit at the position names the child and the rank inside the node (the level's rank minus the ones before the node start, nrank) is
// the position in that child.  The leaf is the list, the last position the offset.  No sort and no decode: a tree holds every id
// 0 .. ntotal - 1 exactly once, so the label is unique.  list_nos == NULL: any-list mode; else the leaf has to equal list_nos[q]
// (negative: skipped; >= nlist: skipped and counted in *invalid).  -1 and one more in *missing for a valid pair that finds nothing.
template <class View>
__global__ void k_wt_locate(View vw, const uint64_t *C, const uint32_t *__restrict__ nrank, uint32_t nlist, uint32_t L, uint64_t ntotal, uint64_t n,
                            const int64_t *__restrict__ list_nos, const uint64_t *__restrict__ ids, int64_t *__restrict__ labels,
                            unsigned long long *missing, unsigned long long *invalid) {
    __shared__ uint64_t s_binom[View::kRrrView ? 64 * 64 : 1];
    __shared__ uint8_t s_ow[64];
    wt_stage_tables(vw, s_binom, s_ow);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); q0 < n; q0 += stride) {  // (q0: wavefront-uniform)
        const uint64_t q = q0 + (threadIdx.x & 63u);
        const bool in = q < n;
        const int64_t l = in ? (list_nos ? list_nos[q] : 0) : -1;
        const bool ok = in && (!list_nos || (l >= 0 && (uint64_t)l < nlist));
        const uint64_t id = in ? ids[q] : 0;
        int64_t lab = -1;
        if (ok && id < ntotal) {
            uint64_t pos = id;
            uint32_t p = 0;
            for (uint32_t level = 0; level < L; level++) {
                const uint32_t sh = L - level;
                uint64_t s_lo = sh >= 32 ? 0 : ((uint64_t)p << sh);
                if (s_lo > nlist) s_lo = nlist;
                const uint64_t ns = C[s_lo];
                auto bv = vw.level(level);
                wt_use_tables(bv, s_binom, s_ow);
                bool bit;
                const uint64_t ones = bv.rank_1_bit(ns + pos, bit) - nrank[wt_nrank_base(level) + p];
                pos = bit ? ones : pos - ones;
                p = 2u * p + (bit ? 1u : 0u);
            }
            if (!list_nos || (int64_t)p == l) lab = (int64_t)(((uint64_t)p << 32) | pos);
        }
        if (in) labels[q] = lab;
        req_count_invalid(in && l >= 0 && !ok, invalid);
        req_count_invalid(ok && lab < 0, missing);
    }
}

// get_ids of the requested lists (custom_invlists_impl.cpp:381-392 loops get_single_id): one thread per output slot,
// its request item found in the m + 1 output offsets
template <class View>
__global__ void k_wt_decode_lists(View vw, const uint64_t *C, const uint32_t *__restrict__ nrank, uint32_t nlist_, uint32_t L, uint64_t m,
                                  const uint64_t *list_nos, const uint64_t *out_off, uint64_t total, uint64_t *out) {
    __shared__ uint64_t s_binom[View::kRrrView ? 64 * 64 : 1];
    __shared__ uint8_t s_ow[64];
    wt_stage_tables(vw, s_binom, s_ow);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        uint64_t lo = 0, hi = m;  // largest i with out_off[i] <= g
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (out_off[mid] <= g) lo = mid; else hi = mid;
        }
        const uint32_t c = (uint32_t)list_nos[lo];
        uint64_t pos = g - out_off[lo];
        for (int level = (int)L - 1; level >= 0; level--) {
            const uint32_t sh = L - (uint32_t)level;
            const uint64_t p = sh >= 32 ? 0 : (uint64_t)(c >> sh);
            const uint64_t ns = C[sh >= 32 ? 0 : (p << sh)];
            uint64_t s_hi = sh >= 32 ? nlist_ : ((p + 1) << sh);
            if (s_hi > nlist_) s_hi = nlist_;
            const uint64_t ne = C[s_hi];
            const bool bit = (c >> (L - 1u - (uint32_t)level)) & 1u;
            auto bv = vw.level((uint32_t)level);
            wt_use_tables(bv, s_binom, s_ow);
            const uint64_t r_ns = nrank[wt_nrank_base((uint32_t)level) + p];
            pos = bv.select_in((bit ? r_ns : ns - r_ns) + pos, bit, ns, ne) - ns;
        }
        out[g] = pos;
    }
}

// get_ids for every list as L stable partitions of the id sequence (the build's own passes, run on ids instead of
// symbols): at level l the element at position i of node p goes to the zeros / ones part of its node, one rank per
// element instead of the select (binary search over the rank directory + word scan) the per-id walk needs per level.
// in == nullptr: level 0 (position i holds id i, prefix 0).  LAST: the final order is the answer (u64 ids).
struct WtItem {
    uint32_t id, pref;
};

// The pass over tiles of 8192 consecutive positions (round 6): the tile's 128 bit-vector words and 16 rank-directory entries give
// every position its bit and rank (v_mbcnt inside the word) -- a per-element form asked the rank directory and up to eight words
// per element --, the destination is one table entry (d_dstab) plus that rank, and all of a thread's 32 items are requested before any
// of them is used.
template <bool LAST>
__global__ void __launch_bounds__(256) k_wt_decode_tile(const WtItem *__restrict__ in, WtItem *__restrict__ out, uint64_t *__restrict__ out_ids,
                                                        const uint64_t *__restrict__ bits, uint64_t nwords, const uint32_t *__restrict__ rank,
                                                        const uint32_t *__restrict__ dstab_l, uint64_t ntotal) {
    __shared__ uint64_t words[VIDC_WTD_EPT * 4];
    __shared__ uint32_t wpre[VIDC_WTD_EPT * 4];  // ones before every word of the tile, from the start of the level
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * (256u * VIDC_WTD_EPT);
    WtItem it[VIDC_WTD_EPT];
#pragma unroll
    for (int j = 0; j < (int)VIDC_WTD_EPT; j++) {
        const uint64_t i = base + (uint64_t)j * 256u + t;
        if (in) it[j] = in[i < ntotal ? i : ntotal - 1u];
        else it[j] = WtItem{(uint32_t)i, 0u};  // level 0: position i holds id i, prefix 0
    }
    if (t < VIDC_WTD_EPT * 4) {
        const uint64_t w = (uint64_t)blockIdx.x * (VIDC_WTD_EPT * 4) + t;
        words[t] = w < nwords ? bits[w] : 0ull;
    }
    __syncthreads();
    if (t < VIDC_WTD_EPT * 4) {
        const uint64_t blk = (uint64_t)blockIdx.x * (VIDC_WTD_EPT / 2) + (t >> 3);
        uint32_t c = blk * 8u < nwords ? rank[blk] : 0u;
        for (uint32_t k = t & ~7u; k < t; k++) c += (uint32_t)__builtin_popcountll(words[k]);
        wpre[t] = c;
    }
    __syncthreads();
#pragma unroll
    for (int j0 = 0; j0 < (int)VIDC_WTD_EPT; j0 += 16) {
        uint32_t tb[16];
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            const int j = j0 + jj;
            const uint64_t wd = words[j * 4 + wave];
            const uint32_t bit = (uint32_t)(wd >> lane) & 1u;
            tb[jj] = dstab_l[2u * it[j].pref + bit];
        }
#pragma unroll
        for (int jj = 0; jj < 16; jj++) {
            const int j = j0 + jj;
            const uint64_t i = base + (uint64_t)j * 256u + t;
            const uint64_t wd = words[j * 4 + wave];
            const uint32_t bit = (uint32_t)(wd >> lane) & 1u;
            const uint64_t r_i = (uint64_t)wpre[j * 4 + wave] +
                                 __builtin_amdgcn_mbcnt_hi((uint32_t)(wd >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)wd, 0u));
            const uint64_t dst = (uint64_t)tb[jj] + (bit ? r_i : i - r_i);
            if (i < ntotal) {
                if (LAST) out_ids[dst] = it[j].id;
                else out[dst] = WtItem{it[j].id, (it[j].pref << 1) | bit};
            }
        }
    }
}

// ---- import (vidc_wt_import): the derived tables rebuilt from an image, and the checks that make an untrusted image one the query
// kernels walk in bounds.  Streaming passes over the level bits / the packed classes, one scan over the concatenated levels each
// (scan.h), and two checks that report through one error word (the smallest key wins: block checks in front of node checks, then
// level << 56 | index << 8 | kind).
#define VIDC_WT_IMP_OFFSET 1u   // an RRR block's offset is >= C(63, class)
#define VIDC_WT_IMP_CLASS 2u    // an RRR block's class exceeds the bits the block has
#define VIDC_WT_IMP_STRAY 3u    // an RRR block has a one behind the end of the level
#define VIDC_WT_IMP_NODE 4u     // ones before a node boundary differ from what the offsets demand
__device__ __forceinline__ unsigned long long wt_imp_key(uint32_t level, uint64_t index, uint32_t kind) {
    return ((unsigned long long)(kind == VIDC_WT_IMP_NODE) << 63) | ((unsigned long long)level << 56) | ((unsigned long long)index << 8) | kind;
}
// ones of every 512-bit block of every level (blockIdx.y): a thread per word -- coalesced --, eight neighbouring lanes add up.
// wpl: words of a level as stored (with its pad word), bpl = ceil(wpl / 8)
__global__ void __launch_bounds__(256) k_wt_imp_block_ones(const uint64_t *__restrict__ bits, uint64_t wpl, uint64_t bpl, uint32_t *__restrict__ ones) {
    const uint64_t level = blockIdx.y, w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t c = w < wpl ? (uint32_t)__builtin_popcountll(bits[level * wpl + w]) : 0u;
    c += (uint32_t)__shfl_xor((int)c, 1, 64);
    c += (uint32_t)__shfl_xor((int)c, 2, 64);
    c += (uint32_t)__shfl_xor((int)c, 4, 64);
    if ((threadIdx.x & 7u) == 0u && (w >> 3) < bpl) ones[level * bpl + (w >> 3)] = c;
}
// sums of the classes and of their offset widths over every sample (32 blocks = six class words) of every level (blockIdx.y)
__global__ void __launch_bounds__(256) k_wt_imp_sample_sums(const uint32_t *__restrict__ cls, uint64_t cls_wpl, uint64_t nsamp, const uint8_t *__restrict__ ow,
                                                            uint32_t *__restrict__ csum, uint32_t *__restrict__ wsum) {
    __shared__ uint8_t s_ow[64];
    if (threadIdx.x < 64u) s_ow[threadIdx.x] = ow[threadIdx.x];
    __syncthreads();
    const uint64_t level = blockIdx.y, s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s >= nsamp) return;
    const uint2 *cw = (const uint2 *)(cls + level * cls_wpl + 6 * s);  // (cls_wpl is even and a sample is 24 bytes: 8-byte aligned)
    const uint2 q0 = cw[0], q1 = cw[1], q2 = cw[2];
    const uint32_t w[7] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, 0u};
    uint32_t cs = 0, ws = 0;
#pragma unroll
    for (uint32_t k = 0; k < RRR_K; k++) {
        const uint32_t bit0 = 6u * k, wi = bit0 >> 5, sh = bit0 & 31u;
        uint32_t c = w[wi] >> sh;
        if (sh > 26u) c |= w[wi + 1] << (32u - sh);
        c &= 63u;
        cs += c;
        ws += s_ow[c];
    }
    csum[level * nsamp + s] = cs;
    wsum[level * nsamp + s] = ws;
}
// per-level exclusive prefixes out of ONE scan over the concatenated levels: out[level][j] = scan[level * per + j] - scan[level * per]
// for j = 0 .. per; totals (may be NULL): the levels' sums
__global__ void __launch_bounds__(256) k_wt_imp_level_prefix(const uint64_t *__restrict__ scan, uint64_t per, uint32_t *__restrict__ out,
                                                             uint64_t *__restrict__ totals) {
    const uint64_t level = blockIdx.y, base = scan[level * per];
    for (uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x; j <= per; j += (uint64_t)gridDim.x * 256u) {
        const uint64_t v = scan[level * per + j] - base;
        out[level * (per + 1) + j] = (uint32_t)v;
        if (totals && j == per) totals[level] = v;
    }
}
// every RRR block of every level (blockIdx.y): offset < C(63, class), class <= the bits the block has, no one behind the level's end.
// The samples and the per-level totals of the widths were checked against off_bits before: every offset field lies inside its stream.
__global__ void __launch_bounds__(256) k_wt_imp_check_blocks(WtRrrView vw, unsigned long long *err) {
    const uint32_t level = blockIdx.y;
    const BvRrr bv = vw.level(level);
    for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < bv.nblk; b += (uint64_t)gridDim.x * 256u) {
        const uint64_t s = b / RRR_K;
        uint64_t bp = bv.ptr[s];
        for (uint64_t k = s * RRR_K; k < b; k++) bp += bv.ow[bv.cls_at(k)];
        const uint32_t c = bv.cls_at(b);
        const uint64_t left = bv.nbits - b * RRR_B;
        const uint32_t len = left < RRR_B ? (uint32_t)left : RRR_B;
        uint32_t kind = 0;
        if (c > len) kind = VIDC_WT_IMP_CLASS;
        else {
            const uint64_t o = bv.offset_at(bp, c);
            if (o >= bv.binom[RRR_B * 64u + c]) kind = VIDC_WT_IMP_OFFSET;
            else if (len < RRR_B && (rrr_unrank_word(c, o, bv.binom) >> len)) kind = VIDC_WT_IMP_STRAY;
        }
        if (kind) atomicMin(err, wt_imp_key(level, b, kind));
    }
}
// every node boundary p = 0 .. 2^level of every level (blockIdx.y): the ones in front of position C[min(p << (L - level), nlist)], asked of
// the imported structure, against the nrank entry computed from the offsets alone
template <class View>
__global__ void __launch_bounds__(256) k_wt_imp_check_nodes(View vw, const uint64_t *__restrict__ C, const uint32_t *__restrict__ nrank, uint32_t nlist,
                                                            uint32_t L, unsigned long long *err) {
    const uint32_t level = blockIdx.y, shn = L - level;
    const uint64_t nodes = 1ull << level;
    const auto bv = vw.level(level);
    const uint32_t *want = nrank + wt_nrank_base(level);
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= nodes; p += (uint64_t)gridDim.x * 256u) {
        uint64_t sym = p << shn;
        if (sym > nlist) sym = nlist;
        if ((uint32_t)bv.rank_1(C[sym]) != want[p]) atomicMin(err, wt_imp_key(level, p, VIDC_WT_IMP_NODE));
    }
}

WtPlainView plain_view(const vidc_wt *w) { return WtPlainView{w->d_bits.p, w->d_rank.p, w->words_per_level, w->blocks_per_level}; }
RrrTab rrr_tab() {
    RrrTab t;
    for (int c = 0; c <= 63; c++) {  // ceil(log2(binom(63, c)))
        long double lg = 0;
        for (int i = 1; i <= c; i++) lg += log2l((long double)(63 - c + i)) - log2l((long double)i);
        t.ow[c] = (uint8_t)ceill(lg - 1e-12L);
    }
    return t;
}
BvRrr rrr_view_level(const vidc_wt *w, uint32_t l) {
    return BvRrr{w->d_cls.p + (uint64_t)l * w->rrr_cls_wpl, w->d_offs.p + w->rrr_off_base[l], w->d_ptr.p + (uint64_t)l * (w->rrr_nsamp + 1),
                 w->d_rs.p + (uint64_t)l * (w->rrr_nsamp + 1), w->d_binom.p, (const uint8_t *)(w->d_binom.p + 64 * 64), w->rrr_nblk,
                 w->rrr_nsamp, w->ntotal};
}
WtRrrView rrr_view(const vidc_wt *w) {
    WtRrrView v{};
    v.cls = w->d_cls.p; v.offs = w->d_offs.p; v.ptr = w->d_ptr.p; v.rs = w->d_rs.p; v.binom = w->d_binom.p;
    v.cls_wpl = w->rrr_cls_wpl; v.nblk = w->rrr_nblk; v.nsamp = w->rrr_nsamp; v.nbits = w->ntotal;
    for (uint32_t l = 0; l < w->L && l < 32; l++) v.off_base[l] = w->rrr_off_base[l];
    return v;
}

}  // namespace

// the tables of an RRR-coded object (build and import): C(n, k) for n, k < 64 and, behind them, the 64 offset widths as bytes
static int wt_rrr_tables(vidc_ctx *ctx, vidc_wt *w, const RrrTab &tab) {
    std::vector<uint64_t> bn(64 * 64, 0);
    for (int n = 0; n < 64; n++) {
        bn[n * 64] = 1;
        for (int k = 1; k <= n; k++) bn[n * 64 + k] = (n ? bn[(n - 1) * 64 + k - 1] : 0) + (k <= n - 1 ? bn[(n - 1) * 64 + k] : 0);
    }
    VIDC_HIP(hipMemcpyAsync(w->d_binom.p, bn.data(), 64 * 64 * 8, hipMemcpyHostToDevice, ctx->stream));
    VIDC_HIP(hipMemcpyAsync(w->d_binom.p + 64 * 64, tab.ow, 64, hipMemcpyHostToDevice, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (bn leaves scope)
    return VIDC_OK;
}

// ---- shared by build and import.  What they decide is wt_plan.h's; the stages below only queue it.
// the object of a geometry: its fields and every device array the geometry sizes (the offset streams follow their bit counts:
// wt_set_offset_streams)
static int wt_object_alloc(vidc_ctx *ctx, vidc_wt *w, uint64_t nlist, const WtGeom &g) {
    w->device = ctx->device;
    w->nlist = nlist; w->ntotal = g.ntotal;
    w->wt_type = g.wt_type; w->L = g.L;
    w->words_per_level = g.words_per_level; w->blocks_per_level = g.blocks_per_level;
    if (g.wt_type == 1) {
        w->rrr_nblk = g.nblk; w->rrr_nsamp = g.nsamp; w->rrr_cls_wpl = g.cls_wpl;
        w->rrr_off_base.assign(g.L + 1, 0);
    }
    VIDC_TRY(w->d_C.alloc(g.C_n));
    VIDC_TRY(w->d_nrank.alloc(g.nrank_n));
    VIDC_TRY(w->d_dstab.alloc(g.dstab_n));
    VIDC_TRY(w->d_bits.alloc(g.bits_n));
    VIDC_TRY(w->d_rank.alloc(g.rank_n));
    VIDC_TRY(w->d_cls.alloc(g.cls_n));
    VIDC_TRY(w->d_ptr.alloc(g.samp_n));
    VIDC_TRY(w->d_rs.alloc(g.samp_n));
    VIDC_TRY(w->d_binom.alloc(g.binom_n));
    return VIDC_OK;
}
static WtGeom wt_geom_of(const vidc_wt *w) { return wt_geom(w->nlist, w->ntotal, w->wt_type); }
// wt_type 1: the exact-size offset streams, level after level
static int wt_set_offset_streams(vidc_wt *w, const WtGeom &g, const uint64_t *off_bits) {
    w->rrr_off_bits.assign(off_bits, off_bits + g.L);
    w->rrr_off_base = wt_off_base(g, off_bits);
    return w->d_offs.alloc(w->rrr_off_base[g.L]);
}
// the ones before every node start of every level and the partition tables, from the symbol start table alone (d_nrank is cleared
// by the caller, where each call always queued that: the build in front of its timed region, the import inside)
static int wt_queue_node_tables(vidc_ctx *ctx, vidc_wt *w, const WtGeom &g) {
    hipLaunchKernelGGL(k_wt_node_ranks_from_C, dim3(wt_nr_grid(g)), dim3(256), 0, ctx->stream, w->d_C.p, (uint32_t)w->nlist, g.L, w->d_nrank.p,
                       w->d_dstab.p);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// ---- build: the stages wt_build_begin .. wt_build_finish over one WtBuildCall
// offsets: host array (vidc_wt_build), or NULL and d_offsets + ntotal (vidc_wt_build_dev: copied into d_C and validated by
// k_offsets_ingest, whose summary is read at the build's wait for the verdict on the ids, before any level is built)
struct WtBuildIn {
    vidc_ctx *ctx;
    uint64_t nlist;
    const uint64_t *offsets, *d_offsets;
    uint64_t ntotal;  // (device offsets)
    const uint64_t *d_ids;
    int wt_type;
    WtBuildPolicy pol;
};
struct WtBuildCall : WtBuildIn {
    explicit WtBuildCall(const WtBuildIn &in) : WtBuildIn(in), t(in.ctx) {}
    std::unique_ptr<vidc_wt> w;  // the object under construction
    WtGeom g{};
    WtBuildPlan plan;
    RrrTab tab;
    Pinned h_dsum;  // device offsets: the ingest's summary
    Scratch s_a, s_b, s_err, s_lvl_bits, s_lvl_rank, s_width, s_bitpos, s_scan, s_offs_tmp, s_part, s_state;
    EventTimer t;
    uint32_t *cur = nullptr, *nxt = nullptr;  // the level's order and the next one's
    std::vector<uint64_t> lvl_bits;           // wt_type 1: bits of every level's offset stream
    bool rrr() const { return g.wt_type == 1; }  // (keeps one level of plain bits at a time, scratch, and the RRR coding of every level)
};

static int wt_build_shape(uint64_t nlist, uint64_t ntotal, int wt_type) {
    switch (wt_shape_check(nlist, ntotal, wt_type)) {
    case WT_SHAPE_OK: return VIDC_OK;
    case WT_SHAPE_TYPE: return VIDC_ERR_INVALID;
    case WT_SHAPE_NLIST: set_error("wavelet tree needs 1 <= nlist < 2^32"); return VIDC_ERR_INVALID;
    default: set_error("wavelet tree: ntotal must be < 2^32"); return VIDC_ERR_UNSUPPORTED;
    }
}

// checks, geometry and plan, the object and its arrays
static int wt_build_begin(WtBuildCall &c) {
    VIDC_TRY(wt_build_shape(c.nlist, 0, c.wt_type));  // (nlist first: ntotal is read behind nlist offsets)
    VIDC_HIP(hipSetDevice(c.ctx->device));
    const uint64_t nt = c.offsets ? c.offsets[c.nlist] : c.ntotal;
    if (nt && !c.d_ids && !c.offsets) return VIDC_ERR_INVALID;
    VIDC_TRY(wt_build_shape(c.nlist, nt, c.wt_type));
    c.g = wt_geom(c.nlist, nt, c.wt_type);
    c.plan = wt_build_plan(c.g, c.nlist, c.pol);
    c.w.reset(new vidc_wt());
    if (c.offsets) c.w->offsets.assign(c.offsets, c.offsets + c.nlist + 1);
    else c.w->offsets_host = false;
    if (c.rrr()) c.tab = rrr_tab();
    c.lvl_bits.assign(c.g.L, 0);
    return wt_object_alloc(c.ctx, c.w.get(), c.nlist, c.g);
}

// the symbol start table: copied from the host, or ingested from the device
static int wt_build_ingest_offsets(WtBuildCall &c) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    if (c.offsets) {
        VIDC_HIP(hipMemcpyAsync(w->d_C.p, w->offsets.data(), c.g.C_n * 8, hipMemcpyHostToDevice, ctx->stream));
        return VIDC_OK;
    }
    unsigned long long *acc = nullptr;
    VIDC_TRY(doff_block(ctx, &acc));
    VIDC_TRY(c.h_dsum.get(ctx, sizeof(DevOffSummary)));
    c.h_dsum.as<DevOffSummary>()->done = 0;
    hipLaunchKernelGGL(k_offsets_ingest, dim3(doff_grid(c.nlist)), dim3(256), 0, ctx->stream, c.d_offsets, w->d_C.p, c.nlist, w->ntotal, 0u,
                       0u, ~0ull, acc, acc + DOFF_NACC, c.h_dsum.as<DevOffSummary>());
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// the scratch of the call; what has to be zero is cleared, the RRR tables go up
static int wt_build_alloc(WtBuildCall &c) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    const WtBuildPlan &pl = c.plan;
    if (!c.rrr()) {
        VIDC_HIP(hipMemsetAsync(w->d_bits.p, 0, c.g.bits_n * 8, ctx->stream));
    } else {
        VIDC_HIP(hipMemsetAsync(w->d_cls.p, 0, c.g.cls_n * 4, ctx->stream));
        VIDC_TRY(c.s_lvl_bits.get(ctx, pl.lvl_bits_n * 8));
        VIDC_TRY(c.s_lvl_rank.get(ctx, pl.lvl_rank_n * 4));
        VIDC_TRY(c.s_width.get(ctx, pl.width_n * 4));
        VIDC_TRY(c.s_bitpos.get(ctx, pl.bitpos_n * 8));
        VIDC_TRY(c.s_offs_tmp.get(ctx, (size_t)pl.offs_tmp_n * 8));
        VIDC_HIP(hipMemsetAsync(c.s_offs_tmp.p, 0, (size_t)pl.offs_tmp_n * 8, ctx->stream));
        VIDC_TRY(wt_rrr_tables(ctx, w, c.tab));
    }
    VIDC_HIP(hipMemsetAsync(w->d_nrank.p, 0, c.g.nrank_n * 4, ctx->stream));
    VIDC_TRY(c.s_a.get(ctx, pl.syms_n * 4));
    VIDC_TRY(c.s_b.get(ctx, pl.syms_n * 4));
    VIDC_TRY(c.s_err.get(ctx, 4));
    VIDC_HIP(hipMemsetAsync(c.s_err.p, 0, 4, ctx->stream));
    if (!pl.part2) VIDC_HIP(hipMemsetAsync(c.s_a.p, 0xff, pl.syms_n * 4, ctx->stream));  // (k_wt_check_syms looks for slots nobody wrote)
    else VIDC_TRY(c.s_part.get(ctx, (size_t)pl.part_n * 4));
    VIDC_TRY(c.s_state.get(ctx, (size_t)pl.state_n * 8));
    c.cur = c.s_a.as<uint32_t>();
    c.nxt = c.s_b.as<uint32_t>();
    return VIDC_OK;
}

// list_nos[id] into s_a: partition + place, or the direct scatter and its check
static int wt_build_symbols(WtBuildCall &c) {
    vidc_ctx *ctx = c.ctx;
    const WtBuildPlan &pl = c.plan;
    const uint64_t nt = c.g.ntotal;
    const uint64_t *C = c.w->d_C.p;
    uint32_t *syms = c.s_a.as<uint32_t>(), *err = c.s_err.as<uint32_t>();
    VIDC_HIP(c.t.start());
    if (pl.part2) {
        uint32_t *part = c.s_part.as<uint32_t>(), *tot = part + (size_t)VIDC_WTP_NBLK * VIDC_WTP_MAXB, *bstart = tot + VIDC_WTP_MAXB;
        uint32_t *pairs = c.s_b.as<uint32_t>();  // (the second symbol array is free until the first level has run)
        hipLaunchKernelGGL(k_wt_part_hist, dim3(VIDC_WTP_NBLK), dim3(256), 0, ctx->stream, c.d_ids, nt, part);
        hipLaunchKernelGGL(k_wt_part_scan, dim3(VIDC_WTP_MAXB / 64), dim3(64), 0, ctx->stream, part, tot);
        hipLaunchKernelGGL(k_wt_part_scatter, dim3(VIDC_WTP_NBLK), dim3(256), 0, ctx->stream, c.d_ids, C, (uint32_t)c.nlist, nt, part, tot,
                           bstart, pairs, err);
        hipLaunchKernelGGL(k_wt_part_place, dim3(pl.nbuckets), dim3(256), VIDC_WTP_BUCKET * 4, ctx->stream, pairs, bstart, nt, syms, err);
        VIDC_HIP(hipGetLastError());
    } else if (nt) {
        hipLaunchKernelGGL(k_wt_scatter_syms, dim3(pl.scatter_grid), dim3(256), 0, ctx->stream, c.d_ids, C, (uint32_t)c.nlist, nt, syms, err);
        hipLaunchKernelGGL(k_wt_check_syms, dim3(pl.check_grid), dim3(256), 0, ctx->stream, syms, nt, err);
        VIDC_HIP(hipGetLastError());
    }
    return VIDC_OK;
}

// scan states of every level's pass (zeroed once) and the node tables: queued in front of the wait for the verdict on the ids, which
// they do not depend on
static int wt_build_node_tables(WtBuildCall &c) {
    VIDC_HIP(hipMemsetAsync(c.s_state.p, 0, (size_t)c.plan.state_n * 8, c.ctx->stream));
    return wt_queue_node_tables(c.ctx, c.w.get(), c.g);
}

// the one wait in front of the levels, and what it brings back: the status of device offsets, the verdict on the ids
static int wt_build_verdict(WtBuildCall &c) {
    vidc_ctx *ctx = c.ctx;
    uint32_t err = 0;
    VIDC_HIP(hipMemcpyAsync(&err, c.s_err.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    if (!c.offsets) {  // (bad offsets were replaced by a valid split on the device: nothing above wrote outside its buffers)
        const DevOffSummary sum = *c.h_dsum.as<DevOffSummary>();  // (after the wait)
        if (!sum.done) { set_error("wavelet tree: the offsets summary was not written"); return VIDC_ERR_HIP; }
        VIDC_TRY(doff_status(sum, "wavelet tree", VIDC_ERR_INVALID));
    }
    if (err) {
        set_error("wavelet tree: ids must be a permutation of 0..ntotal-1, ascending inside every list "
                  "(asserts at custom_invlists_impl.cpp:359-360)");
        return VIDC_ERR_DOMAIN;
    }
    return VIDC_OK;
}

// wt_type 1, one level: classes -> offset widths -> bit positions (scan) -> offsets, samples; the bits of its offset stream come back
static int wt_build_rrr_level(WtBuildCall &c, uint32_t level, const uint64_t *bits, const uint32_t *rank) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    const WtGeom &g = c.g;
    const WtBuildPlan &pl = c.plan;
    uint32_t *width = c.s_width.as<uint32_t>();
    uint64_t *bitpos = c.s_bitpos.as<uint64_t>();
    uint64_t *otmp = c.s_offs_tmp.as<uint64_t>() + (size_t)level * pl.offs_tmp_per_level;
    hipLaunchKernelGGL(k_rrr_classes, dim3(pl.rrr_block_grid), dim3(256), 0, ctx->stream, bits, g.nblk, c.tab,
                       w->d_cls.p + (uint64_t)level * g.cls_wpl, width);
    VIDC_TRY(device_exscan(ctx, width, (uint32_t)g.nblk, bitpos, c.s_scan));
    hipLaunchKernelGGL(k_rrr_offsets, dim3(pl.rrr_block_grid), dim3(256), 0, ctx->stream, bits, g.nblk, c.tab, w->d_binom.p, bitpos,
                       (unsigned long long *)otmp);
    hipLaunchKernelGGL(k_rrr_samples, dim3(pl.rrr_sample_grid), dim3(256), 0, ctx->stream, bits, rank, g.ntotal, g.nblk, g.nsamp, bitpos,
                       w->d_ptr.p + (uint64_t)level * (g.nsamp + 1), w->d_rs.p + (uint64_t)level * (g.nsamp + 1));
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(hipMemcpyAsync(&c.lvl_bits[level], bitpos + g.nblk, 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch of the level is reused by the next one)
    return VIDC_OK;
}

// one level: its bits, rank directory and the next level's order in one pass; then its RRR coding
static int wt_build_level(WtBuildCall &c, uint32_t level) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    const WtGeom &g = c.g;
    const bool rrr = c.rrr(), last = level + 1 == g.L;
    uint64_t *bits = rrr ? c.s_lvl_bits.as<uint64_t>() : w->d_bits.p + (uint64_t)level * g.words_per_level;
    uint32_t *rank = rrr ? c.s_lvl_rank.as<uint32_t>() : w->d_rank.p + (uint64_t)level * (g.blocks_per_level + 1);
    if (rrr) VIDC_HIP(hipMemsetAsync(bits, 0, g.words_per_level * 8, ctx->stream));
    unsigned long long *st = c.s_state.as<unsigned long long>() + (size_t)level * g.state_per_level;
    hipLaunchKernelGGL(k_wt_level, dim3(g.level_tiles), dim3(256), 0, ctx->stream, c.cur, last ? (uint32_t *)nullptr : c.nxt, g.ntotal,
                       (uint32_t)c.nlist, g.L, level, w->d_dstab.p + 2 * wt_nrank_base(level), bits, g.words_per_level, rank,
                       g.blocks_per_level, st, g.level_tiles);
    if (!last) std::swap(c.cur, c.nxt);
    VIDC_HIP(hipGetLastError());
    return rrr ? wt_build_rrr_level(c, level, bits, rank) : VIDC_OK;
}

// wt_type 1: the offset streams at their exact size; the size; the call's last wait
static int wt_build_finish(WtBuildCall &c) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    if (c.rrr()) {
        VIDC_TRY(wt_set_offset_streams(w, c.g, c.lvl_bits.data()));
        for (uint32_t level = 0; level < c.g.L && c.g.ntotal; level++)
            VIDC_HIP(hipMemcpyAsync(w->d_offs.p + w->rrr_off_base[level], c.s_offs_tmp.as<uint64_t>() + (size_t)level * c.plan.offs_tmp_per_level,
                                    (w->rrr_off_base[level + 1] - w->rrr_off_base[level]) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    w->size_bytes = wt_size_bytes(c.g, c.nlist, c.lvl_bits.data());
    return c.t.finish();
}

static int wt_build_impl(const WtBuildIn &in, vidc_wt **out) {
    WtBuildCall c(in);
    c.pol.direct_scatter = std::getenv("VIDC_WT_SCATTER") != nullptr;
    c.pol.num_cu = in.ctx->num_cu;
    VIDC_TRY(wt_build_begin(c));
    VIDC_TRY(wt_build_ingest_offsets(c));
    VIDC_TRY(wt_build_alloc(c));
    VIDC_TRY(wt_build_symbols(c));
    VIDC_TRY(wt_build_node_tables(c));
    VIDC_TRY(wt_build_verdict(c));
    for (uint32_t level = 0; level < c.g.L && c.g.ntotal; level++) VIDC_TRY(wt_build_level(c, level));
    VIDC_TRY(wt_build_finish(c));
    *out = c.w.release();
    return VIDC_OK;
}

// ---- bulk decode: one level of a compressed tree back as plain bits + rank directory (scratch), each block unranked once
static int wt_decode_expand_level(vidc_ctx *ctx, const vidc_wt *w, const WtDecodePlan &pl, uint32_t level, uint64_t *bits, uint32_t *rank) {
    const BvRrr rv = rrr_view_level(w, level);
    VIDC_HIP(hipMemsetAsync(bits, 0, pl.lvl_bits_n * 8, ctx->stream));
    hipLaunchKernelGGL(k_rrr_expand, dim3(pl.expand_grid), dim3(256), 0, ctx->stream, rv, (unsigned long long *)bits);
    hipLaunchKernelGGL(k_rrr_rankdir, dim3(pl.rankdir_grid), dim3(256), 0, ctx->stream, rv, w->blocks_per_level, rank);
    return VIDC_OK;
}

// ---- import: the stages over one WtImportCall, behind the host verdict (wt_import_host_verdict)
struct WtImportIn {  // (the arrays' word counts are checked by the host verdict and not needed behind it)
    vidc_ctx *ctx;
    uint64_t nlist;
    const uint64_t *offsets;
    int wt_type;
    const uint64_t *bits;
    const uint32_t *cls;
    const uint64_t *offs, *off_bits;
};
struct WtImportCall : WtImportIn {
    explicit WtImportCall(const WtImportIn &in) : WtImportIn(in), guard(in.ctx), t(in.ctx) {}
    std::unique_ptr<vidc_wt> w;
    WtGeom g{};
    WtImportPlan plan;
    Scratch s_sum, s_sum2, s_scan, s_scan2, s_tmp, s_tmp2, s_err;
    StreamGuard guard;  // (behind the blocks: an early return waits before they go back to the pool)
    EventTimer t;
    double kernel_ms_before = 0;
    unsigned long long *d_err = nullptr;  // the error word of the device checks
    uint64_t *d_tot = nullptr;            // the levels' width totals
    bool rrr() const { return g.wt_type == 1; }
};

// the verdict of wt_image_check as the call's message and status
static int wt_import_host_verdict(const WtImportIn &in, uint64_t n_bits, uint64_t n_cls, uint64_t n_offs) {
    const WtImageVerdict v = wt_image_check(in.nlist, in.offsets, in.wt_type, in.bits, n_bits, in.cls, n_cls, in.offs, n_offs, in.off_bits);
    const unsigned long long a = v.a, b = v.b;
    switch (v.kind) {
    case WT_IMG_OK: return VIDC_OK;
    case WT_IMG_TYPE: set_error("wt import: wt_type must be 0 or 1, not %d", in.wt_type); break;
    case WT_IMG_NLIST: set_error("wt import: nlist must be 1 <= nlist < 2^32"); break;
    case WT_IMG_OFFSETS_START: set_error("wt import: offsets[0] must be 0"); break;
    case WT_IMG_OFFSETS_ORDER: set_error("wt import: offsets decrease at list %llu", a); break;
    case WT_IMG_NTOTAL: set_error("wt import: offsets: ntotal must be < 2^32"); return VIDC_ERR_UNSUPPORTED;
    case WT_IMG_N_BITS: set_error("wt import: n_bits = %llu, the offsets need %llu words", a, b); break;
    case WT_IMG_PLAIN_EXTRA: set_error("wt import: n_cls and n_offs must be 0 for wt_type 0"); break;
    case WT_IMG_BITS_STRAY: set_error("wt import: bits: level %u has a bit set behind position ntotal", v.level); break;
    case WT_IMG_RRR_EXTRA: set_error("wt import: n_bits must be 0 for wt_type 1"); break;
    case WT_IMG_N_CLS: set_error("wt import: n_cls = %llu, the offsets need %llu words", a, b); break;
    case WT_IMG_OFF_BITS_NULL: set_error("wt import: off_bits is NULL"); break;
    case WT_IMG_OFF_BITS_MAX: set_error("wt import: off_bits[%u] = %llu exceeds 61 bits per block", v.level, a); break;
    case WT_IMG_N_OFFS: set_error("wt import: n_offs = %llu, off_bits needs %llu words", a, b); break;
    case WT_IMG_CLS_STRAY: set_error("wt import: cls: level %u has a class field behind its last block", v.level); break;
    case WT_IMG_OFFS_STRAY: set_error("wt import: offs: level %u has a bit set behind off_bits", v.level); break;
    }
    return VIDC_ERR_INVALID;
}

// the object and its arrays; the image copied in, every pad word zero
static int wt_import_object(WtImportCall &c) {
    vidc_ctx *ctx = c.ctx;
    const WtGeom &g = c.g = wt_geom(c.nlist, c.offsets[c.nlist], c.wt_type);
    c.plan = wt_import_plan(g, ctx->num_cu);
    c.w.reset(new vidc_wt());
    vidc_wt *w = c.w.get();
    w->offsets.assign(c.offsets, c.offsets + c.nlist + 1);
    VIDC_TRY(wt_object_alloc(ctx, w, c.nlist, g));
    VIDC_TRY(c.s_err.get(ctx, (size_t)c.plan.err_n * 8));
    c.d_err = c.s_err.as<unsigned long long>();
    c.d_tot = c.s_err.as<uint64_t>() + 1;
    if (c.rrr()) {
        VIDC_TRY(wt_set_offset_streams(w, g, c.off_bits));
        VIDC_TRY(wt_rrr_tables(ctx, w, rrr_tab()));
    }
    // the pad words (one behind every level's bits; two class words and one offset word behind every level's RRR coding): everything
    // else is overwritten by the copies
    for (uint32_t l = 0; l < g.L; l++) {
        if (!c.rrr()) VIDC_HIP(hipMemsetAsync(w->d_bits.p + (uint64_t)l * g.words_per_level + g.W, 0, 8, ctx->stream));
        else {
            VIDC_HIP(hipMemsetAsync(w->d_cls.p + (uint64_t)l * g.cls_wpl + g.cls_img_wpl, 0, 8, ctx->stream));
            VIDC_HIP(hipMemsetAsync(w->d_offs.p + w->rrr_off_base[l + 1] - 1, 0, 8, ctx->stream));
        }
    }
    VIDC_HIP(hipEventRecord(ctx->tev[0], ctx->stream));
    VIDC_HIP(hipMemcpyAsync(w->d_C.p, c.offsets, g.C_n * 8, hipMemcpyHostToDevice, ctx->stream));
    uint64_t at = 0;
    for (uint32_t l = 0; l < g.L; l++) {
        if (!c.rrr()) {
            if (g.W) VIDC_HIP(hipMemcpyAsync(w->d_bits.p + (uint64_t)l * g.words_per_level, c.bits + (uint64_t)l * g.W, g.W * 8, hipMemcpyHostToDevice, ctx->stream));
            continue;
        }
        if (g.nsamp) VIDC_HIP(hipMemcpyAsync(w->d_cls.p + (uint64_t)l * g.cls_wpl, c.cls + (uint64_t)l * g.cls_img_wpl, g.cls_img_wpl * 4, hipMemcpyHostToDevice, ctx->stream));
        const uint64_t ow = wt_words(c.off_bits[l]);
        if (ow) VIDC_HIP(hipMemcpyAsync(w->d_offs.p + w->rrr_off_base[l], c.offs + at, ow * 8, hipMemcpyHostToDevice, ctx->stream));
        at += ow;
    }
    VIDC_HIP(hipEventRecord(ctx->tev[1], ctx->stream));
    return VIDC_OK;
}

// the error word, and the node tables from the offsets alone
static int wt_import_node_tables(WtImportCall &c) {
    VIDC_HIP(c.t.start());
    VIDC_HIP(hipMemsetAsync(c.d_err, 0xff, 8, c.ctx->stream));
    VIDC_HIP(hipMemsetAsync(c.w->d_nrank.p, 0, c.g.nrank_n * 4, c.ctx->stream));
    return wt_queue_node_tables(c.ctx, c.w.get(), c.g);
}

template <class View>
static int wt_import_check_nodes(WtImportCall &c, const View &vw) {
    const vidc_wt *w = c.w.get();
    hipLaunchKernelGGL(k_wt_imp_check_nodes<View>, dim3(c.plan.node_grid, c.g.L), dim3(256), 0, c.ctx->stream, vw, w->d_C.p, w->d_nrank.p,
                       (uint32_t)c.nlist, c.g.L, c.d_err);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// wt_type 0, the rank directory: ones of every 512-bit block, one scan over the levels back to back, per-level prefixes; the node check
static int wt_import_rank_dir(WtImportCall &c) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    const WtGeom &g = c.g;
    const WtImportPlan &pl = c.plan;
    VIDC_TRY(c.s_sum.get(ctx, pl.sum_n * 4));
    VIDC_TRY(c.s_scan.get(ctx, pl.scan_n * 8));
    hipLaunchKernelGGL(k_wt_imp_block_ones, dim3(pl.ones_grid, g.L), dim3(256), 0, ctx->stream, w->d_bits.p, g.words_per_level, g.blocks_per_level,
                       c.s_sum.as<uint32_t>());
    VIDC_TRY(device_exscan(ctx, c.s_sum.as<uint32_t>(), (uint32_t)(g.L * pl.per_level), c.s_scan.as<uint64_t>(), c.s_tmp));
    hipLaunchKernelGGL(k_wt_imp_level_prefix, dim3(pl.prefix_grid, g.L), dim3(256), 0, ctx->stream, c.s_scan.as<uint64_t>(), pl.per_level, w->d_rank.p,
                       (uint64_t *)nullptr);
    return wt_import_check_nodes(c, plain_view(w));
}

// wt_type 1, the samples: sums of the classes and of their widths per sample, two scans, per-level prefixes; the levels' width totals
// are compared with off_bits before anything reads an offset stream; then the block check and the node check
static int wt_import_samples(WtImportCall &c) {
    vidc_ctx *ctx = c.ctx;
    vidc_wt *w = c.w.get();
    const WtGeom &g = c.g;
    const WtImportPlan &pl = c.plan;
    const uint32_t n = (uint32_t)(g.L * pl.per_level);
    VIDC_TRY(c.s_sum.get(ctx, pl.sum_n * 4));
    VIDC_TRY(c.s_sum2.get(ctx, pl.sum_n * 4));
    VIDC_TRY(c.s_scan.get(ctx, pl.scan_n * 8));
    VIDC_TRY(c.s_scan2.get(ctx, pl.scan_n * 8));
    if (g.nsamp)
        hipLaunchKernelGGL(k_wt_imp_sample_sums, dim3(pl.sums_grid, g.L), dim3(256), 0, ctx->stream, w->d_cls.p, g.cls_wpl, g.nsamp,
                           (const uint8_t *)(w->d_binom.p + 64 * 64), c.s_sum.as<uint32_t>(), c.s_sum2.as<uint32_t>());
    VIDC_TRY(device_exscan(ctx, c.s_sum.as<uint32_t>(), n, c.s_scan.as<uint64_t>(), c.s_tmp));
    VIDC_TRY(device_exscan(ctx, c.s_sum2.as<uint32_t>(), n, c.s_scan2.as<uint64_t>(), c.s_tmp2));
    const dim3 pgrid(pl.prefix_grid, g.L);
    hipLaunchKernelGGL(k_wt_imp_level_prefix, pgrid, dim3(256), 0, ctx->stream, c.s_scan.as<uint64_t>(), g.nsamp, w->d_rs.p, (uint64_t *)nullptr);
    hipLaunchKernelGGL(k_wt_imp_level_prefix, pgrid, dim3(256), 0, ctx->stream, c.s_scan2.as<uint64_t>(), g.nsamp, w->d_ptr.p, c.d_tot);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(c.t.mark());  // (the kernel time of the call is the two intervals around this read-back, not the wait between them)
    std::vector<uint64_t> tot(g.L, 0);
    VIDC_HIP(hipMemcpyAsync(tot.data(), c.d_tot, (size_t)g.L * 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    c.kernel_ms_before = c.t.elapsed();
    for (uint32_t l = 0; l < g.L; l++)
        if (tot[l] != c.off_bits[l]) {
            set_error("wt import: off_bits[%u] = %llu, the classes of the level need %llu bits", l, (unsigned long long)c.off_bits[l],
                      (unsigned long long)tot[l]);
            return VIDC_ERR_INVALID;
        }
    VIDC_HIP(c.t.start());
    if (g.nblk)
        hipLaunchKernelGGL(k_wt_imp_check_blocks, dim3(pl.blocks_grid, g.L), dim3(256), 0, ctx->stream, rrr_view(w), c.d_err);
    return wt_import_check_nodes(c, rrr_view(w));
}

// the call's last wait, the times, the verdict of the device checks, the size
static int wt_import_device_verdict(WtImportCall &c) {
    vidc_ctx *ctx = c.ctx;
    unsigned long long err = 0;
    VIDC_HIP(hipMemcpyAsync(&err, c.d_err, 8, hipMemcpyDeviceToHost, ctx->stream));
    c.guard.disarm();
    VIDC_TRY(c.t.finish());
    ctx->last_kernel_ms += c.kernel_ms_before;
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->tev[0], ctx->tev[1]) == hipSuccess) ctx->phase_ms[VIDC_PHASE_IMPORT_H2D] = ms;
    }
    if (err != ~0ull) {
        const uint32_t level = (uint32_t)(err >> 56) & 0x7fu, kind = (uint32_t)(err & 0xffu);
        const unsigned long long idx = (err >> 8) & 0xffffffffffffull;
        if (kind == VIDC_WT_IMP_NODE)
            set_error("wt import: the image does not match the offsets: ones before node %llu of level %u differ", idx, level);
        else
            set_error("wt import: %s: block %llu of level %u %s", kind == VIDC_WT_IMP_OFFSET ? "offs" : "cls", idx, level,
                      kind == VIDC_WT_IMP_OFFSET ? "has an offset >= C(63, class)"
                      : kind == VIDC_WT_IMP_CLASS ? "has a class above the number of its bits" : "has a one behind the end of the level");
        return VIDC_ERR_INVALID;
    }
    c.w->size_bytes = wt_size_bytes(c.g, c.nlist, c.off_bits);
    return VIDC_OK;
}

static int wt_ensure_offsets(const vidc_wt *w) { return ensure_offsets_host(w, w->d_C.p); }

extern "C" {

int vidc_wt_build(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, int wt_type,
                  vidc_wt **out) {
    if (!ctx || !out || (nlist && !offsets) || (wt_type != 0 && wt_type != 1)) return VIDC_ERR_INVALID;
    *out = nullptr;
    return wt_build_impl(WtBuildIn{ctx, nlist, offsets, nullptr, 0, d_ids, wt_type, WtBuildPolicy{}}, out);
}

int vidc_wt_build_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids, int wt_type,
                      vidc_wt **out) {
    if (!ctx || !out || !d_offsets || (wt_type != 0 && wt_type != 1)) return VIDC_ERR_INVALID;
    *out = nullptr;
    if (!wt_ntotal_ok(ntotal)) return wt_build_shape(1, ntotal, wt_type);  // (in front of the refusal of nlist)
    return wt_build_impl(WtBuildIn{ctx, nlist, nullptr, d_offsets, ntotal, d_ids, wt_type, WtBuildPolicy{}}, out);
}

int vidc_wt_offsets(vidc_ctx *ctx, const vidc_wt *w, uint64_t *offsets) {
    if (!ctx || !w || !offsets) return VIDC_ERR_INVALID;
    VIDC_TRY(wt_ensure_offsets(w));
    std::memcpy(offsets, w->offsets.data(), (w->nlist + 1) * 8);
    return VIDC_OK;
}

void vidc_wt_destroy(vidc_wt *w) { delete w; }
uint64_t vidc_wt_size_in_bytes(const vidc_wt *w) { return w ? w->size_bytes : 0; }
uint32_t vidc_wt_levels(const vidc_wt *w) { return w ? w->L : 0; }

int vidc_wt_select(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, const uint64_t *offs,
                   int64_t *ids_out) {
    if (!ctx || !w || (m && (!list_nos || !offs || !ids_out))) return VIDC_ERR_INVALID;
    if (!m) return VIDC_OK;
    VIDC_TRY(wt_ensure_offsets(w));
    return get_request(ctx, "wt select", w->nlist, w->offsets, m, list_nos, offs, ids_out, [&](const uint64_t *d_l, const uint64_t *d_o, int64_t *d_r) {
        const dim3 sgrid((uint32_t)std::min<uint64_t>((m + 127) / 128, 1u << 16));
        if (w->wt_type == 1)
            hipLaunchKernelGGL(k_wt_select<WtRrrView>, sgrid, dim3(128), 0, ctx->stream, rrr_view(w), w->d_C.p, w->d_nrank.p, (uint32_t)w->nlist,
                               w->L, m, d_l, d_o, d_r);
        else
            hipLaunchKernelGGL(k_wt_select<WtPlainView>, sgrid, dim3(128), 0, ctx->stream, plain_view(w), w->d_C.p, w->d_nrank.p,
                               (uint32_t)w->nlist, w->L, m, d_l, d_o, d_r);
    });
}

int vidc_wt_translate_labels_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                 uint64_t *d_invalid) {
    VIDC_TRY(req_check_labels(ctx, w, n, d_labels, d_ids));
    if (!n) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const dim3 sgrid((uint32_t)std::min<uint64_t>((n + 127) / 128, 1u << 16));
    const uint64_t *lab = (const uint64_t *)d_labels;
    unsigned long long *inv = (unsigned long long *)d_invalid;
    if (w->wt_type == 1)
        hipLaunchKernelGGL((k_wt_select<WtRrrView, true>), sgrid, dim3(128), 0, ctx->stream, rrr_view(w), w->d_C.p, w->d_nrank.p,
                           (uint32_t)w->nlist, w->L, n, lab, (const uint64_t *)nullptr, d_ids, inv);
    else
        hipLaunchKernelGGL((k_wt_select<WtPlainView, true>), sgrid, dim3(128), 0, ctx->stream, plain_view(w), w->d_C.p, w->d_nrank.p,
                           (uint32_t)w->nlist, w->L, n, lab, (const uint64_t *)nullptr, d_ids, inv);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// Locate (include/vidc.h): one walk from the root per pair (k_wt_locate), over the tables the select calls use.  Enqueue only, like
// vidc_wt_translate_labels_dev: no scratch, no wait, vidc_ctx_last_kernel_ms is left alone.
int vidc_wt_locate_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, int64_t *d_labels,
                       uint64_t *d_missing, uint64_t *d_invalid) {
    if (!ctx || !w || (n && (!d_ids || !d_labels))) {
        set_error("wt locate: NULL context, object, id or label array");
        return VIDC_ERR_INVALID;
    }
    if (n >= 0xffffffffull) { set_error("wt locate: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    if (!n) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const dim3 sgrid((uint32_t)std::min<uint64_t>((n + 127) / 128, 1u << 16));
    unsigned long long *mis = (unsigned long long *)d_missing, *inv = (unsigned long long *)d_invalid;
    if (w->wt_type == 1)
        hipLaunchKernelGGL(k_wt_locate<WtRrrView>, sgrid, dim3(128), 0, ctx->stream, rrr_view(w), w->d_C.p, w->d_nrank.p, (uint32_t)w->nlist, w->L,
                           w->ntotal, n, d_list_nos, d_ids, d_labels, mis, inv);
    else
        hipLaunchKernelGGL(k_wt_locate<WtPlainView>, sgrid, dim3(128), 0, ctx->stream, plain_view(w), w->d_C.p, w->d_nrank.p, (uint32_t)w->nlist,
                           w->L, w->ntotal, n, d_list_nos, d_ids, d_labels, mis, inv);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// Append (include/vidc.h): decode_all into scratch, the shared merge (append.h), vidc_wt_build_dev on the merged CSR -- which checks
// what the reference asserts of it (a permutation of 0 .. ntotal - 1, ascending inside every list).
int vidc_wt_append_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids, vidc_wt **out,
                       int64_t *d_labels, uint64_t *d_invalid) {
    VIDC_TRY(append_check(ctx, w, out, n_add, d_list_nos, d_ids));
    VIDC_HIP(hipSetDevice(ctx->device));
    AppendMerged m;
    VIDC_TRY(append_merge(ctx, w->nlist, w->ntotal, w->d_C.p, n_add, d_list_nos, d_ids, d_labels, d_invalid, true, m,
                          [&](uint64_t *d) { return vidc_wt_decode_all(ctx, w, d); }));
    return vidc_wt_build_dev(ctx, w->nlist, m.batch.new_off, m.ntotal_new, m.s_merged.as<uint64_t>(), w->wt_type, out);
}

// Merge (include/vidc.h): decode_all of both objects into scratch, the placement of merge.h, vidc_wt_build_dev on the merged CSR with
// a's wt_type -- which checks what the reference asserts of it (add_id = ntotal(a) makes it so).  d_src of this container (ascending
// lists, and M_l must be ascending) is arithmetic on the three offset arrays.
int vidc_wt_merge_dev(vidc_ctx *ctx, const vidc_wt *a, const vidc_wt *b, uint64_t add_id, vidc_wt **out, int64_t *d_src) {
    VIDC_TRY(merge_check(ctx, a, b, out));
    VIDC_HIP(hipSetDevice(ctx->device));
    MergeRebuilt m;
    VIDC_TRY(merge_rebuild(ctx, a->nlist, a->ntotal, b->ntotal, a->d_C.p, b->d_C.p, add_id, a == b, m,
                           [&](uint64_t *d) { return vidc_wt_decode_all(ctx, a, d); }, [&](uint64_t *d) { return vidc_wt_decode_all(ctx, b, d); }));
    vidc_wt *nw = nullptr;
    VIDC_TRY(vidc_wt_build_dev(ctx, a->nlist, m.new_off, m.ntotal_new, m.s_merged.as<uint64_t>(), a->wt_type, &nw));
    double kernel_ms = m.kernel_ms + ctx->last_kernel_ms;
    const int st = merge_write_src(ctx, a->nlist, m.ntotal_new, a->d_C.p, b->d_C.p, nw->d_C.p, nullptr, nullptr, nullptr, d_src, kernel_ms);
    if (st != VIDC_OK) { delete nw; return st; }
    ctx->last_kernel_ms = kernel_ms;
    *out = nw;
    return VIDC_OK;
}

int vidc_wt_decode_lists(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                         uint64_t *out_offsets) {
    if (!ctx || !w || (m && !list_nos) || !out_offsets) return VIDC_ERR_INVALID;
    VIDC_TRY(wt_ensure_offsets(w));
    VIDC_TRY(lists_request_offsets(w->nlist, w->offsets, m, list_nos, out_offsets));
    const uint64_t total = out_offsets[m];
    ctx->last_kernel_ms = 0;
    if (!total) return VIDC_OK;
    if (!d_out) return VIDC_ERR_INVALID;
    VIDC_HIP(hipSetDevice(ctx->device));
    Scratch s_l, s_o;
    VIDC_TRY(s_l.get(ctx, m * 8)); VIDC_TRY(s_o.get(ctx, (m + 1) * 8));
    VIDC_HIP(hipMemcpyAsync(s_l.p, list_nos, m * 8, hipMemcpyHostToDevice, ctx->stream));
    VIDC_HIP(hipMemcpyAsync(s_o.p, out_offsets, (m + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    const dim3 dgrid((uint32_t)std::min<uint64_t>((total + 127) / 128, 1u << 16));
    if (w->wt_type == 1)
        hipLaunchKernelGGL(k_wt_decode_lists<WtRrrView>, dgrid, dim3(128), 0, ctx->stream, rrr_view(w), w->d_C.p, w->d_nrank.p, (uint32_t)w->nlist, w->L, m,
                           s_l.as<uint64_t>(), s_o.as<uint64_t>(), total, d_out);
    else
        hipLaunchKernelGGL(k_wt_decode_lists<WtPlainView>, dgrid, dim3(128), 0, ctx->stream, plain_view(w), w->d_C.p, w->d_nrank.p, (uint32_t)w->nlist, w->L, m,
                           s_l.as<uint64_t>(), s_o.as<uint64_t>(), total, d_out);
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());
    return VIDC_OK;
}

int vidc_wt_decode_gather(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                          const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out) {
    if (!ctx || !w) return VIDC_ERR_INVALID;
    VIDC_TRY(wt_ensure_offsets(w));
    return vidc_decode_gather_impl(ctx, w->nlist, m, list_nos, n_items, item_slot, item_off, ids_out,
                                   [&](uint64_t l) { return w->offsets[l + 1] - w->offsets[l]; },
                                   [&](uint64_t *d, uint64_t *lo) { return vidc_wt_decode_lists(ctx, w, m, list_nos, d, lo); });
}

int vidc_wt_decode_all(vidc_ctx *ctx, const vidc_wt *w, uint64_t *d_out) {
    if (!ctx || !w || (w->ntotal && !d_out)) return VIDC_ERR_INVALID;
    if (!w->ntotal) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const WtDecodePlan pl = wt_decode_plan(wt_geom_of(w), ctx->num_cu);
    Scratch s_a, s_b;        // ping-pong (id, symbol prefix) arrays
    Scratch s_bits, s_rank;  // wt_type 1: one level as plain bits + rank directory
    EventTimer t(ctx);
    VIDC_HIP(t.start());
    if (w->wt_type == 1) {
        VIDC_TRY(s_bits.get(ctx, pl.lvl_bits_n * 8));
        VIDC_TRY(s_rank.get(ctx, pl.lvl_rank_n * 4));
    }
    if (pl.item_arrays > 0) VIDC_TRY(s_a.get(ctx, pl.items_n * sizeof(WtItem)));
    if (pl.item_arrays > 1) VIDC_TRY(s_b.get(ctx, pl.items_n * sizeof(WtItem)));
    const WtItem *in = nullptr;
    for (uint32_t level = 0; level < w->L; level++) {
        const bool last = level + 1 == w->L;
        WtItem *out = last ? nullptr : ((level & 1u) ? s_b.as<WtItem>() : s_a.as<WtItem>());
        uint64_t *oid = last ? d_out : nullptr;
        const uint64_t *bits = s_bits.as<uint64_t>();
        const uint32_t *rank = s_rank.as<uint32_t>();
        if (w->wt_type == 1) {
            VIDC_TRY(wt_decode_expand_level(ctx, w, pl, level, s_bits.as<uint64_t>(), s_rank.as<uint32_t>()));
        } else {
            bits = w->d_bits.p + (uint64_t)level * w->words_per_level;
            rank = w->d_rank.p + (uint64_t)level * (w->blocks_per_level + 1);
        }
        const uint32_t *dt = w->d_dstab.p + 2 * wt_nrank_base(level);
        if (last) hipLaunchKernelGGL(k_wt_decode_tile<true>, dim3(pl.tile_grid), dim3(256), 0, ctx->stream, in, out, oid, bits, w->words_per_level, rank,
                                     dt, w->ntotal);
        else hipLaunchKernelGGL(k_wt_decode_tile<false>, dim3(pl.tile_grid), dim3(256), 0, ctx->stream, in, out, oid, bits, w->words_per_level, rank,
                                dt, w->ntotal);
        in = out;
    }
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());  // (waits: the scratch of the levels goes back to the pool when the call returns)
    return VIDC_OK;
}

// ---- flat images (include/vidc.h): what is stored is the level bits, or the RRR classes and offset streams; the rank directory, the
// samples and the node tables are rebuilt on import
int vidc_wt_type(const vidc_wt *w) { return w ? w->wt_type : -1; }

int vidc_wt_image_words(const vidc_wt *w, uint64_t *n_bits, uint64_t *n_cls, uint64_t *n_offs) {
    if (!w) { set_error("wt image_words: NULL object"); return VIDC_ERR_INVALID; }
    const WtImageWords iw = wt_image_words(wt_geom_of(w), w->rrr_off_bits.data());
    if (n_bits) *n_bits = iw.n_bits;
    if (n_cls) *n_cls = iw.n_cls;
    if (n_offs) *n_offs = iw.n_offs;
    return VIDC_OK;
}

int vidc_wt_export_all(vidc_ctx *ctx, const vidc_wt *w, uint64_t *bits, size_t bits_cap, uint32_t *cls, size_t cls_cap, uint64_t *offs,
                       size_t offs_cap, uint64_t *off_bits) {
    if (!ctx || !w) { set_error("wt export_all: NULL context or object"); return VIDC_ERR_INVALID; }
    const WtGeom g = wt_geom_of(w);
    const WtImageWords iw = wt_image_words(g, w->rrr_off_bits.data());
    if (iw.n_bits > bits_cap || iw.n_cls > cls_cap || iw.n_offs > offs_cap) { set_error("wt export_all: export buffer too small"); return VIDC_ERR_INVALID; }
    if ((iw.n_bits && !bits) || (iw.n_cls && !cls) || (iw.n_offs && !offs) || (w->wt_type == 1 && !off_bits)) {
        set_error("wt export_all: NULL array");
        return VIDC_ERR_INVALID;
    }
    VIDC_HIP(hipSetDevice(w->device));
    StreamGuard guard(ctx);
    if (w->wt_type == 0) {
        for (uint32_t l = 0; l < g.L && g.W; l++)  // (without the level's pad word)
            VIDC_HIP(hipMemcpyAsync(bits + (uint64_t)l * g.W, w->d_bits.p + (uint64_t)l * g.words_per_level, g.W * 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        const uint64_t cw = g.cls_img_wpl;
        uint64_t at = 0;
        for (uint32_t l = 0; l < g.L; l++) {
            off_bits[l] = w->rrr_off_bits[l];
            if (cw) VIDC_HIP(hipMemcpyAsync(cls + (uint64_t)l * cw, w->d_cls.p + (uint64_t)l * g.cls_wpl, cw * 4, hipMemcpyDeviceToHost, ctx->stream));
            const uint64_t ow = wt_words(w->rrr_off_bits[l]);
            if (ow) VIDC_HIP(hipMemcpyAsync(offs + at, w->d_offs.p + w->rrr_off_base[l], ow * 8, hipMemcpyDeviceToHost, ctx->stream));
            at += ow;
        }
    }
    guard.disarm();
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    return VIDC_OK;
}

int vidc_wt_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, int wt_type, const uint64_t *bits, uint64_t n_bits,
                   const uint32_t *cls, uint64_t n_cls, const uint64_t *offs, uint64_t n_offs, const uint64_t *off_bits, vidc_wt **out) {
    if (out) *out = nullptr;
    if (!ctx || !out) { set_error("wt import: NULL context or out"); return VIDC_ERR_INVALID; }
    if (!offsets) { set_error("wt import: offsets is NULL"); return VIDC_ERR_INVALID; }
    const WtImportIn in{ctx, nlist, offsets, wt_type, bits, cls, offs, off_bits};
    VIDC_TRY(wt_import_host_verdict(in, n_bits, n_cls, n_offs));
    VIDC_HIP(hipSetDevice(ctx->device));
    WtImportCall c(in);
    VIDC_TRY(wt_import_object(c));
    VIDC_TRY(wt_import_node_tables(c));
    VIDC_TRY(c.rrr() ? wt_import_samples(c) : wt_import_rank_dir(c));
    VIDC_TRY(wt_import_device_verdict(c));
    *out = c.w.release();
    return VIDC_OK;
}

}  // extern "C"
