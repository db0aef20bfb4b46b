// ef_plan.h -- the deciding half of the Elias-Fano host calls (ef.hip): the per-list geometry of elias_fano.hpp:28-29, which the
// kernels share, and every choice the encoder (ef_encode_lists) and the bulk decoder (vidc_ef_decode_all) make between two launches:
// tiling, speculative stream bounds, chunk-kernel form, clearing, bulk-decode records, decode-kernel form, the three-pass path's sort
// plan.  Host code with no HIP include and nothing that touches a stream: tests/ef_plan_test.cpp builds it with g++.  ef.hip fills
// EfEncPolicy from the environment and the context at the points where it always read them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#ifndef VIDC_HD
#ifdef __HIPCC__
#define VIDC_HD __host__ __device__
#else
#define VIDC_HD
#endif
#endif

// ids per chunk record of the single-pass encoder (VIDC_EF_CHUNK: build-time experiment hook)
#ifndef VIDC_EF_CHUNK
#define VIDC_EF_CHUNK 512
#endif
#define EF_SINGLE_LISTS 1024u         // lists of the one-tile geometry kernel (512 threads, two lists each)
#define EF_SINGLE_MAX_CHUNKS 16384u   // chunk records the single-tile geometry kernel writes itself (S1: 2.4 k)
#define EF_E1_MAX_LISTS 262144u       // up to here one list per thread of a 256-thread tile, four beyond
#define EF_BIG_CHUNKS 8u              // a list of more chunks leaves the records behind its first one to k_ef_big_recs
#define EF_BATCH_BITS 4096u           // high bits per select-directory entry (64 high words)
#define EF_CLEAR_HIGH_BYTES (64ull << 20)  // high streams beyond this are cleared ahead of the chunk kernels (comment at the memset)
#define EF_ENC_RECS_MAX (1u << 18)    // objects of fewer batches: records written by the encoder, LDS table sized by the longest list

namespace vidc {
namespace dev {

constexpr uint32_t EF_CHUNK = VIDC_EF_CHUNK;

VIDC_HD inline int msb64(uint64_t x) { return 63 - __builtin_clzll(x); }

// ---- geometry of one non-empty list of m ids in the universe u (= its largest id), elias_fano.hpp:28-29
// l = msb(u / m), 0 when the quotient is 0 -- without the division: with k = msb(u) - msb(m), u / m lies in (2^(k-1), 2^(k+1)) and
// reaches 2^k exactly when (u >> k) >= m  (u < m: the quotient is 0).  tests/ef_plan_test.cpp holds it against the division.
VIDC_HD inline uint32_t ef_low_bits(uint64_t m, uint64_t u) {
    if (u < m) return 0u;
    const uint32_t k = (uint32_t)(msb64(u) - msb64(m));
    return (u >> k) >= m ? k : k - 1u;
}
struct EfGeom {
    uint64_t high_bits;   // (m + 1) + (u >> l) + 1
    uint64_t low_words;   // m * l bits + one padding word for read_bits (l = 0: the padding word alone)
    uint64_t high_words;
    uint64_t batches;     // select-directory entries: one per 64 high words
};
// (the two parts ef_make_rec takes one at a time, at the points k_ef_offsets was scheduled from: through the whole ef_list_geom the
// compiler orders that kernel's instructions differently)
VIDC_HD inline uint64_t ef_high_bits(uint64_t m, uint64_t u, uint32_t l) { return (m + 1) + (u >> l) + 1; }
VIDC_HD inline uint64_t ef_high_words(uint64_t m, uint64_t u, uint32_t l) { return (ef_high_bits(m, u, l) + 63) / 64; }
VIDC_HD inline uint64_t ef_batches_of(uint64_t high_words) { return (high_words + 63) / 64; }
VIDC_HD inline EfGeom ef_list_geom(uint64_t m, uint64_t u, uint32_t l) {
    EfGeom g;
    g.high_bits = ef_high_bits(m, u, l);
    g.low_words = (m * l + 63) / 64 + 1;
    g.high_words = ef_high_words(m, u, l);
    g.batches = ef_batches_of(g.high_words);
    return g;
}

}  // namespace dev

// ---- shared with the geometry kernels (k_ef_offsets)
struct EfLimits {  // sizes the host allocated ahead of the geometry kernels (all ~0 / wide_ok: it allocates after them)
    uint64_t low_words, high_words, nbatches;
    uint32_t wide_ok, pad;
};
struct EfSummary {  // what the host needs before it can allocate the streams
    uint64_t low_words, high_words, nbatches, nchunks, total_bits;
    uint32_t wide, unsorted;
};

// ---- encoder
struct EfEncPolicy {
    bool no_spec = false;        // VIDC_EF_NO_SPEC (once per process): always size the streams after the geometry kernels
    int memset = -1;             // VIDC_EF_MEMSET (per call): -1 unset, 1 always clear the high stream, 0 never
    bool lazy_recs = false;      // VIDC_EF_LAZY_RECS (per call): leave the bulk-decode records to the first decode_all
    uint64_t universe_hint = 0;  // largest list universe the context has met
    int num_cu = 0;
};
// spec: the streams are allocated BEFORE the geometry kernels run, by bounds that need only the list lengths and a guess of the
// largest universe (ef_spec_limits).  Geometry and chunk kernels are then queued back to back and the call waits ONCE, at its end
// (before: a wait between them for the sizes, 20-25 us of an S1-sized call's 60).  k_ef_offsets checks the exact sizes against the
// allocation on the device; if they do not fit (a universe beyond the guess, ids >= 2^32) it raises *abort, the chunk kernels return
// at once and the host, which reaches the same verdict after its wait (ef_spec_fits), runs the call again the old way.  Cost of the
// bound: the buffers are up to ~15 % larger than the streams (n_low / n_high hold the exact word counts).  Only objects whose ids can
// all be below 2^32 are tried this way.
inline bool ef_want_spec(uint64_t ntotal, const EfEncPolicy &p) { return !p.no_spec && ntotal && ntotal <= 0xffffffffull; }
// The speculative bounds need only the list lengths and a guess U of the largest universe (ids of an index are 0 .. ntotal-1 unless
// the caller numbers them himself; the context remembers a larger one it has met):
//   low  <= sum n_i msb(U / n_i) <= ntotal log2(U nlist / ntotal) bits (n log(U / n) is concave) + 2 words per list,
//   high  = (n + 1) + (u >> l) + 1 <= 3 n + 1 bits per list (u >> l < 2 n) whatever U is.
inline EfLimits ef_spec_limits(uint64_t nlist, uint64_t ntotal, uint64_t universe_hint) {
    EfLimits lim{};
    const uint64_t U = std::max<uint64_t>(ntotal ? ntotal - 1 : 0, universe_hint);
    const double ratio = ntotal ? (double)U * (double)nlist / (double)ntotal : 0.0;
    const double low_bits = ratio > 1.0 ? (double)ntotal * std::log2(ratio) * 1.0001 : 0.0;
    lim.low_words = (uint64_t)(low_bits / 64.0) + 2 * nlist + 4;
    lim.high_words = (3 * ntotal + nlist) / 64 + nlist + 2;
    lim.nbatches = lim.high_words / 64 + nlist + 2;
    lim.wide_ok = 0u;
    return lim;
}
// the verdict k_ef_offsets reaches on the device (*abort) and the host after its wait: do the exact sizes fit the allocation?
inline bool ef_spec_fits(const EfSummary &s, const EfLimits &lim) {
    return !(s.low_words > lim.low_words || s.high_words > lim.high_words || s.nbatches > lim.nbatches || (s.wide && !lim.wide_ok));
}

// (a tile = the lists of one workgroup of the geometry kernels)
struct EfEncPlan {
    // one tile only for objects whose chunk records one workgroup can write: 1024 lists of a million ids each are two million
    // records, and spreading those over the GPU is what k_ef_big_recs is for
    bool single = false;
    uint32_t tile_lists = 0, ntiles = 0, lists_per_thread = 0;
    // long lists (more than EF_BIG_CHUNKS chunks: at most nchunks / (EF_BIG_CHUNKS + 1) of them)
    uint64_t big_cap = 0;
    bool big_recs = false;   // k_ef_big_recs is queued (some list is that long; a single tile writes every record itself)
    bool spec = false, dev_forms = false;  // dev_forms: the chunk-kernel form is chosen on the device (device offsets, one wait)
    EfLimits lim{~0ull, ~0ull, ~0ull, 1u, 0u};
    uint64_t raw_n = 0, tiles_n = 0, recs_n = 0;  // scratch, in elements: per-list counts, tile totals, chunk records (+ big_cap lists)
};
// nchunks / max_list: exact from host offsets; with device offsets the bounds floor(ntotal / EF_CHUNK) + nlist and ntotal
inline EfEncPlan ef_enc_plan(uint64_t nlist, uint64_t ntotal, uint64_t nchunks, uint64_t max_list, bool dev_offsets, bool spec,
                             const EfEncPolicy &p) {
    EfEncPlan pl;
    const uint32_t nl32 = (uint32_t)nlist;
    pl.single = nl32 <= EF_SINGLE_LISTS && nchunks <= EF_SINGLE_MAX_CHUNKS;
    pl.tile_lists = pl.single ? EF_SINGLE_LISTS : (nl32 <= EF_E1_MAX_LISTS ? 256u : 1024u);
    pl.lists_per_thread = pl.single ? 2u : pl.tile_lists / 256u;
    pl.ntiles = nl32 ? (nl32 + pl.tile_lists - 1u) / pl.tile_lists : 1u;
    pl.big_cap = nchunks / (EF_BIG_CHUNKS + 1u) + 1u;
    pl.big_recs = !pl.single && max_list > (uint64_t)dev::EF_CHUNK * EF_BIG_CHUNKS;
    pl.spec = spec;
    pl.dev_forms = dev_offsets && spec;
    if (spec) pl.lim = ef_spec_limits(nlist, ntotal, p.universe_hint);
    pl.raw_n = nlist + 1;
    pl.tiles_n = pl.ntiles;
    pl.recs_n = nchunks ? nchunks : 1;
    return pl;
}

// The chunk kernel of a call.  Adding a form: one entry here, one line of ef_chunk_form, one launch in ef_enc_chunks.
enum EfChunkForm {
    EF_FORM_NONE,   // no chunk: nothing is launched
    EF_FORM_DEV,    // the three k_ef_lowhigh32_dev forms back to back; two of them return at once (counts known on the device only)
    EF_FORM_WIDE,   // some id of 2^32 or more, or a list of 2^30 ids: k_ef_lowhigh
    EF_FORM_SHORT,  // no list above 256 ids: k_ef_lowhigh32<4, SMALL>
    EF_FORM_HALF,   // chunks half full on average: <8, SMALL>
    EF_FORM_FULL    // <8>
};
inline const char *ef_chunk_form_name(EfChunkForm f) {
    static const char *const names[] = {"none", "dev", "wide", "short", "half", "full"};
    return names[f];
}
struct EfChunkLaunch { EfChunkForm form; uint32_t grid; };
inline EfChunkLaunch ef_chunk_form(uint64_t nchunks, uint64_t ntotal, uint64_t max_list, bool wide, bool dev_forms, int num_cu) {
    if (!nchunks) return {EF_FORM_NONE, 0u};
    // (device forms: 32 wavefronts per CU, looping over the chunks -- the two forms that return at once then cost two small dispatches,
    // not two of up to 256 wavefronts per CU)
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nchunks, (uint64_t)num_cu * (dev_forms ? 32 : 256));
    return {dev_forms                   ? EF_FORM_DEV  // (spec: the ids are below 2^32)
            : wide                      ? EF_FORM_WIDE
            : max_list <= 256           ? EF_FORM_SHORT
            : ntotal < 256 * nchunks    ? EF_FORM_HALF
                                        : EF_FORM_FULL,
            grid};
}
// The chunk kernels write every word of the high stream (k_ef_lowhigh), so nothing has to zero it.  A stream that does not fit the
// caches is cleared all the same: the kernels store a chunk's 100-200 bytes at a time, lines shared between wavefronts reach HBM as
// partial writes, and the same kernel runs 8 % faster on lines a fill has just left in the memory-side cache (S2, 250 MB of high
// words: 2.95 + 0.08 ms instead of 3.19; 16 M ids, 4 MB: 68.7 instead of 65.8 + 4.5 us).
inline bool ef_clear_high(uint64_t high_words, const EfEncPolicy &p) {
    return p.memset >= 0 ? p.memset == 1 : high_words * 8 > EF_CLEAR_HIGH_BYTES;
}
// Objects of up to 2^18 batches get their bulk-decode records (EfRec) from the encoder: the wavefront that writes a batch's directory
// entry holds everything the record needs, and the first decode_all of a fresh object is one launch instead of k_ef_build_recs +
// decode (16 M ids in lists of 256: 53 -> ~47 us; S1-sized: 20 -> ~15 us).  Larger objects keep the lazy build: it also finds the
// exact size of the largest batch, which sets the occupancy of their millisecond-long decode.
inline bool ef_enc_recs(uint64_t nchunks, uint64_t max_list, uint64_t nbatches, const EfEncPolicy &p) {
    return nchunks && max_list && nbatches && nbatches < EF_ENC_RECS_MAX && !p.lazy_recs;
}

// ---- bulk decoder
// records built without the read-back of the largest batch: the longest list bounds it (no batch holds more ids than its list)
inline bool ef_recs_bounded(uint64_t max_list, uint64_t nbatches) { return max_list && nbatches < EF_ENC_RECS_MAX; }
inline uint32_t ef_recs_max_cnt(uint64_t max_list) { return (uint32_t)std::min<uint64_t>(max_list, EF_BATCH_BITS); }
struct EfDecodeForm { uint32_t elem_bytes, per_lane, lds_bytes; };  // k_ef_decode_rec<uint32_t / uint64_t, 4 / 8>, its position table
inline EfDecodeForm ef_decode_form(bool narrow, uint32_t max_cnt) {
    return {narrow ? 4u : 8u, max_cnt <= 256 ? 4u : 8u, std::min<uint32_t>(EF_BATCH_BITS, (max_cnt + 63u) & ~63u) * 2};
}

// ---- three-pass path: the lists k_ef_sort takes (flagged unsorted and not empty), longest first and stable, and where each one's
// power-of-two key array starts
struct EfSortPlan {
    std::vector<uint32_t> lists;
    std::vector<uint64_t> key_off;  // lists.size() + 1
};
template <class Unsorted>
inline EfSortPlan ef_sort_plan(const uint64_t *offsets, uint64_t nlist, Unsorted &&is_unsorted) {
    EfSortPlan sp;
    for (uint64_t l = 0; l < nlist; l++)
        if (offsets[l + 1] > offsets[l] && is_unsorted(l)) sp.lists.push_back((uint32_t)l);
    std::stable_sort(sp.lists.begin(), sp.lists.end(), [&](uint32_t a, uint32_t b) {
        return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b];
    });
    sp.key_off.assign(sp.lists.size() + 1, 0);
    for (size_t i = 0; i < sp.lists.size(); i++) {
        uint64_t n = offsets[sp.lists[i] + 1] - offsets[sp.lists[i]], p2 = 1;
        while (p2 < n) p2 <<= 1;
        sp.key_off[i + 1] = sp.key_off[i] + p2;
    }
    return sp;
}

}  // namespace vidc
