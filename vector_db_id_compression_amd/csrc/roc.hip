// roc.hip -- host side of the ROC codec: scheduling of lists onto wavefronts, arenas, compaction,
// and the vidc_roc_* C-ABI (include/vidc.h).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <numeric>
#include <thread>

#include "append.h"
#include "merge.h"
#include "remove.h"
#include "subset.h"
#include "locate.h"
#include "common.h"
#include "host_call.h"
#include "roc_dec_plan.h"
#include "roc_enc_plan.h"
#include "roc_kernels.h"
#include "roc_u.h"
#include "roc_u2.h"
#include "rows_csr.h"
#include "roc_lane.h"
#include "roc_grp.h"
#include "requests.h"
#include "rows_update.h"
#include "scan.h"

using namespace vidc;
using namespace vidc::dev;

struct vidc_roc {
    int device = 0;
    uint64_t nlist = 0, ntotal = 0;
    bool rows = false;
    uint32_t K = 0;
    // Host copies of the per-list metadata.  The device arrays are authoritative; the host side is filled lazily
    // (ensure_meta / ensure_offsets) because with ~10^6 lists or graph nodes the PCIe round trip of these arrays
    // costs more than the codec kernels.  `offsets` is always valid for IVF objects (it is an input), `prec` holds
    // the values the decode planner needs (lists above TINY_MAX) as soon as encode returns.
    mutable std::vector<uint64_t> offsets;   // nlist+1
    mutable std::vector<uint32_t> prec, nwords, draws;
    // HEURISTIC input of the decode planner (bucket geometry of the b2 kernels), never a correctness input: the prepass' view of
    // a list's largest id -- its true maximum after the full prepass, its LAST id after the light one (== the maximum of an
    // ascending list; a list that turned out not to be ascending is redone by the sorting pass and set to 0 here).  A value
    // below the true maximum only makes the planner assume more ids per bucket.  Empty / 0 = unknown (imported streams).
    std::vector<uint32_t> umax;
    // every list of the object, longest first (stable), when the encoder built that order (calls classified by length alone);
    // empty otherwise.  The decode planner of the whole object cuts its classes out of it.
    std::vector<uint32_t> order_desc;
    uint64_t order_max_n = 0;
    mutable std::vector<uint64_t> heads;
    mutable std::vector<uint64_t> word_off;  // nlist+1
    mutable bool meta_host = false, offsets_host = false;
    mutable std::mutex mu;  // guards the lazy host mirrors and the cached decode plan (objects are otherwise immutable)
    uint64_t total_words = 0, compressed_bytes = 0;
    // device-resident compressed representation
    DevBuf<uint64_t> d_offsets, d_heads, d_word_off;
    DevBuf<uint32_t> d_prec, d_nwords, d_draws, d_words, d_perm;
    mutable uint64_t last_nonclean = 0;
    mutable uint64_t last_handed_back = 0;  // work items of the last decode call that came back with VIDC_ST_RETRY
    // graph objects: the rows ordered by edge count (k_rows_order_*), built by the first whole-graph decode_rows (guarded by mu)
    mutable DevBuf<uint32_t> d_row_order;
    mutable bool row_order_ready = false;
    // decode_all plan, built on first use (depends only on the immutable metadata)
    mutable std::shared_ptr<struct DecPlanCache> plan_all;
    // the same plan without its device arrays, built by the encoder while its kernels run (the host would only wait)
    mutable std::shared_ptr<struct DecPlanCache> plan_ahead;
    ~vidc_roc() {  // the large host arrays go back to the process-wide vector cache (common.h)
        vec_pool<uint64_t>().give(std::move(offsets)); vec_pool<uint64_t>().give(std::move(heads)); vec_pool<uint64_t>().give(std::move(word_off));
        vec_pool<uint32_t>().give(std::move(prec)); vec_pool<uint32_t>().give(std::move(nwords)); vec_pool<uint32_t>().give(std::move(draws));
        vec_pool<uint32_t>().give(std::move(umax)); vec_pool<uint32_t>().give(std::move(order_desc));
    }
};

namespace {

constexpr uint32_t TINY_MAX = 64;
constexpr uint32_t GEN_SMALL_MAX = 4096;   // decoder: fb <= 9 -> 2 KiB of LDS (full occupancy)
// Lists longer than this go to the bitmap kernels (one wave per CU, lowest step latency: they are the critical
// path); shorter ones cost about the same per step in the general kernels, which keep thousands in flight.
constexpr uint32_t U_MIN_LIST = 4097;

inline uint64_t arena_words_for(uint64_t n) { return n * 37 / 32 + 8; }  // <= P+4 bits of growth per step, P <= 32

static_assert(VIDC_LANE_MAX64 == VIDC_LANE_TAB, "divisor table size");
// Kernel family for short lists.  The lane-per-list kernels advance 64 lists per instruction but every list still
// pays the full per-step latency, so they only win once a call has enough lists to fill the machine with them
// (measured crossover ~8 000 lists of 65..1024 ids, ~2 000 tiny lists); smaller calls -- e.g. the few hundred lists
// a search touches -- keep the latency-optimised wave-per-list kernels.  Test hooks: VIDC_NO_LANE=1 (never),
// VIDC_FORCE_LANE=1 (always); both families produce the same bits.
constexpr uint64_t R2_MIN_LIST = 256;   // shorter lists: the general kernel (the chain kernel's set-up -- 32 KiB bitmap, counters -- is ~10 us)
constexpr uint64_t LANE_MIN_LISTS = 8192, LANE_MIN_LISTS64 = 8192, LANE_MIN_TINY = 2048;  // 64: lists of 1025..4096 ids
inline bool env_1(const char *name) {  // starts with '1'
    const char *e = getenv(name);
    return e && e[0] == '1';
}
inline LanePolicy lane_policy() { return env_1("VIDC_NO_LANE") ? LANE_NEVER : env_1("VIDC_FORCE_LANE") ? LANE_ALWAYS : LANE_AUTO; }

inline bool env_on(const char *name) {  // set, not empty, not "0"
    const char *e = std::getenv(name);
    return e && *e && !(e[0] == '0' && !e[1]);
}
// Row-per-list kernels (roc_grp.h: 16 lanes per list, four lists per wavefront) for lists of 4097 .. 131 072 ids.  They are
// throughput kernels -- a step costs about as many instructions as a wave-per-list step but advances four lists -- and
// every list pays a longer step (LDS round trips instead of v_readlane), so they only pay once a call has more such
// lists than the wave-per-list kernels keep resident.  Test hooks: VIDC_NO_GRP=1 (never), VIDC_FORCE_GRP=1 (every list
// of 65 .. 131 072 ids).
constexpr uint64_t GRP_MIN_LISTS = 8192;
inline GrpPolicy grp_policy() {
    // (lists beyond 32 768 ids are chains of >= 40 ms at this family's 1.2 us per step: they keep the lower-latency
    // wave-per-list kernels unless VIDC_FORCE_GRP says otherwise)
    // Decode: up to 16 384 ids -- the 16 385..32 768-id lists are the longest chains next to the b2 / general-kernel lists of a
    // big call, and their step under load is 1.7-2.6 us here against ~1 us on the general decoder (S2: 53-85 ms against 32).
    GrpPolicy g{GRP_MIN_LISTS, VIDC_LANE_MAX64 + 1u, 32768u, 16384u, VIDC_LANE_MAX64 + 1u};
    if (env_on("VIDC_NO_GRP") || env_on("VIDC_FORCE_GENERAL") || env_on("VIDC_OLD_U")) { g.min_lists = ~0ull; return g; }
    if (env_on("VIDC_FORCE_GRP")) { g.min_lists = 0; g.min_n = g.dec_min_n = VIDC_GRP_MIN_LIST; g.max_n = g.dec_max_n = VIDC_GRP_MAX_LIST; }
    return g;
}

// test hook: VIDC_OLD_U=1 keeps the round-1 bitmap kernels (roc_u.h) instead of the hand-scheduled ones (roc_u2.h)
// Lists per wavefront of a lane-per-list launch (VIDC_LPW=8|16|32, measurements only; default 64).  Every list of a
// launch is in flight at once either way, so fewer lists per wavefront only adds wavefronts: measured no better on
// 65 536 x 256 ids (decode 0.99 / 1.01 / 1.04 / 1.16 ms for 64 / 32 / 16 / 8), worse for the 16 / 64-word strips.
inline uint32_t lane_lists_per_wave(const vidc_ctx *, uint32_t, uint32_t) {
    static const int forced = [] { const char *e = std::getenv("VIDC_LPW"); return e ? std::atoi(e) : 0; }();
    return (forced == 8 || forced == 16 || forced == 32) ? (uint32_t)forced : 64u;
}
inline bool old_u_kernels() { return env_1("VIDC_OLD_U"); }
// VIDC_U2_DENSE=0 keeps every list of the 20-bit chain launch on the bitmap body; default: lists of 4097 .. 65 536 ids select from
// dense 16-id blocks (roc_u2.h, U2Dense)
inline bool u2_dense() {
    const char *e = std::getenv("VIDC_U2_DENSE");
    return !(e && e[0] == '0' && !e[1]);
}
// VIDC_U2_DEC_WORD=0 decodes the 20-bit chain launch with the four-word step on U2Geom<20>::DEC_* (A/B runs and tests); default: the
// one-word step on word-granular rows (roc_u2.h, U2DecWord).  Same output either way.
inline bool u2_dec_word() {
    const char *e = std::getenv("VIDC_U2_DEC_WORD");
    return !(e && e[0] == '0' && !e[1]);
}

// test hook: VIDC_FORCE_GENERAL=1 routes every list through the general (sorted-position / bucket) kernels
inline bool force_general() { return env_1("VIDC_FORCE_GENERAL"); }

// kernels that ask for more than 64 KiB of dynamic LDS must opt in
inline int set_big_lds(const void *fn, size_t bytes) {
    VIDC_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return VIDC_OK;
}

template <typename T>
int upload(vidc_ctx *ctx, DevBuf<T> &dst, const std::vector<T> &src) {
    VIDC_TRY(dst.alloc(src.size(), ctx->dpool));
    if (!src.empty())
        VIDC_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return VIDC_OK;
}
template <typename T>
int upload_scratch(vidc_ctx *ctx, Scratch &dst, const std::vector<T> &src) {
    VIDC_TRY(dst.get(ctx, src.size() * sizeof(T)));
    if (!src.empty())
        VIDC_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return VIDC_OK;
}

// device -> host through pinned staging (blocks until the data is there)
template <typename T>
int download(vidc_ctx *ctx, std::vector<T> &dst, const T *d_src, size_t count) {
    dst.resize(count);
    if (!count) return VIDC_OK;
    Pinned st;
    VIDC_TRY(st.get(ctx, count * sizeof(T)));
    VIDC_HIP(hipMemcpyAsync(st.p, d_src, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    std::memcpy(dst.data(), st.p, count * sizeof(T));
    return VIDC_OK;
}

int ensure_offsets_locked(const vidc_roc *r) { return ensure_offsets_host_locked(r, r->d_offsets.p); }
int ensure_offsets(const vidc_roc *r) { return ensure_offsets_host(r, r->d_offsets.p); }
int ensure_meta(const vidc_roc *r) {
    std::lock_guard<std::mutex> g(r->mu);
    VIDC_TRY(ensure_offsets_locked(r));
    if (r->meta_host) return VIDC_OK;
    VIDC_HIP(hipSetDevice(r->device));
    VIDC_TRY(mirror_to_host(r->prec, (const uint32_t *)r->d_prec.p, r->nlist));
    VIDC_TRY(mirror_to_host(r->nwords, (const uint32_t *)r->d_nwords.p, r->nlist));
    VIDC_TRY(mirror_to_host(r->draws, (const uint32_t *)r->d_draws.p, r->nlist));
    VIDC_TRY(mirror_to_host(r->heads, (const uint64_t *)r->d_heads.p, r->nlist));
    VIDC_TRY(mirror_to_host(r->word_off, (const uint64_t *)r->d_word_off.p, r->nlist + 1));
    r->meta_host = true;
    return VIDC_OK;
}

int check_status(const std::vector<uint32_t> &status, const char *what) {
    for (size_t l = 0; l < status.size(); l++) {
        switch (status[l]) {
            case VIDC_ST_OK: break;
            case VIDC_ST_DOMAIN:
                set_error("%s: list %zu holds an id outside [0, 2^31) (reference: int max_id, "
                          "custom_invlists_impl.cpp:163)", what, l);
                return VIDC_ERR_DOMAIN;
            case VIDC_ST_OVERFLOW:
                set_error("%s: list %zu overflowed its ANS word arena", what, l);
                return VIDC_ERR_OVERFLOW;
            case VIDC_ST_MT:
                set_error("%s: list %zu needed more than %d mt19937 underflow words", what, l, VIDC_MT_TABLE);
                return VIDC_ERR_OVERFLOW;
            default:
                set_error("%s: list %zu finished with status %u", what, l, status[l]);
                return VIDC_ERR_INVALID;
        }
    }
    return VIDC_OK;
}

// Host loops over the lists of a call (classification, work-list sorts): with 10^6 lists they are the host's
// critical path between the prepass and the first encode kernel (7 ms single-threaded), so they are split over a few
// threads.  f(begin, end, part) for `parts` contiguous ranges; small calls stay on the calling thread.
constexpr uint64_t PAR_MIN_LISTS = 131072;
inline unsigned par_parts(uint64_t n) {
    if (n < PAR_MIN_LISTS) return 1;
    const char *e = getenv("VIDC_HOST_THREADS");  // test hook: 1 = single-threaded host loops
    const unsigned cap = e && e[0] ? (unsigned)std::max(1, atoi(e)) : 8u;
    const unsigned hw = std::thread::hardware_concurrency();
    return std::max(1u, std::min(cap, hw ? hw : 1u));
}
template <class F>
void par_ranges(uint64_t n, unsigned parts, F &&f) {
    if (parts <= 1 || n == 0) { f((uint64_t)0, n, 0u); return; }
    std::vector<std::thread> th;
    const uint64_t per = (n + parts - 1) / parts;
    for (unsigned t = 1; t < parts; t++) {
        const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
        th.emplace_back([&f, a, b, t] { f(a, b, t); });
    }
    f((uint64_t)0, std::min<uint64_t>(n, per), 0u);
    for (auto &x : th) x.join();
}

// lists sorted longest first: the hardware dispatches workgroups in order, so this is LPT scheduling.
// Counting sort by length (lengths are bounded by VIDC_ROC_MAX_LIST): O(n), stable.
void sort_desc(std::vector<uint32_t> &wl, const std::vector<uint64_t> &offsets) {
    if (wl.size() < 2) return;
    uint64_t maxlen = 0, prev = ~0ull;
    bool sorted = true;  // equal-sized lists, or an index whose lists come longest first: nothing to do
    for (uint32_t l : wl) {
        const uint64_t n = offsets[l + 1] - offsets[l];
        maxlen = std::max<uint64_t>(maxlen, n);
        sorted &= n <= prev;
        prev = n;
    }
    if (sorted) return;
    if (maxlen > (1u << 22)) {  // not reachable for ROC lists; keep a comparison sort for safety
        std::stable_sort(wl.begin(), wl.end(), [&](uint32_t a, uint32_t b) {
            return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b];
        });
        return;
    }
    std::vector<uint32_t> out = vec_pool<uint32_t>().take(wl.size());
    out.resize(wl.size());
    struct Back { std::vector<uint32_t> &v; ~Back() { vec_pool<uint32_t>().give(std::move(v)); } } out_back{out};  // (holds wl's old array after the swap)
    const unsigned parts = maxlen <= 65536 ? par_parts(wl.size()) : 1;
    if (parts > 1) {  // the same stable counting sort, histogram and scatter per contiguous part of the work list
        const size_t nb = maxlen + 1;
        std::vector<uint32_t> hist((size_t)parts * nb, 0);
        par_ranges(wl.size(), parts, [&](uint64_t a, uint64_t b, unsigned t) {
            uint32_t *h = &hist[(size_t)t * nb];
            for (uint64_t i = a; i < b; i++) h[maxlen - (offsets[wl[i] + 1] - offsets[wl[i]])]++;
        });
        uint32_t run = 0;  // bucket-major, part-minor: equal lengths keep their work-list order
        for (size_t k = 0; k < nb; k++)
            for (unsigned t = 0; t < parts; t++) {
                const uint32_t c = hist[(size_t)t * nb + k];
                hist[(size_t)t * nb + k] = run;
                run += c;
            }
        par_ranges(wl.size(), parts, [&](uint64_t a, uint64_t b, unsigned t) {
            uint32_t *h = &hist[(size_t)t * nb];
            for (uint64_t i = a; i < b; i++) out[h[maxlen - (offsets[wl[i] + 1] - offsets[wl[i]])]++] = wl[i];
        });
        wl.swap(out);
        return;
    }
    std::vector<uint32_t> start(maxlen + 2, 0);
    for (uint32_t l : wl) start[maxlen - (offsets[l + 1] - offsets[l]) + 1]++;  // bucket 0 = longest
    for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
    for (uint32_t l : wl) out[start[maxlen - (offsets[l + 1] - offsets[l])]++] = l;
    wl.swap(out);
}

// End of an encode call: status check + word offsets + sizes + compaction, all on the device.  Two halves so that the first
// can be queued right behind the encode kernels -- while the host still plans the decode -- and ONE synchronisation serves the
// kernels, the status summary (errors / lists waiting for the sorting pass) and the size read-back:
//   finish_enqueue: status summary + totals into `t`; the exclusive scan of the word counts (IVF lists: k_roc_tail)
//   finish_complete (after a synchronisation of the stream): checks, allocation of the stream, compaction (graph rows: with the scans
//                   of the word and edge counts inside, k_roc_rows_compact), final synchronisation
struct EncodeTail {
    Scratch s_sum, s_tmp, s_tmp2, s_state;
    bool state_zeroed = false;  // the tile states of k_roc_tail were cleared ahead of the encode kernels
    const uint32_t *d_sizes = nullptr;  // graph rows: the edge counts, for the scan inside the compaction
    Pinned tail;
    unsigned long long *t = nullptr;  // [0..3] status summary (first bad list, -, retries, pending sorts), [4] total words, [5] ntotal, [6] non-empty rows
};
// (ahead of the encode kernels: the tile states of the tail kernel, so that clearing them is not part of the tail)
inline uint32_t rows_tiles(uint64_t nlist) { return (uint32_t)((nlist + 63) / 64); }  // tiles of k_roc_rows_compact
inline uint32_t rows_chunks(uint64_t nlist) { return (uint32_t)((nlist + VIDC_ROWS_CHUNK - 1) / VIDC_ROWS_CHUNK); }  // workgroups of k_roc_rows_totals
inline size_t rows_state_bytes(uint64_t nlist) {  // tile sums (words, edges) | chunk sums | counter | chunk prefixes
    return ((size_t)rows_tiles(nlist) * 2 + (size_t)rows_chunks(nlist) * 10 + 1) * 8;
}
int finish_prepare(vidc_ctx *ctx, const vidc_roc *r, EncodeTail &e) {
    if (!r->nlist) return VIDC_OK;
    // graph rows: [word scan | edge scan | tile counter | sum[8]] of k_roc_rows_totals / k_roc_rows_compact
    const size_t bytes = r->rows ? rows_state_bytes(r->nlist) : ((size_t)(r->nlist / VIDC_TAIL_TILE + 1u) + 10) * 8;
    VIDC_TRY(e.s_state.get(ctx, bytes));
    VIDC_HIP(hipMemsetAsync(e.s_state.p, 0, bytes, ctx->stream));
    e.state_zeroed = true;
    return VIDC_OK;
}
int finish_enqueue(vidc_ctx *ctx, vidc_roc *r, EncodeTail &e, Scratch &d_status_buf, const uint32_t *d_sizes) {
    const uint64_t nlist = r->nlist;
    VIDC_TRY(e.tail.get(ctx, 128));
    unsigned long long *t = e.t = e.tail.as<unsigned long long>();
    t[0] = ~0ull; t[1] = 0; t[2] = 0; t[3] = 0; t[4] = 0; t[5] = 0; t[6] = 0; t[7] = 0;
    VIDC_TRY(r->d_word_off.alloc(nlist + 1, ctx->dpool));
    if (nlist && r->rows) {  // totals only: the scans ride on the compaction (k_roc_rows_compact)
        const uint32_t nt = rows_tiles(nlist);
        if (!e.state_zeroed) {
            VIDC_TRY(e.s_state.get(ctx, rows_state_bytes(nlist)));
            VIDC_HIP(hipMemsetAsync(e.s_state.p, 0, rows_state_bytes(nlist), ctx->stream));
        }
        e.state_zeroed = false;  // (used up)
        e.d_sizes = d_sizes;
        VIDC_TRY(r->d_offsets.alloc(nlist + 1, ctx->dpool));
        hipLaunchKernelGGL(k_roc_rows_totals, dim3(rows_chunks(nlist)), dim3(256), 0, ctx->stream, r->d_nwords.p, d_sizes, d_status_buf.as<uint32_t>(),
                           (uint32_t)nlist, e.s_state.as<unsigned long long>() + 2ull * nt, t);
        VIDC_HIP(hipGetLastError());
        return VIDC_OK;
    }
    if (nlist) {  // summary + word offsets + totals in one launch; its last workgroup stores the results into `t`
        const uint32_t ntiles = (uint32_t)(nlist / VIDC_TAIL_TILE + 1u);
        const size_t state_bytes = ((size_t)ntiles + 10) * 8;
        if (!e.state_zeroed) {
            VIDC_TRY(e.s_state.get(ctx, state_bytes));
            VIDC_HIP(hipMemsetAsync(e.s_state.p, 0, state_bytes, ctx->stream));
        }
        e.state_zeroed = false;  // (used up)
        hipLaunchKernelGGL(k_roc_tail, dim3(ntiles), dim3(256), 0, ctx->stream, r->d_nwords.p, (uint32_t)nlist, r->d_word_off.p,
                           d_status_buf.as<uint32_t>(), e.s_state.as<unsigned long long>(), t);
        VIDC_HIP(hipGetLastError());
        return VIDC_OK;
    }
    // no lists: the offsets of an empty object
    VIDC_HIP(hipMemsetAsync(r->d_word_off.p, 0, 8, ctx->stream));
    if (r->rows) { VIDC_TRY(r->d_offsets.alloc(1, ctx->dpool)); VIDC_HIP(hipMemsetAsync(r->d_offsets.p, 0, 8, ctx->stream)); }
    return VIDC_OK;
}
int finish_complete(vidc_ctx *ctx, vidc_roc *r, EncodeTail &e, const uint32_t *d_arena, uint32_t arena_stride, Scratch &d_status_buf,
                    uint64_t nonempty_lists, double &kernel_ms) {
    const uint64_t nlist = r->nlist;
    const unsigned long long *t = e.t;
    if (t[0] != ~0ull) {
        std::vector<uint32_t> status;
        VIDC_TRY(download(ctx, status, d_status_buf.as<uint32_t>(), nlist));
        VIDC_TRY(check_status(status, "roc encode"));
    }
    r->total_words = t[4];
    if (r->rows) { r->ntotal = t[5]; nonempty_lists = t[6]; }
    // ANSState::size() = 8 + 4 * words per non-empty list; "let's pretend no memory is used" for empty ones
    // (custom_invlists_impl.cpp:196-206).  Empty lists have no words.
    r->compressed_bytes = 8ull * nonempty_lists + 4ull * r->total_words;
    VIDC_TRY(r->d_words.alloc(r->total_words + 16, ctx->dpool));  // + padding: the look-ahead of the lane / row decoders reads up to 15 words past the last stream
    if (nlist) {
        EventTimer tm = EventTimer::started(ctx);
        const uint64_t *d_off = r->rows ? (const uint64_t *)nullptr : (const uint64_t *)r->d_offsets.p;
        if (r->rows) {  // 64 rows per wavefront; word offsets and CSR offsets are scanned on the way
            const uint32_t nt = rows_tiles(nlist);
            // Every wavefront of the launch resident at once (what the runtime says fits, not a guess: a tile waits for the tiles in
            // front of it in its chunk), and a multiple of 64 of them: the 64 tiles of a chunk are then 64 consecutive workgroups
            // in the same trip of their loops, so a tile only ever waits for workgroups with smaller numbers.
            static const int occ = [] {
                int o = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, k_roc_rows_compact, 64, 0) != hipSuccess || o < 1) o = 1;
                return o;
            }();
            const uint32_t cap = std::max<uint32_t>(64u, (uint32_t)ctx->num_cu * (uint32_t)occ / 64u * 64u);
            const uint32_t grid = std::min<uint32_t>(nt, cap);
            hipLaunchKernelGGL(k_roc_rows_compact, dim3(grid), dim3(64), 0, ctx->stream, d_arena, arena_stride, r->d_nwords.p, e.d_sizes,
                               (uint32_t)nlist, e.s_state.as<unsigned long long>(), nt,
                               e.s_state.as<unsigned long long>() + 2ull * nt + 8ull * rows_chunks(nlist) + 1, r->d_word_off.p, r->d_offsets.p,
                               r->d_words.p);
        } else if (r->total_words / nlist < 64) {  // tiny lists (a few dozen words each): one wavefront per 64 lists
            const uint32_t grid = (uint32_t)std::min<uint64_t>((nlist + 63) / 64, (uint64_t)ctx->num_cu * 64);
            hipLaunchKernelGGL(k_roc_compact_groups, dim3(grid), dim3(64), 0, ctx->stream, d_arena, d_off, arena_stride,
                               r->d_word_off.p, r->d_words.p, (uint32_t)nlist);
        } else if (r->total_words / nlist < 200 ){  // a wavefront per four lists (k_roc_compact_waves)
            const uint32_t grid = (uint32_t)std::min<uint64_t>((nlist + 15) / 16, (uint64_t)ctx->num_cu * 8);
            hipLaunchKernelGGL(k_roc_compact_waves, dim3(grid), dim3(256), 0, ctx->stream, d_arena, d_off, arena_stride,
                               r->d_word_off.p, r->d_words.p, (uint32_t)nlist);
        } else {
            const uint32_t grid = (uint32_t)std::min<uint64_t>(nlist, (uint64_t)ctx->num_cu * 16);
            hipLaunchKernelGGL(k_roc_compact, dim3(grid), dim3(256), 0, ctx->stream, d_arena, d_off, arena_stride,
                               r->d_word_off.p, r->d_words.p, (uint32_t)nlist);
        }
        VIDC_HIP(hipGetLastError());
        double ms = tm.stop();  // (synchronises: the call's last wait)
        ctx->phase_ms[VIDC_PHASE_ROC_COMPACT] = ms;
        kernel_ms += ms;
    } else {
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    }
    return VIDC_OK;
}

// ---- decode planning (roc_dec_plan.h): work items grouped by kernel class, each with private scratch
#define VIDC_LANE_ALIGN_DEFAULT 16u        // bucket rows of the lane decoders on 64-byte boundaries (S2 decode 70.9 -> 69.8 ms: DESIGN section 13)
constexpr uint32_t B2_MASK_MIN_CHAINS = 512;  // k_roc_decode_b2 launches of this many chains size their row loads by the member count
constexpr DecLimits DEC_LIMITS{TINY_MAX, GEN_SMALL_MAX, U_MIN_LIST, R2_MIN_LIST, VIDC_LANE_REG_MAX, VIDC_LANE_PAIR_MAX, VIDC_LANE_QUAD_MAX, VIDC_LANE_MAX,
                               VIDC_LANE_MAX128, VIDC_LANE_MAX64, VIDC_B2L_MAX_LIST, VIDC_B2L_MID_LIST, VIDC_B2L_LOAD, LANE_MIN_LISTS, LANE_MIN_LISTS64,
                               LANE_MIN_TINY};
// a plan whose arrays come from and go back to the process-wide vector cache (common.h)
struct PooledDecPlan : DecPlan {
    ~PooledDecPlan() {
        vec_pool<uint32_t>().give(std::move(wl)); vec_pool<uint32_t>().give(std::move(item));
        vec_pool<uint64_t>().give(std::move(scratch_off)); vec_pool<uint64_t>().give(std::move(slots_off));
    }
};

}  // namespace

// device copy of a plan, kept with the compressed object for repeated decode_all calls
struct DecPlanCache {
    PooledDecPlan plan;
    bool wide = false;  // the stream mode the plan was built for (a context of the other mode builds its own: ADVICE round 4)
    DevBuf<uint32_t> d_wl;
    DevBuf<uint64_t> d_scratch_off, d_slots_off;
};

namespace {

// decode_all plan of a freshly encoded object (defined with the planner below)
std::shared_ptr<DecPlanCache> plan_ahead_build(const vidc_roc *r, bool wide);
constexpr uint64_t PLAN_AHEAD_MIN_LISTS = 4096;

static_assert(VIDC_PF_UNSORTED == ENC_PF_UNSORTED && VIDC_PF_DOMAIN == ENC_PF_DOMAIN && VIDC_OK == 0, "roc_enc_plan.h mirrors these");
constexpr EncLimits ENC_LIMITS{TINY_MAX, VIDC_LANE_MAX, VIDC_LANE_MAX64, VIDC_GRP_LEV2_MAX, U_MIN_LIST, R2_MIN_LIST, VIDC_ROC_MAX_LIST,
                               LANE_MIN_LISTS, LANE_MIN_LISTS64, LANE_MIN_TINY};
// Every kernel class of a call is one entry of its launch list: its name, its default stream (0 = the caller's, i = auxiliary i - 1)
// and its launch.  Default streams / order = the schedule measured best (comments at the entries); VIDC_ENC_SCHED (measurements)
// replaces it (grammar: roc_enc_plan.h); names: U20 R2 C3 G3.<k> G2.<k> (octaves of the row-per-list classes, longest first) C2 U18
// C1 L64 L32 L16 L4 TINY.  Launches the string does not name keep their default stream and go out last.
struct EncLaunch { std::string name; int def_stream; std::function<int(hipStream_t)> fn; };
// One encode call: the object under construction, the call's scratch and staging blocks, its work lists, and what one stage of
// encode_impl leaves for the next.  (destroyed last member first: the guard ahead of the blocks it protects, the object last)
struct EncodeCall {
    vidc_ctx *ctx;
    uint64_t nlist; const uint64_t *offsets, *d_ids; bool rows; uint32_t K; const int32_t *d_rows; int precision_mode;  // the call's arguments
    std::unique_ptr<vidc_roc> r{new vidc_roc()};
    double kernel_ms = 0;
    HostTrace tr{"roc encode"};
    EncPolicy pol; EncUse use; EncWorkLists w;
    uint64_t ntotal_in = 0, max_n = 0, n_tiny_lists = 0, n_mid_lists = 0, arena_words = 0, nonempty = 0, ntiny = 0;
    bool any_big = false, all_desc = false, light_prepass = false, pre_deferred = false, plan_on_device = false;
    const uint32_t *maxid = nullptr, *pflags = nullptr;  // prepass results on the host (null: none, or read back later)
    uint32_t arena_stride = 0;
    Scratch s_arena, s_status, s_sizes, s_sid, s_wl, s_maxid, s_flags;
    EncodeTail tail;  // status summary + sizes of the call, queued behind the encode kernels
    Pinned h_wl, h_pre, h_off, h_plan;
    // an early return while the offsets upload / the deferred prepass copy is in flight must not release their staging blocks
    // (declared behind them: destroyed first; armed where such a copy is enqueued)
    StreamGuard pre_guard{ctx, false};
    const uint32_t *d_wl = nullptr;
    RocEncArgs a{};
    int enc_prio = 0;
    std::vector<EncLaunch> L;
    uint32_t aux_used = 0;  // auxiliary streams that have joined the call
    std::vector<uint32_t> pend;  // lists the first pass handed back for the sorting pass
    const std::vector<uint32_t> &wl(int cls) const { return w.wl[cls]; }
    uint64_t len(uint32_t l) const { return r->offsets[l + 1] - r->offsets[l]; }
};

// policies of the call, persistent outputs; graph rows: everything the offsets stages would find out
int enc_begin(EncodeCall &c, uint64_t N, uint32_t flags) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    r->device = ctx->device; r->rows = c.rows; r->K = c.K; r->nlist = c.nlist;
    c.pol.want_perm = (flags & VIDC_ROC_WANT_PERM) && !c.rows;
    c.ntotal_in = c.rows ? N * c.K : (c.nlist ? c.offsets[c.nlist] : 0);
    c.pol.f_general = force_general();  // getenv once, not per list
    c.pol.lpol = c.pol.f_general ? LANE_NEVER : lane_policy();
    c.pol.gpol = grp_policy(); c.pol.wide = ctx->wide; c.pol.num_cu = ctx->num_cu;
    VIDC_TRY(r->d_heads.alloc(c.nlist, ctx->dpool)); VIDC_TRY(r->d_prec.alloc(c.nlist, ctx->dpool));
    VIDC_TRY(r->d_nwords.alloc(c.nlist, ctx->dpool)); VIDC_TRY(r->d_draws.alloc(c.nlist, ctx->dpool));
    if (c.pol.want_perm) VIDC_TRY(r->d_perm.alloc(c.ntotal_in ? c.ntotal_in : 1, ctx->dpool));
    c.tr.mark("persistent allocs");
    // (graph rows: slots of whole 64-byte sectors -- a row's ~100 bytes of stream then lie in two sectors, not in two and a half)
    c.arena_stride = c.rows ? (uint32_t)((arena_words_for(c.K) + 15u) & ~15ull) : 0u;
    if (!c.rows) return VIDC_OK;
    // graph rows: every row is a tiny list, in order -- no offsets, no prepass, no work list array (kernels take l = work item)
    if (c.K == 0 || c.K > TINY_MAX) { set_error("graph rows: K=%u unsupported (1..64)", c.K); return VIDC_ERR_UNSUPPORTED; }
    c.arena_words = roc_arena_at(nullptr, c.arena_stride, c.nlist);
    c.ntiny = c.nlist;
    c.use.lane_tiny = lane_wanted(c.pol.lpol, c.nlist, LANE_MIN_TINY);
    return c.s_sizes.get(c.ctx, c.nlist * 4);
}

// the offsets: the object's host copy, validation, longest list, non-empty lists, the class sizes the policies look at, staging, upload
int enc_scan_offsets(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    const uint64_t nlist = c.nlist, *offsets = c.offsets;
    if (!offsets) return VIDC_ERR_INVALID;
    // the object's host copy of the offsets: on a helper thread for calls of 10^5 lists and more (8 MB at 10^6 lists: 0.6 ms
    // of the 1.3 ms this phase took on S2), next to the validation pass and the staging copy below; joined before the
    // classification, the first reader
    std::thread offsets_copy;
    struct JoinOnExit { std::thread &t; ~JoinOnExit() { if (t.joinable()) t.join(); } } offsets_copy_guard{offsets_copy};
    r->offsets = vec_pool<uint64_t>().take(nlist + 1);
    if (par_parts(nlist) > 1) offsets_copy = std::thread([&] { r->offsets.assign(offsets, offsets + nlist + 1); });
    else r->offsets.assign(offsets, offsets + nlist + 1);
    r->offsets_host = true;
    c.tr.mark("offsets: object's copy");
    // (no synchronisation of its own for the upload below: the staging block lives until the call returns; an early error return
    // before the call's first wait synchronises through the guard)
    VIDC_TRY(c.h_off.get(ctx, (nlist + 1) * 8));
    const unsigned parts = par_parts(nlist);
    const GrpPolicy &gpol = c.pol.gpol;
    // (first the cheap facts -- extremes, order, validity as ONE flag --; the class sizes only need their own pass when the
    // lengths straddle a class boundary: an index of equal-sized lists, or a graph, is classified by its extremes)
    std::vector<EncCounts> acc(parts);
    par_ranges(nlist, parts, [&](uint64_t la, uint64_t lb, unsigned t) {
        // (threaded calls count the classes in the same pass: every pass costs a round of thread starts)
        if (parts > 1) { acc[t] = count_classes(offsets, la, lb, gpol, ENC_LIMITS); return; }
        // (one thread: the staging copy for the upload rides along; four lists per instruction where the host can)
        OffsetsPass op;
        offsets_pass(offsets + la, lb - la, c.h_off.as<uint64_t>() + la, op);
        acc[t].bad = op.bad; acc[t].nonempty = op.nonempty; acc[t].max_n = op.max_n; acc[t].min_n = op.min_n; c.all_desc = op.desc;
    });
    EncCounts all;
    for (unsigned t = 0; t < parts; t++) all.add(acc[t]);
    if (all.bad)  // the first offending list, as a single pass would report it
        for (uint64_t l = 0; l < nlist; l++) {
            if (offsets[l + 1] < offsets[l]) { set_error("offsets not monotone at list %llu", (unsigned long long)l); return VIDC_ERR_INVALID; }
            if (offsets[l + 1] - offsets[l] > VIDC_ROC_MAX_LIST) {
                set_error("list %llu has %llu ids; ROC lists are limited to %u (the reference codec is only lossless up to 65536, SURVEY 8a-Q2)",
                          (unsigned long long)l, (unsigned long long)(offsets[l + 1] - offsets[l]), VIDC_ROC_MAX_LIST);
                return VIDC_ERR_DOMAIN;
            }
        }
    const uint64_t max_n = c.max_n = all.max_n, min_n = all.min_n;
    c.nonempty = all.nonempty;
    uint64_t n_mid64_lists = 0, n_grp_lists = 0;
    auto in_one = [&](uint64_t lo, uint64_t hi) { return nlist && min_n >= lo && max_n <= hi; };
    if (parts > 1) {
        c.n_tiny_lists = all.c0; c.n_mid_lists = all.c1; n_mid64_lists = all.c2; n_grp_lists = all.cg;
    } else {
        const bool one_class = in_one(0, TINY_MAX) || in_one(TINY_MAX + 1, VIDC_LANE_MAX) || in_one(VIDC_LANE_MAX + 1, VIDC_LANE_MAX64) || (nlist && min_n > VIDC_LANE_MAX64);
        const bool grp_reach = max_n >= gpol.min_n && min_n <= gpol.max_n;  // (lists in reach of the row-per-list kernels)
        const EncCounts x = (!one_class || grp_reach) ? count_classes(offsets, 0, nlist, gpol, ENC_LIMITS) : EncCounts();
        if (one_class) {
            c.n_tiny_lists = max_n <= TINY_MAX ? nlist : 0;
            c.n_mid_lists = in_one(TINY_MAX + 1, VIDC_LANE_MAX) ? nlist : 0;
            n_mid64_lists = in_one(VIDC_LANE_MAX + 1, VIDC_LANE_MAX64) ? nlist : 0;
        } else {
            c.n_tiny_lists = x.c0; c.n_mid_lists = x.c1; n_mid64_lists = x.c2;
        }
        if (grp_reach) n_grp_lists = x.cg;
    }
    c.any_big = max_n > TINY_MAX;
    c.tr.mark("offsets: pass + staging");
    c.arena_words = roc_arena_at(offsets, 0, nlist);
    r->ntotal = offsets[nlist];
    VIDC_TRY(r->d_offsets.alloc(nlist + 1, ctx->dpool));
    if (parts > 1 || nlist == 0)  // (a single-threaded pass above has copied them already)
        par_ranges(nlist + 1, parts, [&](uint64_t a0, uint64_t b0, unsigned) {
            std::memcpy(c.h_off.as<uint64_t>() + a0, offsets + a0, (b0 - a0) * 8);
        });
    if (offsets_copy.joinable()) offsets_copy.join();
    c.tr.mark("offsets: blocks");
    VIDC_HIP(hipMemcpyAsync(r->d_offsets.p, c.h_off.p, (nlist + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    c.pre_guard.arm();
    c.tr.mark("offsets: upload call");
    c.use = enc_families(c.n_tiny_lists, c.n_mid_lists, n_mid64_lists, n_grp_lists, c.pol, ENC_LIMITS);
    return VIDC_OK;
}

// classification prepass (one workgroup per list): max id -> precision, sortedness, domain
int enc_prepass(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    const uint64_t nlist = c.nlist;
    if (!c.any_big) { r->prec.assign(nlist, 0); return VIDC_OK; }  // tiny lists only: the planner does not look at their precision
    VIDC_TRY(c.s_maxid.get(ctx, nlist * 4)); VIDC_TRY(c.s_flags.get(ctx, nlist * 4)); VIDC_TRY(c.h_pre.get(ctx, nlist * 8));
    EventTimer t = EventTimer::started(ctx);
    // Every kernel that takes a list streams it anyway and checks what the full prepass would (ids inside
    // [0, 2^31), ascending order where it matters, ids that fit the precision; the lane-per-list encoders since
    // round 3: each sampled id against its left neighbour): the prepass only looks at the LAST id of each list -- the maximum of an ascending
    // list -- instead of re-reading all of them (8 bytes per id).  A list that turns out not to be ascending
    // comes back with VIDC_ST_PENDING_SORT and takes the sorting second pass like a multiset does.
    c.light_prepass = !old_u_kernels() && !std::getenv("VIDC_FULL_PREPASS");
    // No list long enough for the bitmap kernels (the only classes chosen by the width of a list's ids): the host
    // classifies by length alone and reads the maxima back when it needs them -- for the decode plan, while the
    // encode kernels run -- instead of waiting for the prepass here (0.1 ms per call at 65 536 lists).  A last id
    // outside the domain is then reported by the kernel that takes the list, like one in the middle of a list.
    c.pre_deferred = c.light_prepass && c.max_n < U_MIN_LIST;
    auto prepass_last = [&] {
        hipLaunchKernelGGL(k_roc_prepass_last, dim3((uint32_t)((nlist + 255) / 256)), dim3(256), 0, ctx->stream, c.d_ids,
                           r->d_offsets.p, (uint32_t)nlist, c.precision_mode, c.s_maxid.as<uint32_t>(), c.s_flags.as<uint32_t>(), r->d_prec.p);
    };
    r->prec = vec_pool<uint32_t>().take(nlist); r->prec.resize(nlist);
    if (c.pre_deferred) {
        VIDC_HIP(hipEventRecord(ctx->ev_pre[0], ctx->stream));
        prepass_last();
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(hipEventRecord(ctx->ev_pre[1], ctx->stream));
        VIDC_HIP(hipMemcpyAsync(c.h_pre.p, c.s_maxid.p, nlist * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipEventRecord(ctx->ev_pre[2], ctx->stream));
        c.pre_guard.arm();
        c.tr.mark("prepass kernel (read back later)");
        return VIDC_OK;
    }
    if (c.light_prepass) prepass_last();
    else
        hipLaunchKernelGGL(k_roc_prepass, dim3((uint32_t)std::min<uint64_t>(nlist, (uint64_t)ctx->num_cu * 32)), dim3(256), 0, ctx->stream, c.d_ids,
                           r->d_offsets.p, (uint32_t)nlist, c.precision_mode, c.s_maxid.as<uint32_t>(), c.s_flags.as<uint32_t>(), r->d_prec.p);
    VIDC_HIP(hipGetLastError());
    (void)t.mark();
    VIDC_HIP(hipMemcpyAsync(c.h_pre.p, c.s_maxid.p, nlist * 4, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(hipMemcpyAsync(c.h_pre.as<uint32_t>() + nlist, c.s_flags.p, nlist * 4, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    c.pre_guard.disarm();
    c.kernel_ms += t.elapsed();
    c.maxid = c.h_pre.as<uint32_t>();
    c.pflags = c.maxid + nlist;
    c.tr.mark("prepass kernel + d2h");
    // what the decode planner needs later (kernel class, bucket geometry) is known right here
    // (the precisions are filled in by the classification: one pass over the lists instead of two)
    r->umax = vec_pool<uint32_t>().take(nlist); r->umax.assign(c.maxid, c.maxid + nlist);
    return VIDC_OK;
}

// every list into the work list of its kernel class, every class longest first, the longest chains to the position-bitmap kernel
int enc_classify(EncodeCall &c) {
    vidc_roc *r = c.r.get();
    const uint64_t nlist = c.nlist; const unsigned parts = par_parts(nlist);
    // (the switch is read where it always was: only by a call that could take the by-length route)
    if (!c.maxid && !c.pflags && parts == 1 && !c.pol.f_general && !(c.pol.no_length_classes = env_on("VIDC_NO_LENGTH_CLASSES"))) {
        // (the precisions are filled in when the prepass has been read back; tiny-only calls have set them)
        std::vector<uint32_t> order = vec_pool<uint32_t>().take(nlist);
        classify_by_length(c.offsets, nlist, c.max_n, c.all_desc, c.use, c.pol, ENC_LIMITS, c.w, order);
        r->order_desc.swap(order);
        r->order_max_n = c.max_n;
    } else {
        auto par = [](uint64_t n, unsigned np, auto &&f) { par_ranges(n, np, f); };
        const int64_t bad = classify_per_list(c.offsets, nlist, c.maxid, c.pflags, c.precision_mode, c.use, c.pol, ENC_LIMITS, c.n_tiny_lists,
                                              c.use.lane ? c.n_mid_lists : 0, parts, par, r->prec.data(), c.w);
        if (bad >= 0) {
            set_error("roc encode: list %llu holds an id outside [0, 2^31) (reference: int max_id, custom_invlists_impl.cpp:163)", (unsigned long long)bad);
            return VIDC_ERR_DOMAIN;
        }
    }
    c.ntiny = c.w.wl[W_TINY].size();
    c.tr.mark("classify");
    if (parts > 1) {  // one thread per class (independent vectors, read-only offsets)
        std::vector<std::thread> th;
        for (int k = W_U20; k < W_COUNT; k++)
            if (c.w.wl[k].size() > 1) th.emplace_back([&c, r, k] { sort_desc(c.w.wl[k], r->offsets); });
        sort_desc(c.w.wl[W_U18], r->offsets);
        for (auto &x : th) x.join();
    } else {
        for (int k = W_U18; k < W_COUNT; k++)
            if (!c.w.sorted[k]) sort_desc(c.w.wl[k], r->offsets);
    }
    c.pol.old_u = !c.pol.f_general && old_u_kernels(); c.pol.no_r2 = !c.pol.f_general && !c.pol.old_u && env_on("VIDC_NO_R2");  // (short-circuit, as ever)
    promote_r2(c.w, r->offsets.data(), c.pol, ENC_LIMITS);
    c.tr.mark("sort work lists");
    return VIDC_OK;
}

// arena, status array, tail state; the work lists in one block, class after class (EncClass order); the kernels' arguments
int enc_upload_worklists(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    VIDC_TRY(c.s_arena.get(ctx, c.arena_words * 4));
    VIDC_TRY(c.s_status.get(ctx, c.nlist * 4));
    if (c.nlist) VIDC_HIP(hipMemsetAsync(c.s_status.p, 0xff, c.nlist * 4, ctx->stream));
    VIDC_TRY(finish_prepare(ctx, r, c.tail));
    if (!c.rows) {
        const size_t total = c.w.total();
        VIDC_TRY(c.h_wl.get(ctx, total * 4));
        size_t k = 0;
        for (const std::vector<uint32_t> &v : c.w.wl) {
            if (!v.empty()) std::memcpy(c.h_wl.as<uint32_t>() + k, v.data(), v.size() * 4);
            k += v.size();
        }
        VIDC_TRY(c.s_wl.get(ctx, total * 4));
        if (total) VIDC_HIP(hipMemcpyAsync(c.s_wl.p, c.h_wl.p, total * 4, hipMemcpyHostToDevice, ctx->stream));
        c.d_wl = c.s_wl.as<uint32_t>();
    }
    RocEncArgs &a = c.a;
    a.ids = c.d_ids; a.rows = c.d_rows; a.K = c.K;
    a.offsets = c.rows ? nullptr : r->d_offsets.p; a.precision_mode = c.precision_mode;
    a.heads = r->d_heads.p; a.prec = r->d_prec.p; a.nwords = r->d_nwords.p; a.draws = r->d_draws.p;
    a.sizes = c.s_sizes.as<uint32_t>(); a.status = c.s_status.as<uint32_t>();
    a.arena = c.s_arena.as<uint32_t>(); a.arena_stride = c.arena_stride;
    a.perm = c.pol.want_perm ? r->d_perm.p : nullptr;
    a.sid = c.s_sid.as<uint32_t>(); a.spos = nullptr; a.skey = nullptr; a.skey_off = nullptr; a.mt = ctx->d_mt;
    // VIDC_ENC_PRIO=<mask>: s_setprio 3 for the general wave-per-list class (1), the 64- / 32-word lane classes (2), the
    // position-bitmap chains (4).  Default 2: the few wavefronts of the 2049..4096-id lane classes run 4096 steps ahead of the other
    // lane launches of their stream, and a step of theirs takes 9.5 us next to the chain classes (2.3 alone); first in their SIMD's
    // arbitration the S2 encode is 53.5-53.9 instead of 54.7-55.6 ms (interleaved, profiles/r05v_s2_ab_enc_prio.txt; the other
    // classes: no effect)
    c.enc_prio = [] { const char *e = std::getenv("VIDC_ENC_PRIO"); return e ? std::atoi(e) : 2; }();
    a.dense = u2_dense() ? 1u : 0u;
    c.tr.mark("alloc + upload");
    return VIDC_OK;
}

// ---- the launches, one small function per kernel family (in this order: the code object holds the kernels in the order of their first use)
// (a kernel that can report input positions comes as a <.., true> / <.., false> pair: the call's want_perm picks)
template <class Kernel, class... Args>
int enc_launch(EncodeCall &c, Kernel with_perm, Kernel without, dim3 grid, size_t lds, hipStream_t st_, const Args &...args) {
    hipLaunchKernelGGL(c.pol.want_perm ? with_perm : without, grid, dim3(64), lds, st_, args...);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
int enc_launch_gen(EncodeCall &c, hipStream_t st_, const uint32_t *wl, uint32_t nwork, uint32_t rl_max) {
    if (!nwork) return VIDC_OK;
    RocEncArgs b = c.a;
    b.worklist = wl; b.nwork = nwork;
    if (c.enc_prio & 1) b.lpw = 0x80000000u;
    hipLaunchKernelGGL(k_roc_encode_gen, dim3(nwork), dim3(64), (size_t)64 * rl_max * 12, st_, b, rl_max);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
void enc_note_chain(EncodeCall &c, const std::vector<uint32_t> &w, uint32_t ub) {
    uint64_t tot = 0;
    for (uint32_t l : w) tot += c.len(l);
    c.ctx->chain_info[0][0] = tot; c.ctx->chain_info[0][1] = w.size(); c.ctx->chain_info[0][2] = c.len(w[0]); c.ctx->chain_info[0][3] = ub;
}
// universe-bitmap lists; the 20-bit launch (or, without one, the 18-bit launch) is the call's chain launch
template <int BITS>
int enc_launch_u(EncodeCall &c, hipStream_t st_) {
    vidc_ctx *ctx = c.ctx; constexpr int cls = BITS == 20 ? W_U20 : W_U18;
    const bool is_chain = BITS == 20 || c.wl(W_U20).empty();
    if (is_chain) { enc_note_chain(c, c.wl(cls), BITS); VIDC_HIP(hipEventRecord(ctx->ev_chain[0], st_)); }
    RocEncArgs b = c.a;
    b.worklist = c.d_wl + c.w.base(cls); b.nwork = (uint32_t)c.wl(cls).size();
    const U2Div *dt = (const U2Div *)ctx->d_u2tab;
    if (old_u_kernels()) {
        if constexpr (BITS == 20) {
            VIDC_TRY(set_big_lds((const void *)k_roc_encode_u<BITS, false>, UGeom<BITS>::LDS_BYTES));
            VIDC_TRY(set_big_lds((const void *)k_roc_encode_u<BITS, true>, UGeom<BITS>::LDS_BYTES));
        }
        VIDC_TRY(enc_launch(c, k_roc_encode_u<BITS, true>, k_roc_encode_u<BITS, false>, dim3(b.nwork), UGeom<BITS>::LDS_BYTES, st_, b));
    } else {
        const uint32_t lds = u2_enc_lds_bytes<BITS>(b.dense != 0u);  // (one workgroup per CU with either body)
        if constexpr (BITS == 20) {
            VIDC_TRY(set_big_lds((const void *)k_roc_encode_u2<BITS, false>, lds));
            VIDC_TRY(set_big_lds((const void *)k_roc_encode_u2<BITS, true>, lds));
        }
        VIDC_TRY(enc_launch(c, k_roc_encode_u2<BITS, true>, k_roc_encode_u2<BITS, false>, dim3(b.nwork), lds, st_, b, dt));
    }
    if (is_chain) VIDC_HIP(hipEventRecord(ctx->ev_chain[1], st_));
    return VIDC_OK;
}
int enc_launch_r2(EncodeCall &c, hipStream_t st_r2);
// main stream: bitmap-20 lists and the deepest general class (the critical paths), position-bitmap chains
void enc_add_chains(EncodeCall &c) {
    const bool u20 = !c.wl(W_U20).empty(), r2 = !c.wl(W_R2).empty();
    // (bitmap-20 lists: the critical path of the 1 M-vector configurations)
    if (u20) c.L.push_back({"U20", 0, [&c](hipStream_t st_) { return enc_launch_u<20>(c, st_); }});
    // (behind a 20-bit bitmap launch on the main stream these chains would only start when that one has finished:
    // S1 encode 12.5 -> 13.5 ms; they go to the first auxiliary stream then)
    if (r2) c.L.push_back({"R2", u20 ? 1 : 0, [&c](hipStream_t st_) { return enc_launch_r2(c, st_); }});
    // the deepest class: prefix rows sized for its longest list (first of the work list).  With the fixed
    // 48 KiB layout a CU held 3 of these chains; lists up to 65 536 ids need 12 KiB (S2 encode 152 -> see DESIGN)
    // (behind a chain launch on the main stream it would only start when that one has finished)
    if (!c.wl(W_C3).empty())
        c.L.push_back({"C3", (r2 && !u20) ? 1 : 0, [&c](hipStream_t st_c3) -> int {
            const uint64_t nmax3 = c.len(c.wl(W_C3)[0]);
            uint32_t rl3 = 16;
            while ((uint64_t)64 * 64 * rl3 < nmax3) rl3 <<= 1;
            return enc_launch_gen(c, st_c3, c.d_wl + c.w.base(W_C3), (uint32_t)c.wl(W_C3).size(), rl3);
        }});
}
int enc_launch_r2(EncodeCall &c, hipStream_t st_r2) {
    RocEncArgs b = c.a;
    b.worklist = c.d_wl + c.w.base(W_R2); b.nwork = (uint32_t)c.wl(W_R2).size();
    if (c.enc_prio & 4) b.lpw = 0x80000000u;
    const U2Div *dt = (const U2Div *)c.ctx->d_u2tab;
    // (the bitmap of a launch whose longest list -- the first of the work list -- has at most 65 536 positions: 8 KiB)
    if (c.len(c.wl(W_R2)[0]) <= 65536) return enc_launch(c, k_roc_encode_r2<true, 10>, k_roc_encode_r2<false, 10>, dim3(b.nwork), VIDC_R2_LDS_BYTES(10), st_r2, b, dt);
    return enc_launch(c, k_roc_encode_r2<true, 12>, k_roc_encode_r2<false, 12>, dim3(b.nwork), VIDC_R2_LDS_BYTES(12), st_r2, b, dt);
}
// row-per-list kernels: one launch per octave of list length (grp_segments)
void enc_add_grp(EncodeCall &c, int cls, size_t &seg_no) {
    // Every launch is latency-bound (its duration is its longest list's chain) and light on issue slots, so the octaves
    // must overlap: they alternate between the first and the third auxiliary stream (the lane classes own the second).
    // stream digit per segment (0 = main, 1.. = auxiliary; wide: the last auxiliary stream is the plan upload's: ADVICE round 4)
    const char *gmap = c.ctx->wide ? "456" : "13";
    const size_t gmap_n = std::strlen(gmap), wbase = c.w.base(cls);
    const bool lev3 = cls == W_G3;
    int seg_of_class = 0;
    for (const GrpSegment &s : grp_segments(c.wl(cls), c.r->offsets.data())) {
        const int sd = gmap[seg_no++ % gmap_n] - '0';
        c.L.push_back({std::string(lev3 ? "G3." : "G2.") + std::to_string(seg_of_class++), (sd >= 1 && sd <= c.ctx->naux()) ? sd : 0,
                       [&c, n0 = s.longest, nwork = (uint32_t)s.count, woff = wbase + s.first, lev3](hipStream_t st_g) -> int {
            const U2Div *dt = (const U2Div *)c.ctx->d_u2tab;
            RocEncArgs b = c.a;
            b.worklist = c.d_wl + woff; b.nwork = nwork;
            const uint32_t nblk = (uint32_t)((n0 + 511) >> 9);
            const size_t lds = (size_t)4 * 4 * (lev3 ? roc_grp_enc_lds_words<3>(nblk) : roc_grp_enc_lds_words<2>(nblk));
            const dim3 grid((b.nwork + 3u) / 4u);
            if (lev3 && lds > 65536) {
                VIDC_TRY(set_big_lds((const void *)k_roc_encode_grp<3, true>, lds));
                VIDC_TRY(set_big_lds((const void *)k_roc_encode_grp<3, false>, lds));
            }
            if (lev3) return enc_launch(c, k_roc_encode_grp<3, true>, k_roc_encode_grp<3, false>, grid, lds, st_g, b, dt, nblk);
            return enc_launch(c, k_roc_encode_grp<2, true>, k_roc_encode_grp<2, false>, grid, lds, st_g, b, dt, nblk);
        }});
    }
}
void enc_add_gen(EncodeCall &c, int cls, int sdef) {  // C2 / C1: mid-size and short general lists
    if (c.wl(cls).empty()) return;
    c.L.push_back({cls == W_C2 ? "C2" : "C1", sdef, [&c, cls](hipStream_t st_) {
        return enc_launch_gen(c, st_, c.d_wl + c.w.base(cls), (uint32_t)c.wl(cls).size(), cls == W_C2 ? 8 : 1);
    }});
}
template <int NW>
int enc_launch_lane(EncodeCall &c, hipStream_t st_, const RocEncArgs &b) {
    const dim3 grid((b.nwork + (b.lpw & 0xffffu) - 1u) / (b.lpw & 0xffffu));
    return enc_launch(c, k_roc_encode_lane<NW, true>, k_roc_encode_lane<NW, false>, grid, 0, st_, b, (const LaneDiv *)c.ctx->d_ltab);
}
// aux 0: mid-size general lists (calls without lane classes) and bitmap-18 lists; aux 1: the lane-per-list kernels, then the general classes
void enc_add_short_classes(EncodeCall &c) {
    const bool lanes_present = !c.wl(W_L4).empty() || !c.wl(W_L16).empty() || !c.wl(W_L64).empty();
    if (!lanes_present) enc_add_gen(c, W_C2, 1);
    if (!c.wl(W_U18).empty()) c.L.push_back({"U18", 1, [&c](hipStream_t st_) { return enc_launch_u<18>(c, st_); }});
    if (!lanes_present) enc_add_gen(c, W_C1, 2);
    for (int cls = W_L64; cls >= W_L4; cls--) {  // longest chains first
        const std::vector<uint32_t> &w = c.wl(cls);
        if (w.empty()) continue;
        RocEncArgs b = c.a;
        b.worklist = c.d_wl + c.w.base(cls); b.nwork = (uint32_t)w.size();
        // (LDS per wavefront: 4-word strips 14.3 KiB, 16-word 21.5 KiB, 32-word 31.5 KiB, 64-word 50.5 KiB)
        b.lpw = lane_lists_per_wave(c.ctx, b.nwork, cls == W_L4 ? 15 : cls == W_L16 ? 11 : 4);
        if (cls == W_L64) {
            // lists are sorted longest first: the leading wavefronts need the 64-word strips (50.5 KiB of LDS,
            // 3 per CU), everything from the first wavefront whose longest list has <= 2048 ids the 32-word
            // ones (31.5 KiB, 5 per CU)
            uint32_t n_big = 0;
            while (n_big < b.nwork && c.len(w[n_big]) > 2048) n_big++;
            n_big = std::min<uint32_t>(b.nwork, (n_big + b.lpw - 1u) / b.lpw * b.lpw);
            if (c.enc_prio & 2) b.lpw |= 0x80000000u;
            RocEncArgs b2 = b;
            b2.worklist = b.worklist + n_big; b2.nwork = b.nwork - n_big;
            b.nwork = n_big;
            if (b.nwork) c.L.push_back({"L64", 2, [&c, b](hipStream_t st_) { return enc_launch_lane<64>(c, st_, b); }});
            if (b2.nwork) c.L.push_back({"L32", 2, [&c, b2](hipStream_t st_) { return enc_launch_lane<32>(c, st_, b2); }});
        } else if (cls == W_L4) c.L.push_back({"L4", 2, [&c, b](hipStream_t st_) { return enc_launch_lane<4>(c, st_, b); }});
        else c.L.push_back({"L16", 2, [&c, b](hipStream_t st_) { return enc_launch_lane<16>(c, st_, b); }});
    }
    if (lanes_present) { enc_add_gen(c, W_C2, 2); enc_add_gen(c, W_C1, 2); }
}
int enc_launch_tiny(EncodeCall &c, hipStream_t st_) {
    const bool rows = c.rows; const uint32_t K = c.K;
    RocEncArgs b = c.a;
    b.worklist = rows ? nullptr : c.d_wl; b.nwork = (uint32_t)c.ntiny;
    if (c.use.lane_tiny) {  // one list per lane (roc_lane.h)
        const dim3 grid((b.nwork + 63u) / 64u);
        const LaneDiv *dt = (const LaneDiv *)c.ctx->d_ltab;
        if (rows && K == 32) hipLaunchKernelGGL((k_roc_encode_tiny_lane<32, true, true>), grid, dim3(64), 0, st_, b, dt);
        else if (rows && K == 64) hipLaunchKernelGGL((k_roc_encode_tiny_lane<64, true, true>), grid, dim3(64), 0, st_, b, dt);
        else if (rows && K < 32) hipLaunchKernelGGL((k_roc_encode_tiny_lane<32, true>), grid, dim3(64), 0, st_, b, dt);
        else if (rows) hipLaunchKernelGGL((k_roc_encode_tiny_lane<64, true>), grid, dim3(64), 0, st_, b, dt);
        else hipLaunchKernelGGL((k_roc_encode_tiny_lane<64, false>), grid, dim3(64), 0, st_, b, dt);
    } else if (rows) hipLaunchKernelGGL(k_roc_encode_tiny<true>, dim3(b.nwork), dim3(64), 0, st_, b);
    else hipLaunchKernelGGL(k_roc_encode_tiny<false>, dim3(b.nwork), dim3(64), 0, st_, b);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
// Kernel classes run concurrently (one stream each): the longest chains on the caller's stream, shorter
// classes on the auxiliary streams so that they fill the wave slots the long chains leave idle.
void enc_build_launches(EncodeCall &c) {
    enc_add_chains(c);
    // The lane-per-list kernels and the throughput-bound general classes must not share the machine: on S2 the
    // 64-word lane class took 69 ms next to the 26 316-list general class (49 ms) -- 9 ms and ~35 ms when each
    // has the CUs to itself (the lane strips take 141 KiB of a CU's LDS, the general waves the issue slots).
    // With lane classes in the call they go first on aux 1 and the general classes queue behind them; the long
    // chains on the main stream overlap with all of it.
    size_t seg_no = 0;
    enc_add_grp(c, W_G3, seg_no);
    enc_add_grp(c, W_G2, seg_no);
    enc_add_short_classes(c);
    if (c.ntiny) c.L.push_back({"TINY", 3, [&c](hipStream_t st_) { return enc_launch_tiny(c, st_); }});  // aux 2
}

// an auxiliary stream joins the call at its first launch (and only those are joined at the end: a small call that uses
// one of them does not pay event traffic for seven)
inline hipStream_t enc_fork(EncodeCall &c, int i) {
    if (!(c.aux_used >> i & 1u)) { (void)hipStreamWaitEvent(c.ctx->aux[i], c.ctx->ev_fork, 0); c.aux_used |= 1u << i; }
    return c.ctx->aux[i];
}
// fork, the launches in the default or the VIDC_ENC_SCHED order, join
int enc_run_launches(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; std::vector<EncLaunch> &L = c.L;
    VIDC_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    // A call without a class for the caller's stream (no bitmap-20, deepest-general or position-bitmap lists: e.g. an index
    // of equal-sized short lists, graph rows) gives that stream to the first auxiliary class it launches: the class then
    // starts without the fork event and the call ends without its join (65 536 lists of 256 ids: ~0.1 ms of idle GPU
    // between the event records of the encode).
    const bool main_idle = c.wl(W_U20).empty() && c.wl(W_C3).empty() && c.wl(W_R2).empty();
    int promoted = -1;
    const bool serial = env_on("VIDC_SERIAL");  // measurements: every class on the caller's stream, one after the other
    auto stream_no = [&](int sno) -> hipStream_t {  // a launch's default stream
        if (serial || sno == 0) return ctx->stream;
        if (main_idle && (promoted < 0 || promoted == sno - 1)) { promoted = sno - 1; return ctx->stream; }
        return enc_fork(c, sno - 1);
    };
    ctx->chain_info[0][0] = ctx->chain_info[0][1] = ctx->chain_info[0][2] = ctx->chain_info[0][3] = 0;
    ctx->phase_ms[VIDC_PHASE_ROC_ENCODE_CHAIN] = 0;
    enc_build_launches(c);
    // The schedule.  This site's rules (the decoder's differ, see decode_impl): a name's second entry is ignored; a round without
    // progress (a cycle) drops ALL dependencies and goes on; the 24 PhaseTimer events of the context double as "launch i has been
    // queued" markers, so only the first 24 launches can be waited for (other dependencies are dropped, not aliased), and an event
    // is only recorded for a launch that something waits for (no VIDC_ENC_SCHED: none at all).
    std::vector<SchedEntry> sched;
    if (const char *e = std::getenv("VIDC_ENC_SCHED")) {
        auto find = [&](const std::string &t) { for (size_t i = 0; i < L.size(); i++) if (L[i].name == t) return (int)i; return -1; };
        sched = parse_schedule(e, find, ctx->naux(), true);
        std::stable_sort(sched.begin(), sched.end(), [](const SchedEntry &x, const SchedEntry &y) { return x.pos < y.pos; });
    }
    std::vector<char> named(L.size(), 0), waited_on(L.size(), 0), done(L.size(), 0);
    for (const SchedEntry &it : sched) named[it.item] = 1;
    for (size_t i = 0; i < L.size(); i++) if (!named[i]) sched.push_back({(int)i, -1, 0, {}});
    for (SchedEntry &it : sched) {
        it.deps.erase(std::remove_if(it.deps.begin(), it.deps.end(), [](int d) { return d >= 24; }), it.deps.end());
        for (int d : it.deps) waited_on[d] = 1;
    }
    VIDC_TRY(run_schedule(sched, done, true, [&](const SchedEntry &it) -> int {
        hipStream_t st_ = serial || it.group == 0 ? ctx->stream : it.group > 0 ? enc_fork(c, it.group - 1) : stream_no(L[it.item].def_stream);
        for (int d : it.deps) VIDC_HIP(hipStreamWaitEvent(st_, ctx->tev[d], 0));
        VIDC_TRY(L[it.item].fn(st_));
        if (waited_on[it.item]) VIDC_HIP(hipEventRecord(ctx->tev[it.item], st_));
        return VIDC_OK;
    }));
    for (int i = 0; i < ctx->naux(); i++) {
        if (!(c.aux_used >> i & 1u)) continue;
        VIDC_HIP(hipEventRecord(ctx->ev_join[i], ctx->aux[i]));
        VIDC_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
    }
    return VIDC_OK;
}

// the kernels are in flight and the host has nothing to do until they finish: plan the decode of the whole
// object now (7 ms per million lists that decode_all would otherwise spend on its critical path)
int enc_plan_ahead(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    const uint64_t nlist = c.nlist;
    if (c.pre_deferred) {  // the maxima of the lists: precisions and bucket geometry for the decode planner
        VIDC_HIP(vidc::vidc_event_wait(ctx->ev_pre[2]));
        const uint32_t *mx = c.h_pre.as<uint32_t>();
        r->umax.assign(mx, mx + nlist);
        for (uint64_t l = 0; l < nlist; l++) r->prec[l] = prec_from_max(c.offsets[l + 1] - c.offsets[l], mx[l], c.precision_mode);
        float pms = 0;
        if (hipEventElapsedTime(&pms, ctx->ev_pre[0], ctx->ev_pre[1]) == hipSuccess) c.kernel_ms += pms;
    }
    if (c.rows || nlist < PLAN_AHEAD_MIN_LISTS || r->prec.size() != nlist) return VIDC_OK;
    r->plan_ahead = plan_ahead_build(r, ctx->wide);
    // ... and send its work list and scratch offsets to the device behind the kernels (decode_all then finds the
    // plan complete: 0.04 ms of its critical path at 65 536 lists)
    DecPlanCache &pc = *r->plan_ahead;
    const size_t ni = pc.plan.wl.size();
    if (!ni || pc.plan.lean) return VIDC_OK;
    VIDC_TRY(c.h_plan.get(ctx, ni * 20));
    uint64_t *h64 = c.h_plan.as<uint64_t>();
    uint32_t *h32 = (uint32_t *)(h64 + 2 * ni);
    std::memcpy(h64, pc.plan.scratch_off.data(), ni * 8);
    std::memcpy(h64 + ni, pc.plan.slots_off.data(), ni * 8);
    std::memcpy(h32, pc.plan.wl.data(), ni * 4);
    VIDC_TRY(pc.d_scratch_off.alloc(ni, ctx->dpool)); VIDC_TRY(pc.d_slots_off.alloc(ni, ctx->dpool)); VIDC_TRY(pc.d_wl.alloc(ni, ctx->dpool));
    // (on a stream of their own -- the last auxiliary one, which no kernel class of this call uses --: behind the
    // kernels on the caller's stream the 1.3 MB of a 65 536-list plan were 0.06 ms more before the call's wait)
    hipStream_t cs = ctx->aux[VIDC_NAUX - 1];
    VIDC_HIP(hipMemcpyAsync(pc.d_scratch_off.p, h64, ni * 8, hipMemcpyHostToDevice, cs));
    VIDC_HIP(hipMemcpyAsync(pc.d_slots_off.p, h64 + ni, ni * 8, hipMemcpyHostToDevice, cs));
    VIDC_HIP(hipMemcpyAsync(pc.d_wl.p, h32, ni * 4, hipMemcpyHostToDevice, cs));
    VIDC_HIP(hipEventRecord(ctx->ev_join[VIDC_NAUX - 1], cs));
    VIDC_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[VIDC_NAUX - 1], 0));
    c.plan_on_device = true;
    return VIDC_OK;
}

// second pass for lists the first pass handed back: unsorted input of the general kernels (Faiss
// lists are in add order, i.e. normally sorted) and multiset input of the bitmap kernels
int enc_second_pass(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    const uint64_t nlist = c.nlist;
    std::vector<uint32_t> &pend = c.pend;
    if (c.rows || !nlist) return VIDC_OK;
    // how many lists are pending: the summary came back with the sizes, the status array only if there are any
    if (c.tail.t[3]) {
        std::vector<uint32_t> status;
        VIDC_TRY(download(ctx, status, c.s_status.as<uint32_t>(), nlist));
        for (uint64_t l = 0; l < nlist; l++)
            if (status[l] == VIDC_ST_PENDING_SORT) pend.push_back((uint32_t)l);
    }
    if (pend.empty()) return VIDC_OK;
    sort_desc(pend, r->offsets);
    std::vector<uint64_t> skey_off(nlist + 1, 0);
    uint32_t maxn = 0;
    {
        std::vector<uint8_t> is_p(nlist, 0);
        for (uint32_t l : pend) is_p[l] = 1;
        for (uint64_t l = 0; l < nlist; l++) {
            uint64_t n = r->offsets[l + 1] - r->offsets[l], p2 = 0;
            if (is_p[l]) { p2 = 1; while (p2 < n) p2 <<= 1; maxn = std::max<uint32_t>(maxn, (uint32_t)n); }
            skey_off[l + 1] = skey_off[l] + p2;
        }
    }
    Scratch s_skey, s_skey_off, s_spos, s_pend;
    VIDC_TRY(s_skey.get(ctx, skey_off[nlist] * 8));
    VIDC_TRY(upload_scratch(ctx, s_skey_off, skey_off));
    VIDC_TRY(s_spos.get(ctx, c.ntotal_in * 4));
    if (!c.s_sid.p) VIDC_TRY(c.s_sid.get(ctx, c.ntotal_in * 4));
    VIDC_TRY(upload_scratch(ctx, s_pend, pend));
    c.a.sid = c.s_sid.as<uint32_t>();
    c.a.skey = s_skey.as<uint64_t>(); c.a.skey_off = s_skey_off.as<uint64_t>(); c.a.spos = s_spos.as<uint32_t>();
    uint32_t rl_max = maxn <= 4096 ? 1 : (maxn <= 32768 ? 8 : (maxn <= 65536 ? 16 : 64));
    EventTimer t2 = EventTimer::started(ctx);
    VIDC_TRY(enc_launch_gen(c, ctx->stream, s_pend.as<uint32_t>(), (uint32_t)pend.size(), rl_max));
    c.kernel_ms += t2.stop();
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // scratch of this scope is released below
    if (c.light_prepass) {
        // the precision of these lists came from their last id, which was not their maximum if they were not
        // ascending: the general kernel stored the real one
        std::vector<uint32_t> dp;
        VIDC_TRY(download(ctx, dp, r->d_prec.p, nlist));
        for (uint32_t l : pend) { r->prec[l] = dp[l]; r->umax[l] = 0; }
        r->plan_ahead.reset();
    }
    // statuses and word counts of the redone lists: summary and offsets again
    VIDC_TRY(finish_enqueue(ctx, r, c.tail, c.s_status, c.s_sizes.as<uint32_t>()));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    return VIDC_OK;
}

// bitmap-kernel lists wrote sampled ids into the perm buffer: turn them into input positions
int enc_perm_from_order(EncodeCall &c) {
    vidc_ctx *ctx = c.ctx; vidc_roc *r = c.r.get();
    if (!c.pol.want_perm || (c.wl(W_U18).empty() && c.wl(W_U20).empty())) return VIDC_OK;
    std::vector<uint8_t> is_p(c.nlist, 0);
    for (uint32_t l : c.pend) is_p[l] = 1;
    std::vector<uint32_t> ul;
    for (uint32_t l : c.wl(W_U18)) if (!is_p[l]) ul.push_back(l);
    for (uint32_t l : c.wl(W_U20)) if (!is_p[l]) ul.push_back(l);
    if (ul.empty()) return VIDC_OK;
    const std::vector<uint32_t> items = perm_items(ul, r->offsets.data(), VIDC_PERM_CHUNK);
    Scratch s_ul;
    VIDC_TRY(upload_scratch(ctx, s_ul, items));
    const uint32_t nitems = (uint32_t)(items.size() / 2);
    EventTimer t = EventTimer::started(ctx);
    hipLaunchKernelGGL(k_perm_from_order, dim3(nitems), dim3(256), 0, ctx->stream, c.d_ids, r->d_offsets.p, s_ul.as<uint2>(), nitems, r->d_perm.p);
    VIDC_HIP(hipGetLastError());
    c.kernel_ms += t.stop();
    return VIDC_OK;
}

// The host call of every ROC encode (IVF lists; graph rows: rows == true, a short path through the same stages).  The planning
// -- which kernel class takes which list, in which order -- is roc_enc_plan.h; the stages above queue what it decided.
int encode_impl(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, bool rows, uint64_t N,
                uint32_t K, const int32_t *d_rows, int precision_mode, uint32_t flags, vidc_roc **out) {
    if (!ctx || !out) return VIDC_ERR_INVALID;
    *out = nullptr;
    if (precision_mode < VIDC_PREC_EXACT || precision_mode > 32) {
        set_error("precision_mode %d unsupported (fixed precision must be 0..32)", precision_mode);
        return VIDC_ERR_INVALID;
    }
    if (nlist >= 0xffffffffull || N >= 0xffffffffull) { set_error("too many lists"); return VIDC_ERR_INVALID; }
    VIDC_HIP(hipSetDevice(ctx->device));
    EncodeCall c{ctx, rows ? N : nlist, offsets, d_ids, rows, K, d_rows, precision_mode};
    VIDC_TRY(enc_begin(c, N, flags));
    if (!rows) {
        VIDC_TRY(enc_scan_offsets(c));
        VIDC_TRY(enc_prepass(c));
        VIDC_TRY(enc_classify(c));
    }
    VIDC_TRY(enc_upload_worklists(c));
    EventTimer t = EventTimer::started(ctx);
    VIDC_TRY(enc_run_launches(c));
    // (the end event is recorded first: the planning is host time, not part of the kernels' duration)
    (void)t.mark();
    VIDC_TRY(finish_enqueue(ctx, c.r.get(), c.tail, c.s_status, c.s_sizes.as<uint32_t>()));
    VIDC_TRY(enc_plan_ahead(c));
    // ONE wait for the kernels, the status summary and the sizes (queued behind the kernels above)
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    c.pre_guard.disarm();
    c.kernel_ms += t.elapsed();
    if (ctx->chain_info[0][3]) {  // (the main stream joined the auxiliary ones)
        float cms = 0;
        if (hipEventElapsedTime(&cms, ctx->ev_chain[0], ctx->ev_chain[1]) == hipSuccess) ctx->phase_ms[VIDC_PHASE_ROC_ENCODE_CHAIN] = cms;
    }
    c.tr.mark("encode kernels (sync)");
    VIDC_TRY(enc_second_pass(c));
    VIDC_TRY(enc_perm_from_order(c));
    c.tr.mark("second pass / perm");
    ctx->phase_ms[VIDC_PHASE_ROC_ENCODE] = c.kernel_ms;
    VIDC_TRY(finish_complete(ctx, c.r.get(), c.tail, c.s_arena.as<uint32_t>(), c.arena_stride, c.s_status, c.nonempty, c.kernel_ms));
    c.tr.mark("metadata + compaction");
    ctx->last_kernel_ms = c.kernel_ms;
    if (c.plan_on_device && c.r->plan_ahead) c.r->plan_all = std::move(c.r->plan_ahead);  // (a sorting second pass drops the plan)
    *out = c.r.release();
    return VIDC_OK;
}

// ---- decode.  The planning -- which kernel class takes which work item, where its scratch and slots lie, which queue runs which
// class -- is roc_dec_plan.h; plan_decode fills its policy from the environment and the context, the dec_* stages below queue what
// it decided.
inline DecView dec_view(const vidc_roc *r) {
    DecView v;
    v.offsets = r->offsets.data(); v.prec = r->prec.data();
    v.umax = r->umax.data(); v.n_umax = r->umax.size();
    v.nwords = r->meta_host ? r->nwords.data() : nullptr;
    v.order_desc = r->order_desc.data(); v.n_order = r->order_desc.size(); v.order_max_n = r->order_max_n;
    return v;
}
// lists[i] = list number of request item i (a list may appear more than once)
// only_general: the caller decodes into int32 rows (wide graph rows): only the kernels that honour out_rows -- the tiny
// and the general wave-per-list decoders -- may be planned.  whole_sorted, allow_b2, wide: roc_dec_plan.h
void plan_decode(const vidc_roc *r, const std::vector<uint32_t> &lists, bool rows_flavour, DecPlan &p, bool wide,
                 bool allow_lane = true, bool allow_b2 = true, bool only_general = false, bool whole_sorted = false) {
    DecPolicy pol;
    pol.f_general = force_general() || only_general;
    if (only_general) { allow_lane = false; allow_b2 = false; }
    pol.lpol = (allow_lane && !pol.f_general) ? lane_policy() : LANE_NEVER;
    if (plan_decode_lean(lists, rows_flavour, pol, DEC_LIMITS, p)) return;
    pol.wide = wide;
    pol.gpol = grp_policy();
    pol.pair = !env_on("VIDC_NO_LANE_PAIR") && !env_on("VIDC_NO_LANE_REG");
    pol.quad = env_on("VIDC_LANE_QUAD") && pol.pair;
    pol.nb128 = !env_on("VIDC_NO_LANE128");
    pol.pair_min = VIDC_LANE_REG_MAX;
    if (const char *e = std::getenv("VIDC_PAIR_MIN")) pol.pair_min = std::min<uint64_t>(VIDC_LANE_REG_MAX, std::max<uint64_t>(TINY_MAX, (uint64_t)std::atoll(e)));
    pol.no_length_classes = whole_sorted && env_on("VIDC_NO_LENGTH_CLASSES");
    pol.old_u = old_u_kernels();
    pol.no_r2 = env_on("VIDC_NO_R2");
    const char *ae = std::getenv("VIDC_LANE_ALIGN");
    pol.lane_align = ae ? (std::atoi(ae) >= 16 ? 16u : 4u) : VIDC_LANE_ALIGN_DEFAULT;
    const size_t ni = lists.size();
    p.item = vec_pool<uint32_t>().take(ni); p.wl = vec_pool<uint32_t>().take(ni);
    p.scratch_off = vec_pool<uint64_t>().take(ni); p.slots_off = vec_pool<uint64_t>().take(ni);
    plan_decode_classes(dec_view(r), lists, rows_flavour, allow_b2, whole_sorted, pol, DEC_LIMITS, p);
}

// One decode call: its arguments, its scratch and staging blocks, the kernels' common arguments, and what one stage leaves for the
// next.  The stages (dec_*) run in the order decode_impl lists them.
struct DecodeCall {
    vidc_ctx *ctx; const vidc_roc *r; const DecPlan &p;
    const uint64_t *out_off_host; uint64_t *d_out; int32_t *d_out_rows; uint32_t K;
    const DecPlanCache *cache;
    size_t nwork;
    HostTrace tr{"roc decode"};
    Scratch s_wl, s_scr_off, s_slots_off, s_scr, s_slots, s_out_off, s_end;
    Pinned h_up, h_sum;
    const uint32_t *d_wl = nullptr;
    const uint64_t *d_scr_off = nullptr, *d_slots_off = nullptr;
    uint32_t *d_status = nullptr;
    RocDecArgs a{};                   // what every launch of the call shares
    size_t base[DC_COUNT] = {};       // first work item of every class
    int order[DC_COUNT] = {};         // the classes, longest estimated duration first
    hipStream_t stream_of[DC_COUNT] = {};
    std::vector<SchedEntry> sched;    // VIDC_DEC_SCHED
    int chain_class = -1;
    uint32_t aux_used = 0;            // only the auxiliary streams that carry a class of this call are forked and joined
    EventTimer t;
    unsigned long long *sum = nullptr;  // the status summary, in pinned memory
    DecodeCall(vidc_ctx *ctx_, const vidc_roc *r_, const DecPlan &p_, const uint64_t *out_off_host_, uint64_t *d_out_, int32_t *d_out_rows_,
               uint32_t K_, const DecPlanCache *cache_, size_t nwork_)
        : ctx(ctx_), r(r_), p(p_), out_off_host(out_off_host_), d_out(d_out_), d_out_rows(d_out_rows_), K(K_), cache(cache_), nwork(nwork_), t(ctx_) {}
};
constexpr uint32_t DEC_RETRY_SLOTS = 504;  // list numbers of handed-back lists behind the eight summary words

// work list, scratch / slot offsets and output offsets to the device (a cached plan's are there already), the call's scratch,
// and the kernels' common arguments
int dec_upload(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx; const vidc_roc *r = c.r; const DecPlan &p = c.p;
    const size_t nwork = c.nwork;
    if (c.cache) {  // (decode_all: the object's own offsets place the output)
        c.d_wl = c.cache->d_wl.p; c.d_scr_off = c.cache->d_scratch_off.p; c.d_slots_off = c.cache->d_slots_off.p;
    } else if (p.implicit) {
        c.d_wl = p.order_dev;
    } else {
        // one pinned staging block for everything that goes up: work list | scratch offsets | slot offsets | out offsets
        const size_t n8 = p.lean ? 0 : nwork;
        VIDC_TRY(c.h_up.get(ctx, nwork * 4 + 8 + n8 * 24));
        uint32_t *h_wl = c.h_up.as<uint32_t>();
        uint64_t *h_64 = (uint64_t *)((char *)c.h_up.p + ((nwork * 4 + 7) & ~(size_t)7));
        std::memcpy(h_wl, p.wl.data(), nwork * 4);
        VIDC_TRY(c.s_wl.get(ctx, nwork * 4));
        VIDC_HIP(hipMemcpyAsync(c.s_wl.p, h_wl, nwork * 4, hipMemcpyHostToDevice, ctx->stream));
        c.d_wl = c.s_wl.as<uint32_t>();
        if (!p.lean) {
            std::memcpy(h_64, p.scratch_off.data(), nwork * 8);
            std::memcpy(h_64 + nwork, p.slots_off.data(), nwork * 8);
            VIDC_TRY(c.s_scr_off.get(ctx, nwork * 8));
            VIDC_TRY(c.s_slots_off.get(ctx, nwork * 8));
            VIDC_HIP(hipMemcpyAsync(c.s_scr_off.p, h_64, nwork * 8, hipMemcpyHostToDevice, ctx->stream));
            VIDC_HIP(hipMemcpyAsync(c.s_slots_off.p, h_64 + nwork, nwork * 8, hipMemcpyHostToDevice, ctx->stream));
            c.d_scr_off = c.s_scr_off.as<uint64_t>(); c.d_slots_off = c.s_slots_off.as<uint64_t>();
            if (c.out_off_host) {
                std::memcpy(h_64 + 2 * nwork, c.out_off_host, nwork * 8);
                VIDC_TRY(c.s_out_off.get(ctx, nwork * 8));
                VIDC_HIP(hipMemcpyAsync(c.s_out_off.p, h_64 + 2 * nwork, nwork * 8, hipMemcpyHostToDevice, ctx->stream));
            }
        }
    }
    VIDC_TRY(c.s_scr.get(ctx, p.scratch_words * 4));
    VIDC_TRY(c.s_slots.get(ctx, p.slots_words * 4));
    VIDC_TRY(c.s_end.get(ctx, r->nlist * 8 + 64));  // end states | statuses | summary accumulators: one block, one memset
    VIDC_HIP(hipMemsetAsync(c.s_end.p, 0, r->nlist * 8 + 64, ctx->stream));
    c.d_status = c.s_end.as<uint32_t>() + r->nlist;
    c.tr.mark("scratch + uploads");
    RocDecArgs &a = c.a;
    a.offsets = r->d_offsets.p;
    a.heads = r->d_heads.p; a.prec = r->d_prec.p; a.nwords = r->d_nwords.p; a.draws = r->d_draws.p;
    a.words = r->d_words.p; a.word_off = r->d_word_off.p;
    a.out = c.d_out; a.out_rows = c.d_out_rows; a.K = c.K;
    a.out_by_list = (p.implicit && p.order_dev && !p.order_req) ? 1u : 0u;
    a.scratch_words = c.s_scr.as<uint32_t>();
    a.slots = c.s_slots.as<uint32_t>();
    a.end_state = c.s_end.as<uint32_t>(); a.status = c.d_status;
    a.mt = ctx->d_mt;
    size_t acc = 0;
    for (int k = 0; k < DC_COUNT; k++) { c.base[k] = acc; acc += p.count[k]; }
    return VIDC_OK;
}
// rows by edge count, most edges first: histogram per workgroup, segment starts, scatter
int dec_build_row_order(DecodeCall &c) {
    const DecPlan &p = c.p;
    if (!p.order_build) return VIDC_OK;
    hipStream_t st = c.ctx->stream;
    const uint32_t nwork = (uint32_t)c.nwork;
    uint32_t *part = const_cast<uint32_t *>(p.order_dev) + c.nwork;
    hipLaunchKernelGGL(k_rows_order_hist, dim3(VIDC_ORDER_BLOCKS), dim3(256), 0, st, c.r->d_offsets.p, nwork, part);
    hipLaunchKernelGGL(k_rows_order_starts, dim3(1), dim3(128), 0, st, part);
    hipLaunchKernelGGL(k_rows_order_scatter, dim3(VIDC_ORDER_BLOCKS), dim3(256), 0, st, c.r->d_offsets.p, nwork, part, const_cast<uint32_t *>(p.order_dev));
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
// classes run concurrently: the longest chains on the caller's stream, the rest on the auxiliary streams (dec_assign_queues:
// queue 0 = the caller's stream, i = auxiliary stream i - 1)
int dec_assign_streams(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx; const DecPlan &p = c.p;
    // three streams: a 4th one did not run concurrently (HIP maps streams onto 4 hardware queues and the
    // process has other streams; the kernels of aux[2] started when the main stream's had finished)
    // (wide: a stream per class.  S2 decode by stream count, final kernel set (row decoder up to 16 384 ids, lane-pair register
    // decoder): 78-79 ms with 8, 84-85 with 6 -- a class queued behind the lane-pair launch, whose 256-VGPR wavefronts are slow
    // to find room, becomes the tail; without that decoder 81-82 / 83-84)
    int nq = ctx->wide ? VIDC_NAUX + 1 : 3;
    if (const char *e = std::getenv("VIDC_DEC_NQ")) nq = std::max(1, std::min(ctx->naux() + 1, std::atoi(e)));
    if (env_on("VIDC_SERIAL")) nq = 1;  // measurements: one class after the other
    int queue_of[DC_COUNT];
    dec_assign_queues(p.count, p.sum_n, p.max_n, nq, c.order, queue_of);
    for (int k = 0; k < DC_COUNT; k++) c.stream_of[k] = queue_of[k] > 0 ? ctx->aux[queue_of[k] - 1] : ctx->stream;
    ctx->chain_info[1][0] = ctx->chain_info[1][1] = ctx->chain_info[1][2] = ctx->chain_info[1][3] = 0;
    ctx->phase_ms[VIDC_PHASE_ROC_DECODE_CHAIN] = 0;
    c.chain_class = p.count[DC_U20] ? DC_U20 : (p.count[DC_U18] ? DC_U18 : -1);
    // VIDC_DEC_SCHED (measurements): explicit schedule (grammar: roc_enc_plan.h), e.g. "B2;GHUGE;LANEP,LANE,LANE64;GMID^LANEP"; "CLS^DEP"
    // waits for class DEP (on another stream) to finish.  Classes of the call the string does not name keep the automatic assignment.
    // This site's rules (the encoder's differ, see enc_run_launches): a class without lists in this call counts as unknown; a name's
    // second entry is kept and skipped by the loop; an event is recorded for every scheduled class; a round without progress (a
    // cycle) ends the loop and the rest is launched in order[].
    if (const char *e = std::getenv("VIDC_DEC_SCHED")) {
        auto cls_of = [&](const std::string &t) { const int k = dec_class_by_name(t); return k >= 0 && p.count[k] ? k : -1; };
        c.sched = parse_schedule(e, cls_of, ctx->naux(), false);
        for (const SchedEntry &it : c.sched) c.stream_of[it.item] = it.group == 0 ? ctx->stream : ctx->aux[it.group - 1];
    }
    return VIDC_OK;
}
int dec_fork(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx;
    VIDC_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int k = 0; k < DC_COUNT; k++)
        for (int i = 0; i < ctx->naux(); i++)
            if (c.p.count[k] && c.stream_of[k] == ctx->aux[i] && !(c.aux_used >> i & 1u)) {
                VIDC_HIP(hipStreamWaitEvent(ctx->aux[i], ctx->ev_fork, 0));
                c.aux_used |= 1u << i;
            }
    return VIDC_OK;
}

// ---- one launch function per kernel family: b = the class's arguments (its part of the work list and of the offset arrays)
using DecLaunchFn = int (*)(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st);
int dec_launch_tiny(DecodeCall &c, int, RocDecArgs &b, hipStream_t st) {
    if (c.p.tiny_lane) {  // one list per lane (roc_lane.h)
        const dim3 grid((b.nwork + 63u) / 64u);
        const LaneDiv *dt = (const LaneDiv *)c.ctx->d_ltab;
        if (c.d_out_rows) hipLaunchKernelGGL(k_roc_decode_tiny_lane<true>, grid, dim3(64), 0, st, b, dt);
        else hipLaunchKernelGGL(k_roc_decode_tiny_lane<false>, grid, dim3(64), 0, st, b, dt);
    } else if (c.d_out_rows) hipLaunchKernelGGL(k_roc_decode_tiny<true>, dim3(b.nwork), dim3(64), 0, st, b);
    else hipLaunchKernelGGL(k_roc_decode_tiny<false>, dim3(b.nwork), dim3(64), 0, st, b);
    return VIDC_OK;
}
int dec_launch_u(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // universe-bitmap kernels: ids < 2^18 / 2^20
    const U2Div *dt = (const U2Div *)c.ctx->d_u2tab;
    if (cls == DC_U18) {
        if (old_u_kernels()) hipLaunchKernelGGL(k_roc_decode_u<18>, dim3(b.nwork), dim3(64), UGeom<18>::LDS_BYTES, st, b);
        else hipLaunchKernelGGL((k_roc_decode_u2<18, false>), dim3(b.nwork), dim3(64), U2Geom<18>::DEC_LDS_BYTES, st, b, dt);
    } else if (old_u_kernels()) {
        VIDC_TRY(set_big_lds((const void *)k_roc_decode_u<20>, UGeom<20>::LDS_BYTES));
        hipLaunchKernelGGL(k_roc_decode_u<20>, dim3(b.nwork), dim3(64), UGeom<20>::LDS_BYTES, st, b);
    } else if (u2_dec_word()) {
        VIDC_TRY(set_big_lds((const void *)k_roc_decode_u2<20, true>, U2DecWord::LDS_BYTES));
        hipLaunchKernelGGL((k_roc_decode_u2<20, true>), dim3(b.nwork), dim3(64), U2DecWord::LDS_BYTES, st, b, dt);
    } else {
        VIDC_TRY(set_big_lds((const void *)k_roc_decode_u2<20, false>, U2Geom<20>::DEC_LDS_BYTES));
        hipLaunchKernelGGL((k_roc_decode_u2<20, false>), dim3(b.nwork), dim3(64), U2Geom<20>::DEC_LDS_BYTES, st, b, dt);
    }
    return VIDC_OK;
}
// general wave-per-list decoder: nf fine prefix counters of 16 bits in LDS
int dec_launch_gen(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {
    const uint32_t nf = cls == DC_GSMALL ? 512u : (cls == DC_G8K ? 1024u : (cls == DC_G16K ? 2048u : 1u << VIDC_DEC_MAX_FB));
    const uint32_t cap = cls == DC_GHUGE ? VIDC_DEC_CAP_BIG : VIDC_DEC_CAP;
    if (cls == DC_GSMALL && c.p.gsmall_lrows)  // member rows in LDS: 1 + 32 KiB
        hipLaunchKernelGGL((k_roc_decode_gen<uint16_t, true>), dim3(b.nwork), dim3(64), nf * 2 + nf * cap * 4, st, b, nf, cap);
    else
        hipLaunchKernelGGL(k_roc_decode_gen<uint16_t>, dim3(b.nwork), dim3(64), nf * 2, st, b, nf, cap);
    return VIDC_OK;
}
int dec_launch_lane(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // 12.5 KiB of LDS per wavefront
    vidc_ctx *ctx = c.ctx; const DecPlan &p = c.p;
    b.lpw = lane_lists_per_wave(ctx, b.nwork, 24);
    // lists are sorted longest first: those of <= 256 ids (the tail of the work list, from a wavefront
    // boundary on) take the decoder that keeps the decoded ids in registers
    uint32_t n_big = b.nwork;
    if (!std::getenv("VIDC_NO_LANE_REG") && !p.wl.empty()) {
        const uint32_t *wl0 = p.wl.data() + c.base[cls];
        n_big = (uint32_t)(std::partition_point(wl0, wl0 + b.nwork, [&](uint32_t l) {
                               return c.r->offsets[l + 1] - c.r->offsets[l] > VIDC_LANE_REG_MAX;
                           }) - wl0);
        n_big = std::min<uint32_t>(b.nwork, (n_big + b.lpw - 1u) / b.lpw * b.lpw);
    }
    RocDecArgs b2 = b;
    b2.worklist = b.worklist + n_big; b2.nwork = b.nwork - n_big;
    if (b2.out_off) b2.out_off += n_big;
    b.nwork = n_big;
    if (b.nwork && env_on("VIDC_LANE_LOOP"))
        hipLaunchKernelGGL((k_roc_decode_lane<64, false>), dim3((b.nwork + b.lpw - 1u) / b.lpw), dim3(64), 0, st, b,
                           (const LaneDiv *)ctx->d_ltab);
    else if (b.nwork)
        hipLaunchKernelGGL((k_roc_decode_lane<64, true>), dim3((b.nwork + b.lpw - 1u) / b.lpw), dim3(64), 0, st, b,
                           (const LaneDiv *)ctx->d_ltab);
    if (b2.nwork)
        hipLaunchKernelGGL(k_roc_decode_lane_reg<VIDC_LANE_REG_EL>, dim3((b2.nwork + b2.lpw - 1u) / b2.lpw), dim3(64), 0, st,
                           b2, (const LaneDiv *)ctx->d_ltab);
    return VIDC_OK;
}
int dec_launch_lane_nb(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // 256 buckets: 26.5 KiB of LDS per wavefront, 128: 18.5
    b.lpw = lane_lists_per_wave(c.ctx, b.nwork, 7);
    const dim3 grid((b.nwork + b.lpw - 1u) / b.lpw);
    const LaneDiv *dt = (const LaneDiv *)c.ctx->d_ltab;
    if (cls == DC_LANE64 && env_on("VIDC_LANE_LOOP")) hipLaunchKernelGGL((k_roc_decode_lane<256, false>), grid, dim3(64), 0, st, b, dt);
    else if (cls == DC_LANE64) hipLaunchKernelGGL((k_roc_decode_lane<256, true>), grid, dim3(64), 0, st, b, dt);
    else hipLaunchKernelGGL((k_roc_decode_lane<128, true>), grid, dim3(64), 0, st, b, dt);
    return VIDC_OK;
}
int dec_launch_b2(DecodeCall &c, int, RocDecArgs &b, hipStream_t st) {
    // (round 5 measured and dropped: the next step's candidate rows requested one step ahead -- 45.7 against 47.5 ms with
    // the class alone, 72.9 against 72.2 ms for the whole S2 decode: HISTORY.md)
    // VIDC_B2_MASK=1 / 0: the row load under exec = lanes below the bucket's member count (roc_u2.h, U2B_DEC_IDX_MC: a third
    // of the sectors, a later load) / the whole row at once.  Default: calls of many chains, whose rows come from HBM.
    const char *mke = std::getenv("VIDC_B2_MASK");
    const bool mk = mke ? mke[0] == '1' : b.nwork >= B2_MASK_MIN_CHAINS;
    if (mk) hipLaunchKernelGGL((k_roc_decode_b2<0, 2>), dim3(b.nwork), dim3(64), VIDC_B2_LDS_BYTES, st, b, (const U2Div *)c.ctx->d_u2tab);
    else hipLaunchKernelGGL(k_roc_decode_b2<0>, dim3(b.nwork), dim3(64), VIDC_B2_LDS_BYTES, st, b, (const U2Div *)c.ctx->d_u2tab);
    return VIDC_OK;
}
int dec_launch_b2l(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // 32 / 64 / 128 / 256 buckets, member rows in LDS: 8.3 / 16.5 / 33 / 66 KiB
    const U2Div *dt = (const U2Div *)c.ctx->d_u2tab;
    const dim3 grid(b.nwork);
    if (cls == DC_B2T) hipLaunchKernelGGL(k_roc_decode_b2<32>, grid, dim3(64), VIDC_B2L_LDS_BYTES(32u), st, b, dt);
    else if (cls == DC_B2S) hipLaunchKernelGGL(k_roc_decode_b2<64>, grid, dim3(64), VIDC_B2L_LDS_BYTES(64u), st, b, dt);
    else if (cls == DC_B2L) hipLaunchKernelGGL(k_roc_decode_b2<128>, grid, dim3(64), VIDC_B2L_LDS_BYTES(128u), st, b, dt);
    else {
        VIDC_TRY(set_big_lds((const void *)k_roc_decode_b2<256>, VIDC_B2L_LDS_BYTES(256u)));
        hipLaunchKernelGGL(k_roc_decode_b2<256>, grid, dim3(64), VIDC_B2L_LDS_BYTES(256u), st, b, dt);
    }
    return VIDC_OK;
}
int dec_launch_lane_reg(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // the register decoder on quads / pairs of lanes
    const LaneDiv *dt = (const LaneDiv *)c.ctx->d_ltab;
    b.lpw = cls == DC_LANEQ ? 16u : 32u;
    const dim3 grid((b.nwork + b.lpw - 1u) / b.lpw);
    if (cls == DC_LANEQ) hipLaunchKernelGGL((k_roc_decode_lane_reg<VIDC_LANE_REG_EL, 4>), grid, dim3(64), 0, st, b, dt);
    else hipLaunchKernelGGL((k_roc_decode_lane_reg<VIDC_LANE_REG_EL, 2>), grid, dim3(64), 0, st, b, dt);
    return VIDC_OK;
}
int dec_launch_grp(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // row-per-list decoder, four lists per wavefront
    const U2Div *dt = (const U2Div *)c.ctx->d_u2tab;
    const dim3 grid((b.nwork + 3u) / 4u);
    if (cls == DC_GRP0) hipLaunchKernelGGL(k_roc_decode_grp<0>, grid, dim3(64), 16u * roc_grp_dec_lds_words(0), st, b, dt);
    else if (cls == DC_GRP2) hipLaunchKernelGGL(k_roc_decode_grp<2>, grid, dim3(64), 16u * roc_grp_dec_lds_words(2), st, b, dt);
    else if (cls == DC_GRP3) hipLaunchKernelGGL(k_roc_decode_grp<3>, grid, dim3(64), 16u * roc_grp_dec_lds_words(3), st, b, dt);
    else hipLaunchKernelGGL(k_roc_decode_grp<4>, grid, dim3(64), 16u * roc_grp_dec_lds_words(4), st, b, dt);
    return VIDC_OK;
}
int dec_launch_ghuge(DecodeCall &c, int cls, RocDecArgs &b, hipStream_t st) {  // 16-bit row counters unless the class holds a list beyond 65 536 ids
    if (c.p.max_n[DC_GHUGE] <= 65536) return dec_launch_gen(c, cls, b, st);
    hipLaunchKernelGGL(k_roc_decode_gen<uint32_t>, dim3(b.nwork), dim3(64), (1u << VIDC_DEC_MAX_FB) * 4, st, b, 1u << VIDC_DEC_MAX_FB, VIDC_DEC_CAP_BIG);
    return VIDC_OK;
}
// (in the order of DecClass)
const DecLaunchFn DEC_LAUNCH[DC_COUNT] = {
    dec_launch_tiny, dec_launch_u, dec_launch_u, dec_launch_gen, dec_launch_gen, dec_launch_gen, dec_launch_gen, dec_launch_ghuge,
    dec_launch_lane, dec_launch_lane_nb, dec_launch_lane_nb, dec_launch_b2, dec_launch_b2l, dec_launch_b2l, dec_launch_b2l, dec_launch_b2l,
    dec_launch_grp, dec_launch_grp, dec_launch_grp, dec_launch_grp, dec_launch_lane_reg, dec_launch_lane_reg};

// the launch of one class on its stream, between the chain events where it is the call's chain class
int dec_launch_class(DecodeCall &c, int cls) {
    vidc_ctx *ctx = c.ctx; const DecPlan &p = c.p;
    if (!p.count[cls]) return VIDC_OK;
    hipStream_t st = c.stream_of[cls];
    if (cls == c.chain_class) {
        ctx->chain_info[1][0] = p.sum_n[cls]; ctx->chain_info[1][1] = p.count[cls]; ctx->chain_info[1][2] = p.max_n[cls];
        ctx->chain_info[1][3] = cls == DC_U20 ? 20 : 18;
        VIDC_HIP(hipEventRecord(ctx->ev_chain[0], st));
    }
    RocDecArgs b = c.a;
    b.worklist = c.d_wl ? c.d_wl + c.base[cls] : nullptr;
    b.nwork = (uint32_t)p.count[cls];
    b.out_off = (c.out_off_host && !p.lean) ? c.s_out_off.as<uint64_t>() + c.base[cls] : nullptr;
    b.scratch_off = c.d_scr_off ? c.d_scr_off + c.base[cls] : nullptr;
    b.slots_off = c.d_slots_off ? c.d_slots_off + c.base[cls] : nullptr;
    b.row_align = p.lane_align;
    VIDC_TRY(DEC_LAUNCH[cls](c, cls, b, st));
    VIDC_HIP(hipGetLastError());
    if (cls == c.chain_class) VIDC_HIP(hipEventRecord(ctx->ev_chain[1], st));
    return VIDC_OK;
}
// every class of the call: longest first, or as VIDC_DEC_SCHED says (its rules: dec_assign_streams)
int dec_run_launches(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx;
    if (c.sched.empty()) {
        for (int k = 0; k < DC_COUNT; k++) VIDC_TRY(dec_launch_class(c, c.order[k]));
        return VIDC_OK;
    }
    std::vector<char> done(DC_COUNT, 0);
    std::stable_sort(c.sched.begin(), c.sched.end(), [](const SchedEntry &x, const SchedEntry &y) { return x.pos < y.pos; });
    VIDC_TRY(run_schedule(c.sched, done, false, [&](const SchedEntry &it) -> int {
        for (int d : it.deps) VIDC_HIP(hipStreamWaitEvent(c.stream_of[it.item], ctx->tev[d], 0));
        VIDC_TRY(dec_launch_class(c, it.item));
        VIDC_HIP(hipEventRecord(ctx->tev[it.item], c.stream_of[it.item]));
        return VIDC_OK;
    }));
    for (int k = 0; k < DC_COUNT; k++)
        if (!done[c.order[k]]) VIDC_TRY(dec_launch_class(c, c.order[k]));
    return VIDC_OK;
}
int dec_join(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx;
    for (int i = 0; i < ctx->naux(); i++) {
        if (!(c.aux_used >> i & 1u)) continue;
        VIDC_HIP(hipEventRecord(ctx->ev_join[i], ctx->aux[i]));
        VIDC_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join[i], 0));
    }
    return VIDC_OK;
}
// the end event of the kernels, then the 32-byte status summary (instead of copying two nlist-sized arrays back) behind them:
// ONE wait for both
int dec_summary_wait(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx; const vidc_roc *r = c.r;
    (void)c.t.mark();
    VIDC_TRY(c.h_sum.get(ctx, (8 + DEC_RETRY_SLOTS) * 8));
    unsigned long long *sum = c.sum = c.h_sum.as<unsigned long long>();
    sum[0] = ~0ull; sum[1] = 0; sum[2] = 0; sum[3] = 0;
    // (the kernel's last workgroup stores the summary into the pinned block itself: no copy up, no copy down)
    hipLaunchKernelGGL(k_roc_status_summary_host, dim3((uint32_t)std::min<uint64_t>((r->nlist + 1023) / 1024, 256)), dim3(256),
                       0, ctx->stream, c.d_status, c.s_end.as<uint32_t>(), (uint32_t)r->nlist,
                       (unsigned long long *)(c.s_end.as<uint32_t>() + 2 * r->nlist), sum, (c.out_off_host || r->rows) ? 0u : DEC_RETRY_SLOTS);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    ctx->last_kernel_ms = c.t.elapsed();
    ctx->phase_ms[VIDC_PHASE_ROC_DECODE] = ctx->last_kernel_ms;
    if (c.chain_class >= 0) {
        float cms = 0;
        if (hipEventElapsedTime(&cms, ctx->ev_chain[0], ctx->ev_chain[1]) == hipSuccess) ctx->phase_ms[VIDC_PHASE_ROC_DECODE_CHAIN] = cms;
    }
    c.tr.mark("decode kernels + status summary (sync)");
    return VIDC_OK;
}
int decode_impl(vidc_ctx *ctx, const vidc_roc *r, const DecPlan &p, const uint64_t *out_off_host, uint64_t *d_out,
                int32_t *d_out_rows, uint32_t K, const struct DecPlanCache *cache = nullptr);
// errors, and the lists the lane-per-list decoders handed back (a full bucket row on skewed ids): these are redone with the
// wave-per-list kernels, into the same output slots
int dec_check_and_retry(DecodeCall &c) {
    vidc_ctx *ctx = c.ctx; const vidc_roc *r = c.r; const DecPlan &p = c.p;
    const unsigned long long *sum = c.sum;
    const uint64_t *out_off_host = c.out_off_host;
    const double first_ms = ctx->last_kernel_ms;
    uint64_t nonclean = sum[1], handed_back = 0;
    if (sum[0] != ~0ull || sum[2]) {
        // (a few handed-back lists and nothing else to report: their numbers came with the summary; otherwise the statuses are fetched)
        const bool listed = sum[0] == ~0ull && !out_off_host && !r->rows && sum[2] <= DEC_RETRY_SLOTS;
        std::vector<uint32_t> status(listed ? 0 : r->nlist);
        if (!listed) VIDC_HIP(hipMemcpy(status.data(), c.d_status, r->nlist * 4, hipMemcpyDeviceToHost));
        if (sum[2]) {
            std::vector<uint32_t> lists2;
            std::vector<uint64_t> off2;
            if (listed) {
                for (uint64_t k = 0; k < sum[2]; k++) lists2.push_back((uint32_t)sum[8 + k]);
                std::sort(lists2.begin(), lists2.end());
                for (uint32_t l : lists2) off2.push_back(r->offsets[l]);
            } else
            for (size_t k = c.base[DC_LANE]; k < p.wl.size(); k++) {  // lane classes, B2, row-per-list classes
                if (status[p.wl[k]] != VIDC_ST_RETRY) continue;
                lists2.push_back(p.wl[k]);
                off2.push_back(out_off_host ? out_off_host[k] : r->offsets[p.wl[k]]);
            }
            if (!listed) for (uint32_t l : lists2) status[l] = VIDC_ST_OK;
            if (c.tr.on) {
                uint64_t mx = 0, mn = ~0ull;
                for (uint32_t l : lists2) { const uint64_t n = r->offsets[l + 1] - r->offsets[l]; mx = std::max(mx, n); mn = std::min(mn, n); }
                fprintf(stderr, "[vidc] roc decode: %zu lists handed back by the lane decoders (%llu .. %llu ids)\n", lists2.size(),
                        (unsigned long long)mn, (unsigned long long)mx);
            }
            if (!listed) VIDC_TRY(check_status(status, "roc decode"));
            PooledDecPlan p2;
            plan_decode(r, lists2, false, p2, ctx->wide, false, false);
            std::vector<uint64_t> out_off2(lists2.size());
            for (size_t k = 0; k < lists2.size(); k++) out_off2[k] = off2[p2.item[k]];
            handed_back = lists2.size();  // (sum[2] counts lists; an item per mention of a list that a request names twice)
            VIDC_TRY(decode_impl(ctx, r, p2, out_off2.data(), c.d_out, nullptr, 0));
            nonclean += r->last_nonclean;
            ctx->last_kernel_ms += first_ms;
            ctx->phase_ms[VIDC_PHASE_ROC_DECODE] = ctx->last_kernel_ms;
        } else {
            VIDC_TRY(check_status(status, "roc decode"));
        }
    }
    r->last_nonclean = nonclean;
    r->last_handed_back = handed_back;  // (behind the nested decode of the handed-back lists, which stored its own 0)
    return VIDC_OK;
}

// The host call of every ROC decode: a plan (plan_decode, a cached one with its device arrays, or a lean / implicit one of graph
// rows) and where the ids go (out_off_host: an output offset per work item; d_out_rows / K: int32 rows instead of u64 ids).
int decode_impl(vidc_ctx *ctx, const vidc_roc *r, const DecPlan &p, const uint64_t *out_off_host, uint64_t *d_out,
                int32_t *d_out_rows, uint32_t K, const struct DecPlanCache *cache) {
    VIDC_HIP(hipSetDevice(ctx->device));
    const size_t nwork = p.implicit ? (size_t)p.implicit : p.wl.size();
    if (nwork == 0) { ctx->last_kernel_ms = 0; r->last_handed_back = 0; return VIDC_OK; }
    DecodeCall c(ctx, r, p, out_off_host, d_out, d_out_rows, K, cache, nwork);
    VIDC_TRY(dec_upload(c));
    (void)c.t.start();
    VIDC_TRY(dec_build_row_order(c));
    VIDC_TRY(dec_assign_streams(c));
    VIDC_TRY(dec_fork(c));
    VIDC_TRY(dec_run_launches(c));
    VIDC_TRY(dec_join(c));
    VIDC_TRY(dec_summary_wait(c));
    return dec_check_and_retry(c);
}

// ---- device-resident label requests (vidc_roc_translate_labels_dev): ROC has no random access, so the touched lists are decoded.
// mark[l] = size of list l and flag[l] = 1 for every list a valid label names (plain stores of the same value: idempotent, no atomics);
// both arrays are cleared by the call.
__global__ void __launch_bounds__(256) k_req_roc_mark(const int64_t *__restrict__ labels, uint64_t n, const uint64_t *__restrict__ offsets,
                                                      uint64_t nlist, uint32_t *__restrict__ mark, uint32_t *__restrict__ flag,
                                                      unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + lane_id();
        uint64_t l = 0, off = 0;
        const bool pos = req_label(i < n ? labels[i] : -1, l, off);
        uint32_t sz = 0;
        if (pos && l < nlist) sz = (uint32_t)(offsets[l + 1] - offsets[l]);
        const bool ok = pos && l < nlist && off < sz;
        if (ok) { mark[l] = sz; flag[l] = 1u; }
        req_count_invalid(pos && !ok, invalid);
    }
}
// touched[tpos[l]] = l for every flagged list: the touched list numbers in ascending order (tpos = exclusive scan of flag)
__global__ void __launch_bounds__(256) k_req_roc_touched(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ tpos, uint64_t nlist,
                                                         uint32_t *__restrict__ touched) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x)
        if (flag[l]) touched[tpos[l]] = (uint32_t)l;
}
// ids[i] = staging[stage_off[list] + offset] (stage_off = exclusive scan of mark: where each touched list was decoded to)
__global__ void __launch_bounds__(256) k_req_roc_pick(const int64_t *labels, uint64_t n, const uint64_t *__restrict__ offsets, uint64_t nlist,
                                                      const uint64_t *__restrict__ stage_off, const uint64_t *__restrict__ staging, int64_t *ids) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t l = 0, off = 0;
        const bool pos = req_label(labels[i], l, off);
        const bool ok = pos && l < nlist && off < offsets[l + 1] - offsets[l];
        ids[i] = ok ? (int64_t)staging[stage_off[l] + off] : -1;
    }
}

// ---- append (vidc_roc_append_dev): only the lists the batch touches are decoded and re-encoded; the rest of the object is spliced.
// flag[l] = the batch adds to list l, mark[l] = ids of its merged list (0 for an untouched list): their exclusive scans are the
// touched list's number among the touched ones (tpos) and its place in the staging CSR (stage_off).
__global__ void __launch_bounds__(256) k_app_roc_mark(const uint64_t *__restrict__ old_off, const uint64_t *__restrict__ add_off, uint64_t nlist,
                                                      uint32_t *__restrict__ mark, uint32_t *__restrict__ flag) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t add = add_off[l + 1] - add_off[l];
        flag[l] = add ? 1u : 0u;
        const uint64_t n = old_off[l + 1] - old_off[l] + add;
        mark[l] = add ? (uint32_t)(n < 0xffffffffull ? n : 0xffffffffull) : 0u;
    }
}
// touched[tpos[l]] = l, added[tpos[l]] = batch entries of l, for every flagged list, ascending
__global__ void __launch_bounds__(256) k_app_roc_touched(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ tpos,
                                                         const uint64_t *__restrict__ add_off, uint64_t nlist, uint32_t *__restrict__ touched,
                                                         uint32_t *__restrict__ added) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x)
        if (flag[l]) {
            touched[tpos[l]] = (uint32_t)l;
            added[tpos[l]] = (uint32_t)(add_off[l + 1] - add_off[l]);
        }
}

// ---- remove (vidc_roc_remove_dev): the candidates are decoded and marked, the lists that lose an entry are re-encoded, the rest is
// spliced.  flag[l] = list l is a candidate -- non-empty and (run_off != NULL) named by a pair of the batch; mark[l] = its ids.
__global__ void __launch_bounds__(256) k_rm_roc_cand(const uint64_t *__restrict__ old_off, const uint64_t *__restrict__ run_off, uint64_t nlist,
                                                     uint32_t *__restrict__ mark, uint32_t *__restrict__ flag) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t n = old_off[l + 1] - old_off[l];
        const bool c = n != 0 && (!run_off || run_off[l + 1] != run_off[l]);
        flag[l] = c ? 1u : 0u;
        mark[l] = c ? (uint32_t)n : 0u;
    }
}
// candidate k (seg_off: where it was decoded to, new_off: the offsets of its survivors) is touched when it lost an entry:
// tflag[k], tmark[k] = its survivor count (0 for an untouched candidate)
__global__ void __launch_bounds__(256) k_rm_roc_kills(const uint64_t *__restrict__ seg_off, const uint64_t *__restrict__ new_off, uint64_t cnt,
                                                      uint32_t *__restrict__ tflag, uint32_t *__restrict__ tmark) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t n = seg_off[k + 1] - seg_off[k], left = new_off[k + 1] - new_off[k];
        tflag[k] = left != n ? 1u : 0u;
        tmark[k] = left != n ? (uint32_t)left : 0u;
    }
}
// t_cand[tpos[k]] = k, t_left[tpos[k]] = survivors, for every touched candidate, ascending; and for the splice lflag[l] = 1,
// ltpos[l] = tpos[k] of its list l = cand[k] (lflag zeroed by the caller)
__global__ void __launch_bounds__(256) k_rm_roc_touched(const uint32_t *__restrict__ tflag, const uint32_t *__restrict__ tmark,
                                                        const uint64_t *__restrict__ tpos, const uint32_t *__restrict__ cand, uint64_t cnt,
                                                        uint32_t *__restrict__ t_cand, uint32_t *__restrict__ t_left, uint32_t *__restrict__ lflag,
                                                        uint64_t *__restrict__ ltpos) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += (uint64_t)gridDim.x * blockDim.x)
        if (tflag[k]) {
            t_cand[tpos[k]] = (uint32_t)k;
            t_left[tpos[k]] = tmark[k];
            lflag[cand[k]] = 1u;
            ltpos[cand[k]] = tpos[k];
        }
}

// ---- the splice (roc_splice, below): list j of the new object is list k of source s, stream and metadata unchanged.  Every
// operation that derives one object from others ends in it -- append, remove, subset, merge, regroup, update_rows.
// A source: its per-list metadata, and where its words and its lists start.  The N sources of an operation (2, 3, or up to
// VIDC_SHARDS_MAX for the regroup) reach the kernels by value; the regroup's host checked src_no[j] < nsrc, the source non-NULL and list_no[j] < its nlist before anything was uploaded.
struct RocSrc {
    const uint64_t *heads;
    const uint32_t *prec, *nwords, *draws;
    const uint32_t *words;
    const uint64_t *word_off, *offsets;
};
template <int N>
struct RocSrcs {
    RocSrc s[N];
};
// Where list j of the new object comes from: get(j, source, list) -> false for a list that has no source (an empty list).
// The regroup's table, uploaded by the host ...
struct RocRegroupTable {
    const uint32_t *src_no;
    const uint64_t *list_no;
    __device__ __forceinline__ bool get(uint64_t j, uint32_t &s, uint64_t &k) const {
        s = src_no[j];
        k = list_no[j];
        return true;
    }
};
// ... and the slot table of vidc_roc_update_rows_dev (rows_update.h), built on the device: source 1 holds the encoded batch rows,
// source 0 is the old object, a new node without a batch row is the empty row.
struct RocUpdateSlots {
    const uint32_t *slot;
    uint64_t N_old;
    __device__ __forceinline__ bool get(uint64_t j, uint32_t &s, uint64_t &k) const {
        const uint32_t sl = slot[j];
        s = sl ? 1u : 0u;
        k = sl ? (uint64_t)(sl - 1u) : j;
        return sl != 0u || j < N_old;
    }
};
// ... and the class table of vidc_roc_merge_dev (merge.h), built on the device: source cls[j] = 0 is `a`, 1 is `b` -- list j of
// either --, 2 is the fresh encode of the lists that hold ids of both sides, list tpos[j] of it.
struct RocMergeSlots {
    const uint32_t *cls;
    const uint64_t *tpos;
    __device__ __forceinline__ bool get(uint64_t j, uint32_t &s, uint64_t &k) const {
        s = cls[j];
        k = s == MRG_ENCODE ? tpos[j] : j;
        return true;
    }
};
// ... and the flags of the append, the remove and the subset, built on the device: source 1 is the small object of the re-encoded
// lists, list ltpos[j] of it where lflag[j] != 0; source 0 is the old object, list j.
struct RocSmallSlots {
    const uint32_t *lflag;
    const uint64_t *ltpos;
    __device__ __forceinline__ bool get(uint64_t j, uint32_t &s, uint64_t &k) const {
        const bool t = lflag[j] != 0u;
        s = t ? 1u : 0u;
        k = t ? ltpos[j] : j;
        return true;
    }
};
// the five per-list arrays of the new object (sizes: what the scan turns into its offsets); *nonempty += lists with ids
template <int N, typename Lookup>
__global__ void __launch_bounds__(256) k_roc_regroup_meta(RocSrcs<N> srcs, Lookup look, uint64_t m, uint64_t *__restrict__ heads, uint32_t *__restrict__ prec,
                                                          uint32_t *__restrict__ nwords, uint32_t *__restrict__ draws, uint32_t *__restrict__ sizes,
                                                          unsigned long long *nonempty) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); j0 < m; j0 += stride) {  // (j0: wavefront-uniform)
        const uint64_t j = j0 + lane_id();
        uint32_t size = 0;
        if (j < m) {
            uint32_t sn;
            uint64_t k;
            if (look.get(j, sn, k)) {
                const RocSrc &s = srcs.s[sn];
                heads[j] = s.heads[k];
                prec[j] = s.prec[k];
                nwords[j] = s.nwords[k];
                draws[j] = s.draws[k];
                size = (uint32_t)(s.offsets[k + 1] - s.offsets[k]);
            } else {  // what the encoders leave for an empty list (k_roc_encode_tiny)
                heads[j] = VIDC_RANS_L;
                prec[j] = 0u;
                nwords[j] = 0u;
                draws[j] = 0u;
            }
            sizes[j] = size;
        }
        const uint64_t b = ballot(size != 0u);
        if (b && lane_id() == 0) atomicAdd(nonempty, (unsigned long long)popc64(b));
    }
}
// the words: a list's stream from the word array of whichever source holds it.  A wavefront per chunk of the new lists' streams
// (items: app_chunks on dst_off; a list without a source has no words, hence no chunk).
template <int N, typename Lookup>
__global__ void __launch_bounds__(256) k_roc_regroup_copy(RocSrcs<N> srcs, Lookup look, const uint64_t *__restrict__ dst_off, uint32_t *__restrict__ dst,
                                                          const Chunk *__restrict__ items, const uint64_t *__restrict__ n_items) {
    const uint64_t total = *n_items;
    const uint32_t lane = lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = dst_off[ch.list], n = dst_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        uint32_t sn;
        uint64_t k;
        if (!look.get(ch.list, sn, k)) continue;
        const RocSrc &s = srcs.s[sn];
        app_copy_chunk(s.words + s.word_off[k] + ch.start, dst + base + ch.start, nc, lane);
    }
}
// sampling permutation of the new object: source perm_src's (sperm, over its lists at soff) for a list taken from it -- the small
// object of freshly encoded lists --, the identity for every other list (a decoded list of distinct ids re-encodes to the identity).
// sperm == NULL: the identity everywhere.  A wavefront per chunk of the new lists (items: app_chunks on new_off).
template <typename Lookup>
__global__ void __launch_bounds__(256) k_roc_regroup_perm(Lookup look, uint32_t perm_src, const uint32_t *__restrict__ sperm,
                                                          const uint64_t *__restrict__ soff, const uint64_t *__restrict__ new_off,
                                                          const Chunk *__restrict__ items, const uint64_t *__restrict__ n_items,
                                                          uint32_t *__restrict__ perm) {
    const uint64_t total = *n_items;
    const uint32_t lane = lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < total; c += (uint64_t)gridDim.x * 4u) {
        const Chunk ch = items[c];
        const uint64_t base = new_off[ch.list], n = new_off[ch.list + 1] - base;
        const uint32_t nc = (uint32_t)(n - ch.start < APP_COPY_UNIT ? n - ch.start : APP_COPY_UNIT);
        uint32_t sn = 0;
        uint64_t k = 0;
        const bool fresh = sperm && look.get(ch.list, sn, k) && sn == perm_src;
        const uint32_t *src = fresh ? sperm + soff[k] + ch.start : nullptr;
        for (uint32_t j = lane; j < nc; j += 64u) perm[base + ch.start + j] = fresh ? src[j] : ch.start + j;
    }
}

// ---- host side of the operations that derive an object from others: what they share
// what: the prefix of the caller's message ("roc merge: ")
bool roc_precision_ok(const char *what, int precision_mode) {
    if (precision_mode >= VIDC_PREC_EXACT && precision_mode <= 32) return true;
    set_error("%sprecision_mode %d unsupported (fixed precision must be 0..32)", what, precision_mode);
    return false;
}
void clear_chain_info(vidc_ctx *ctx) {
    for (int w = 0; w < 2; w++) ctx->chain_info[w][0] = ctx->chain_info[w][1] = ctx->chain_info[w][2] = ctx->chain_info[w][3] = 0;
}
RocSrc roc_src(const vidc_roc *r) {
    return RocSrc{r->d_heads.p, r->d_prec.p, r->d_nwords.p, r->d_draws.p, r->d_words.p, r->d_word_off.p, r->d_offsets.p};
}
// a new object of nlist lists on the context's device; host_offsets: with a host mirror of nlist + 1 offsets (from the process-wide
// vector cache) that the caller fills in
std::unique_ptr<vidc_roc> roc_derived(vidc_ctx *ctx, uint64_t nlist, bool host_offsets = true) {
    std::unique_ptr<vidc_roc> nr(new vidc_roc());
    nr->device = ctx->device;
    nr->nlist = nlist;
    if (host_offsets) {
        nr->offsets = vec_pool<uint64_t>().take(nlist + 1);
        nr->offsets.resize(nlist + 1);
        nr->offsets_host = true;
    }
    return nr;
}

// The lists `lists` of r, decoded into the staging CSR d_stage: lists[i] goes to d_stage + place(i).  (plan_decode orders the work
// items by class: work item k is lists[p.item[k]].)
template <class Place>
int decode_into_staging(vidc_ctx *ctx, const vidc_roc *r, const std::vector<uint32_t> &lists, Place &&place, uint64_t *d_stage, double &kernel_ms) {
    if (lists.empty()) return VIDC_OK;
    PooledDecPlan p;
    plan_decode(r, lists, false, p, ctx->wide);
    std::vector<uint64_t> out_off(lists.size());
    for (size_t k = 0; k < lists.size(); k++) out_off[k] = place(p.item[k]);  // work item k -> its place in the staging
    VIDC_TRY(decode_impl(ctx, r, p, out_off.data(), d_stage, nullptr, 0));
    kernel_ms += ctx->last_kernel_ms;
    return VIDC_OK;
}

// The splice.  List j of nr (device, nlist, rows / K set; offsets / ntotal too where the caller has a host mirror) takes its
// metadata and its words from the list of S that `look` names, or is the encoders' empty list where it names none:
//   the six per-list arrays; k_roc_regroup_meta (sizes, metadata, the non-empty count); one scan launch set for d_offsets and
//   d_word_off; the totals back (24 bytes: words, ids, non-empty lists); the words with their padding; k_roc_regroup_copy;
//   the permutation (want_perm): sperm over the lists of source perm_src where `look` names that source, the identity elsewhere.
// An untouched list costs a copy of its words, not an ANS chain; like an imported object the result carries no planner hints (prec /
// umax / order_desc are empty: the planners mirror the metadata on first use).  The blocks are the caller's, declared in front of
// its StreamGuard; tm was started by the caller and is stopped into kernel_ms; copy_timer (optional) brackets the word copy alone.
// Ends enqueued: the caller waits.
struct RocSpliceScratch {
    Scratch s_sizes, s_cnt, s_scan;
    Pinned h_tot;  // word total | id total | non-empty lists
    AppChunks ch_w, ch_p;
};
template <int N, class Lookup>
int roc_splice(vidc_ctx *ctx, const RocSrcs<N> &S, const Lookup &look, vidc_roc *nr, bool want_perm, uint32_t perm_src, const uint32_t *sperm,
               VidcPhaseTimer *copy_timer, RocSpliceScratch &sc, EventTimer &tm, double &kernel_ms) {
    const uint64_t m = nr->nlist;
    VIDC_TRY(nr->d_offsets.alloc(m + 1, ctx->dpool));
    VIDC_TRY(nr->d_heads.alloc(m, ctx->dpool)); VIDC_TRY(nr->d_prec.alloc(m, ctx->dpool));
    VIDC_TRY(nr->d_nwords.alloc(m, ctx->dpool)); VIDC_TRY(nr->d_draws.alloc(m, ctx->dpool));
    VIDC_TRY(nr->d_word_off.alloc(m + 1, ctx->dpool));
    VIDC_TRY(sc.s_sizes.get(ctx, (m + 1) * 4));
    VIDC_TRY(sc.s_cnt.get(ctx, 8));
    VIDC_TRY(sc.h_tot.get(ctx, 24));
    uint64_t *h_tot = sc.h_tot.as<uint64_t>();
    h_tot[0] = h_tot[1] = h_tot[2] = 0;
    if (m) {
        VIDC_HIP(hipMemsetAsync(sc.s_cnt.p, 0, 8, ctx->stream));
        hipLaunchKernelGGL((k_roc_regroup_meta<N, Lookup>), req_grid(ctx, m), dim3(256), 0, ctx->stream, S, look, m, nr->d_heads.p, nr->d_prec.p,
                           nr->d_nwords.p, nr->d_draws.p, sc.s_sizes.as<uint32_t>(), sc.s_cnt.as<unsigned long long>());
        VIDC_HIP(hipGetLastError());
        Scan4 scan{};
        scan.in[0] = sc.s_sizes.as<uint32_t>(); scan.in[1] = nr->d_nwords.p; scan.out[0] = nr->d_offsets.p; scan.out[1] = nr->d_word_off.p;
        VIDC_TRY(device_exscan4(ctx, scan, 2, (uint32_t)m, sc.s_scan));
        VIDC_HIP(hipMemcpyAsync(h_tot, nr->d_word_off.p + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipMemcpyAsync(h_tot + 1, nr->d_offsets.p + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipMemcpyAsync(h_tot + 2, sc.s_cnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        VIDC_HIP(hipMemsetAsync(nr->d_offsets.p, 0, 8, ctx->stream));
        VIDC_HIP(hipMemsetAsync(nr->d_word_off.p, 0, 8, ctx->stream));
    }
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    nr->total_words = h_tot[0];
    if (!nr->offsets_host) nr->ntotal = h_tot[1];  // (a caller with a host mirror of the offsets has set it)
    nr->compressed_bytes = 8ull * h_tot[2] + 4ull * nr->total_words;
    VIDC_TRY(nr->d_words.alloc(nr->total_words + 16, ctx->dpool));  // + padding: see finish_complete
    if (want_perm) VIDC_TRY(nr->d_perm.alloc(nr->ntotal ? nr->ntotal : 1, ctx->dpool));
    if (nr->total_words) {
        VIDC_TRY(app_chunks(ctx, nr->d_word_off.p, m, nr->total_words, sc.ch_w));
        if (copy_timer) copy_timer->begin();
        hipLaunchKernelGGL((k_roc_regroup_copy<N, Lookup>), app_chunk_grid(ctx, sc.ch_w.bound), dim3(256), 0, ctx->stream, S, look,
                           (const uint64_t *)nr->d_word_off.p, nr->d_words.p, sc.ch_w.items, sc.ch_w.n_items);
        if (copy_timer) copy_timer->end();
        VIDC_HIP(hipGetLastError());
    }
    if (want_perm && nr->ntotal) {
        VIDC_TRY(app_chunks(ctx, nr->d_offsets.p, m, nr->ntotal, sc.ch_p));
        hipLaunchKernelGGL(k_roc_regroup_perm<Lookup>, app_chunk_grid(ctx, sc.ch_p.bound), dim3(256), 0, ctx->stream, look, perm_src, sperm,
                           sperm ? S.s[perm_src].offsets : (const uint64_t *)nullptr, (const uint64_t *)nr->d_offsets.p, sc.ch_p.items,
                           sc.ch_p.n_items, nr->d_perm.p);
        VIDC_HIP(hipGetLastError());
    }
    kernel_ms += tm.stop();
    return VIDC_OK;
}
// the splice over {the old object, the small object of its re-encoded lists (may be NULL: no list is flagged)}: append, remove, subset
int roc_splice(vidc_ctx *ctx, const vidc_roc *r, const vidc_roc *small, const RocSmallSlots &look, vidc_roc *nr, bool want_perm,
                     RocSpliceScratch &sc, EventTimer &tm, double &kernel_ms) {
    RocSrcs<2> S{};
    S.s[0] = roc_src(r);
    if (small) S.s[1] = roc_src(small);
    return roc_splice(ctx, S, look, nr, want_perm, 1u, small ? (const uint32_t *)small->d_perm.p : nullptr, nullptr, sc, tm, kernel_ms);
}

// The candidate pass of the remove and of the subset by id; the locate runs its first half.
// roc_decode_candidates: the candidates -- the non-empty lists of r that run_off names (NULL: every one; `any_work` false: none) -- are
// compacted on the device and their numbers come back once (4 bytes per candidate, metadata); the host sizes a staging CSR (h_seg,
// s_seg) and the candidates are decoded into it (s_stage), in ascending list order.
// roc_candidate_pass: then mark(d_stage, d_seg, d_cand, cnt, total, d_rm, mk) marks the entries that go.  The candidates that lost an
// entry are the touched lists: their staging numbers and survivor counts come back (8 bytes per touched list) and their survivors are
// compacted into s_small_ids, the CSR (T lists, ts_off) that the caller encodes.  Leaves lflag / ltpos for the splice
// (RocSmallSlots), t_list, killed, and in nr its id total and host offsets.
// tm was started by the caller: what it enqueued since counts with the candidate kernels.  The blocks live in front of the caller's
// StreamGuard.
struct RocCandPass {
    Scratch s_mark, s_off, s_cand, s_t0, s_t1, s_stage, s_seg, s_rm, s_tf, s_tp, s_tl, s_lf, s_lt, s_small_ids;
    Pinned h_back, h_seg;
    RemoveMarked mk;
    uint64_t cnt = 0, total = 0;      // candidates, their ids
    std::vector<uint32_t> cand;       // their list numbers, ascending
    uint64_t T = 0, killed = 0;
    std::vector<uint64_t> ts_off{0};  // the small object's offsets
    std::vector<uint32_t> t_list;     // list numbers of the touched lists, ascending
    RocSmallSlots look() const { return RocSmallSlots{s_lf.as<uint32_t>(), s_lt.as<uint64_t>()}; }
};
// the lflag / ltpos of a pass, or of a caller that fills them itself: allocated, no list flagged
int roc_small_slots_clear(vidc_ctx *ctx, uint64_t nlist, RocCandPass &cp) {
    VIDC_TRY(cp.s_lf.get(ctx, (nlist + 1) * 4));
    VIDC_TRY(cp.s_lt.get(ctx, (nlist + 1) * 8));
    VIDC_HIP(hipMemsetAsync(cp.s_lf.p, 0, (nlist + 1) * 4, ctx->stream));
    return VIDC_OK;
}
int roc_decode_candidates(vidc_ctx *ctx, const vidc_roc *r, bool any_work, const uint64_t *run_off, RocCandPass &cp, HostTrace &tr, EventTimer &tm,
                          double &kernel_ms) {
    const uint64_t nlist = r->nlist;
    VIDC_TRY(cp.s_mark.get(ctx, 2 * (nlist + 1) * 4));  // mark | flag
    VIDC_TRY(cp.s_off.get(ctx, 2 * (nlist + 1) * 8));   // stage_off | cpos
    VIDC_TRY(cp.s_cand.get(ctx, (nlist + 1) * 4));
    uint32_t *mark_sz = cp.s_mark.as<uint32_t>(), *flag = mark_sz + nlist + 1;
    uint64_t *stage_off = cp.s_off.as<uint64_t>(), *cpos = stage_off + nlist + 1;
    uint32_t *d_cand = cp.s_cand.as<uint32_t>();
    VIDC_TRY(cp.h_back.get(ctx, 32 + (nlist + 1) * 8));
    uint64_t *h_cnt = cp.h_back.as<uint64_t>();  // candidates | touched lists | survivors
    uint32_t *h_a = (uint32_t *)(h_cnt + 4);
    h_cnt[0] = h_cnt[1] = h_cnt[2] = 0;
    if (nlist && any_work) {
        hipLaunchKernelGGL(k_rm_roc_cand, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, (const uint64_t *)r->d_offsets.p, run_off, nlist, mark_sz,
                           flag);
        Scan4 sc{};
        sc.in[0] = mark_sz; sc.in[1] = flag; sc.out[0] = stage_off; sc.out[1] = cpos;
        VIDC_TRY(device_exscan4(ctx, sc, 2, (uint32_t)nlist, cp.s_t0));
        hipLaunchKernelGGL(k_req_roc_touched, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, flag, cpos, nlist, d_cand);
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(hipMemcpyAsync(h_cnt, cpos + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    kernel_ms += tm.stop();
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    const uint64_t cnt = cp.cnt = h_cnt[0];
    cp.cand.resize(cnt);
    VIDC_TRY(cp.h_seg.get(ctx, (cnt + 1) * 8));
    uint64_t *seg_off = cp.h_seg.as<uint64_t>();
    seg_off[0] = 0;
    if (cnt) {
        VIDC_HIP(hipMemcpyAsync(h_a, d_cand, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
        for (uint64_t k = 0; k < cnt; k++) {
            cp.cand[k] = h_a[k];
            seg_off[k + 1] = seg_off[k] + (r->offsets[h_a[k] + 1] - r->offsets[h_a[k]]);
        }
    }
    cp.total = seg_off[cnt];
    tr.mark("candidates read back");
    if (cnt) {
        VIDC_TRY(cp.s_stage.get(ctx, cp.total * 8));
        VIDC_TRY(cp.s_seg.get(ctx, (cnt + 1) * 8));
        VIDC_HIP(hipMemcpyAsync(cp.s_seg.p, seg_off, (cnt + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        VIDC_TRY(decode_into_staging(ctx, r, cp.cand, [&](uint32_t i) { return seg_off[i]; }, cp.s_stage.as<uint64_t>(), kernel_ms));
        tr.mark("candidates decoded");
    }
    return VIDC_OK;
}
template <class Mark>
int roc_candidate_pass(vidc_ctx *ctx, const vidc_roc *r, bool any_work, const uint64_t *run_off, Mark &&mark, vidc_roc *nr, RocCandPass &cp,
                       HostTrace &tr, EventTimer &tm, double &kernel_ms) {
    const uint64_t nlist = r->nlist;
    VIDC_TRY(roc_decode_candidates(ctx, r, any_work, run_off, cp, tr, tm, kernel_ms));
    VIDC_TRY(roc_small_slots_clear(ctx, nlist, cp));
    if (const uint64_t cnt = cp.cnt) {
        const uint64_t total = cp.total;
        uint64_t *h_cnt = cp.h_back.as<uint64_t>();
        uint32_t *h_a = (uint32_t *)(h_cnt + 4), *h_b = h_a + nlist + 1;
        uint64_t *d_stage = cp.s_stage.as<uint64_t>(), *d_seg = cp.s_seg.as<uint64_t>();
        uint32_t *d_cand = cp.s_cand.as<uint32_t>();
        VIDC_TRY(cp.s_rm.get(ctx, total));
        (void)tm.start();
        VIDC_TRY(mark(d_stage, d_seg, d_cand, cnt, total, cp.s_rm.as<uint8_t>(), cp.mk));
        VIDC_TRY(cp.s_tf.get(ctx, 2 * (cnt + 1) * 4));  // tflag | tmark
        VIDC_TRY(cp.s_tp.get(ctx, 2 * (cnt + 1) * 8));  // tpos | tdst
        VIDC_TRY(cp.s_tl.get(ctx, 2 * (cnt + 1) * 4));  // t_cand | t_left
        uint32_t *tflag = cp.s_tf.as<uint32_t>(), *tmark = tflag + cnt + 1;
        uint64_t *tpos = cp.s_tp.as<uint64_t>(), *tdst = tpos + cnt + 1;
        uint32_t *t_cand = cp.s_tl.as<uint32_t>(), *t_left = t_cand + cnt + 1;
        hipLaunchKernelGGL(k_rm_roc_kills, req_grid(ctx, cnt), dim3(256), 0, ctx->stream, (const uint64_t *)d_seg, (const uint64_t *)cp.mk.new_off, cnt,
                           tflag, tmark);
        Scan4 sc{};
        sc.in[0] = tflag; sc.in[1] = tmark; sc.out[0] = tpos; sc.out[1] = tdst;
        VIDC_TRY(device_exscan4(ctx, sc, 2, (uint32_t)cnt, cp.s_t1));
        hipLaunchKernelGGL(k_rm_roc_touched, req_grid(ctx, cnt), dim3(256), 0, ctx->stream, (const uint32_t *)tflag, (const uint32_t *)tmark,
                           (const uint64_t *)tpos, (const uint32_t *)d_cand, cnt, t_cand, t_left, cp.s_lf.as<uint32_t>(), cp.s_lt.as<uint64_t>());
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(hipMemcpyAsync(h_cnt + 1, tpos + cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipMemcpyAsync(h_cnt + 2, cp.mk.new_off + cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
        kernel_ms += tm.stop();
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
        cp.T = h_cnt[1];
        cp.killed = total - h_cnt[2];
        if (cp.T) {
            VIDC_HIP(hipMemcpyAsync(h_a, t_cand, cp.T * 4, hipMemcpyDeviceToHost, ctx->stream));
            VIDC_HIP(hipMemcpyAsync(h_b, t_left, cp.T * 4, hipMemcpyDeviceToHost, ctx->stream));
            VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
            cp.ts_off.resize(cp.T + 1);
            cp.t_list.resize(cp.T);
            for (uint64_t t = 0; t < cp.T; t++) {
                cp.t_list[t] = cp.cand[h_a[t]];
                cp.ts_off[t + 1] = cp.ts_off[t] + h_b[t];
            }
            const uint64_t ttotal = cp.ts_off[cp.T];
            VIDC_TRY(cp.s_small_ids.get(ctx, (ttotal ? ttotal : 1) * 8));
            (void)tm.start();
            VIDC_TRY(remove_compact(ctx, cp.mk, d_stage, d_seg, cp.s_rm.as<uint8_t>(), tdst, tflag, cp.s_small_ids.as<uint64_t>()));
            kernel_ms += tm.stop();
        }
    }
    tr.mark("candidates marked, touched lists read back");
    // the new object's host offsets: every list moves down by what the touched lists in front of it lost
    nr->ntotal = r->ntotal - cp.killed;
    uint64_t gone = 0, t = 0;
    for (uint64_t l = 0; l < nlist; l++) {
        nr->offsets[l] = r->offsets[l] - gone;
        if (t < cp.T && cp.t_list[t] == l) { gone += (r->offsets[l + 1] - r->offsets[l]) - (cp.ts_off[t + 1] - cp.ts_off[t]); t++; }
    }
    nr->offsets[nlist] = r->offsets[nlist] - gone;
    return VIDC_OK;
}

}  // namespace

extern "C" {

int vidc_roc_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids,
                    int precision_mode, uint32_t flags, vidc_roc **out) {
    if (nlist && offsets && offsets[nlist] > offsets[0] && !d_ids) return VIDC_ERR_INVALID;
    return encode_impl(ctx, nlist, offsets, d_ids, false, 0, 0, nullptr, precision_mode, flags, out);
}

// Device offsets (include/vidc.h): the host planner classifies the lists by length, so the offsets come to the host once (one D2H
// copy into a pinned block, in stream order) and the host path runs on that copy.
int vidc_roc_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids,
                        int precision_mode, uint32_t flags, vidc_roc **out) {
    if (!ctx || !out || !d_offsets) return VIDC_ERR_INVALID;
    *out = nullptr;
    if (nlist >= 0xffffffffull) return VIDC_ERR_INVALID;
    if (ntotal && !d_ids) return VIDC_ERR_INVALID;
    VIDC_HIP(hipSetDevice(ctx->device));
    Pinned h_off;
    VIDC_TRY(h_off.get(ctx, (nlist + 1) * 8));
    uint64_t *h = h_off.as<uint64_t>();
    VIDC_HIP(hipMemcpyAsync(h, d_offsets, (nlist + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    if (h[0] != 0 || h[nlist] != ntotal) {
        set_error("roc: bad device offsets at list %llu (offsets[0] must be 0, offsets[nlist] == ntotal)",
                  (unsigned long long)(h[0] != 0 || !nlist ? 0 : nlist - 1));
        return VIDC_ERR_INVALID;
    }
    return encode_impl(ctx, nlist, h, d_ids, false, 0, 0, nullptr, precision_mode, flags, out);
}

int vidc_roc_encode_rows(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, int precision_mode,
                         uint32_t flags, vidc_roc **out) {
    if (N && !d_rows) return VIDC_ERR_INVALID;
    if (K > TINY_MAX && ctx && out) {
        // wide rows (NSG128, NSG256, ...): the rows become CSR lists and take the per-list kernels; the object answers
        // decode_rows like a graph object (sizes = edge counts, altid_impl.h:61)
        if (N >= 0xffffffffull) { set_error("too many nodes"); return VIDC_ERR_INVALID; }
        VIDC_HIP(hipSetDevice(ctx->device));
        std::vector<uint64_t> offsets;
        Scratch s_ids;
        VIDC_TRY(rows_to_csr(ctx, N, K, d_rows, offsets, s_ids));
        VIDC_TRY(encode_impl(ctx, N, offsets.data(), s_ids.as<uint64_t>(), false, 0, 0, nullptr, precision_mode,
                             flags & ~VIDC_ROC_WANT_PERM, out));
        (*out)->K = K;
        return VIDC_OK;
    }
    return encode_impl(ctx, 0, nullptr, nullptr, true, N, K, d_rows, precision_mode, flags, out);
}

void vidc_roc_destroy(vidc_roc *r) { delete r; }

uint64_t vidc_roc_nlist(const vidc_roc *r) { return r ? r->nlist : 0; }
uint64_t vidc_roc_ntotal(const vidc_roc *r) { return r ? r->ntotal : 0; }
uint64_t vidc_roc_compressed_bytes(const vidc_roc *r) { return r ? r->compressed_bytes : 0; }
uint64_t vidc_roc_total_words(const vidc_roc *r) { return r ? r->total_words : 0; }
uint64_t vidc_roc_last_decode_nonclean(const vidc_roc *r) { return r ? r->last_nonclean : 0; }
uint64_t vidc_roc_last_decode_handed_back(const vidc_roc *r) { return r ? r->last_handed_back : 0; }

int vidc_roc_list_info(const vidc_roc *r, uint32_t *sizes, uint32_t *precisions, uint64_t *heads,
                       uint32_t *nwords, uint32_t *mt_draws) {
    if (!r) return VIDC_ERR_INVALID;
    VIDC_TRY(ensure_meta(r));
    for (uint64_t l = 0; l < r->nlist; l++) {
        if (sizes) sizes[l] = (uint32_t)(r->offsets[l + 1] - r->offsets[l]);
        if (precisions) precisions[l] = r->prec[l];
        if (heads) heads[l] = r->heads[l];
        if (nwords) nwords[l] = r->nwords[l];
        if (mt_draws) mt_draws[l] = r->draws[l];
    }
    return VIDC_OK;
}

int vidc_roc_export_words(vidc_ctx *ctx, const vidc_roc *r, uint64_t list_no, uint32_t *words, size_t cap) {
    if (!ctx || !r || list_no >= r->nlist) return VIDC_ERR_INVALID;
    VIDC_TRY(ensure_meta(r));
    uint64_t nw = r->nwords[list_no];
    if (nw > cap) { set_error("export buffer too small (%zu < %llu words)", cap, (unsigned long long)nw); return VIDC_ERR_INVALID; }
    return vidc_copy_d2h(ctx, words, r->d_words.p + r->word_off[list_no], nw * 4);
}

int vidc_roc_export_all_words(vidc_ctx *ctx, const vidc_roc *r, uint32_t *words, size_t cap) {
    if (!ctx || !r || (r->total_words && !words)) return VIDC_ERR_INVALID;
    if (r->total_words > cap) { set_error("export buffer too small (%zu < %llu words)", cap, (unsigned long long)r->total_words); return VIDC_ERR_INVALID; }
    return vidc_copy_d2h(ctx, words, r->d_words.p, r->total_words * 4);
}

int vidc_roc_perm(vidc_ctx *ctx, const vidc_roc *r, uint32_t *perm_host) {
    if (!ctx || !r || !perm_host) return VIDC_ERR_INVALID;
    if (!r->d_perm.p) { set_error("encode was called without VIDC_ROC_WANT_PERM"); return VIDC_ERR_INVALID; }
    return vidc_copy_d2h(ctx, perm_host, r->d_perm.p, r->ntotal * 4);
}
const uint32_t *vidc_roc_perm_dev(const vidc_roc *r) { return r ? r->d_perm.p : nullptr; }

int vidc_roc_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint32_t *precisions,
                    const uint64_t *heads, const uint32_t *nwords, const uint32_t *mt_draws,
                    const uint32_t *words_concat, vidc_roc **out) {
    if (!ctx || !out) return VIDC_ERR_INVALID;
    *out = nullptr;
    if (nlist && (!offsets || !precisions || !heads || !nwords)) {
        set_error("roc import: offsets, precisions, heads and nwords are required");
        return VIDC_ERR_INVALID;
    }
    if (nlist >= 0xffffffffull) { set_error("too many lists"); return VIDC_ERR_INVALID; }
    // the image is untrusted (.npz content): geometry and per-list state are checked before anything reaches a kernel
    uint64_t tw = 0;
    for (uint64_t l = 0; l < nlist; l++) {
        if (offsets[l + 1] < offsets[l]) { set_error("roc import: offsets not monotone at list %llu", (unsigned long long)l); return VIDC_ERR_INVALID; }
        const uint64_t n = offsets[l + 1] - offsets[l];
        if (mt_draws && mt_draws[l] > VIDC_MT_TABLE) {
            set_error("roc import: list %llu claims %u mt19937 draws (table holds %d)", (unsigned long long)l, mt_draws[l], VIDC_MT_TABLE);
            return VIDC_ERR_INVALID;
        }
        if (n == 0 && nwords[l] != 0) { set_error("roc import: empty list %llu with %u stream words", (unsigned long long)l, nwords[l]); return VIDC_ERR_INVALID; }
        tw += nwords[l];
    }
    if (tw && !words_concat) { set_error("roc import: %llu stream words announced but words == NULL", (unsigned long long)tw); return VIDC_ERR_INVALID; }
    VIDC_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<vidc_roc> r(new vidc_roc());
    r->device = ctx->device;
    r->nlist = nlist;
    if (nlist) r->offsets.assign(offsets, offsets + nlist + 1); else r->offsets.assign(1, 0);
    r->ntotal = nlist ? offsets[nlist] - offsets[0] : 0;
    if (nlist && offsets[0] != 0) { set_error("roc import: offsets[0] must be 0"); return VIDC_ERR_INVALID; }
    r->prec.assign(precisions, precisions + nlist);
    r->heads.assign(heads, heads + nlist);
    r->nwords.assign(nwords, nwords + nlist);
    if (mt_draws) r->draws.assign(mt_draws, mt_draws + nlist); else r->draws.assign(nlist, 0);
    r->word_off.assign(nlist + 1, 0);
    for (uint64_t l = 0; l < nlist; l++) {
        if (r->prec[l] > 32) { set_error("list %llu: precision %u unsupported", (unsigned long long)l, r->prec[l]); return VIDC_ERR_INVALID; }
        uint64_t n = r->offsets[l + 1] - r->offsets[l];
        if (n > VIDC_ROC_MAX_LIST) { set_error("list %llu too long", (unsigned long long)l); return VIDC_ERR_DOMAIN; }
        r->word_off[l + 1] = r->word_off[l] + r->nwords[l];
        if (n) r->compressed_bytes += 8 + 4ull * r->nwords[l];
    }
    r->total_words = r->word_off[nlist];
    VIDC_TRY(upload(ctx, r->d_offsets, r->offsets));
    VIDC_TRY(upload(ctx, r->d_prec, r->prec));
    VIDC_TRY(upload(ctx, r->d_heads, r->heads));
    VIDC_TRY(upload(ctx, r->d_nwords, r->nwords));
    VIDC_TRY(upload(ctx, r->d_draws, r->draws));
    VIDC_TRY(upload(ctx, r->d_word_off, r->word_off));
    VIDC_TRY(r->d_words.alloc(r->total_words + 16, ctx->dpool));  // + padding: the look-ahead of the lane / row decoders reads up to 15 words past the last stream
    if (r->total_words)
        VIDC_HIP(hipMemcpyAsync(r->d_words.p, words_concat, r->total_words * 4, hipMemcpyHostToDevice, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    r->meta_host = true;
    r->offsets_host = true;
    *out = r.release();
    return VIDC_OK;
}

namespace {
std::shared_ptr<DecPlanCache> plan_ahead_build(const vidc_roc *r, bool wide) {
    std::vector<uint32_t> all(r->nlist);
    std::iota(all.begin(), all.end(), 0u);
    auto c = std::make_shared<DecPlanCache>();
    c->wide = wide;
    plan_decode(r, all, false, c->plan, wide, true, true, false, /*whole_sorted=*/true);
    return c;
}
// the arrays of a plan that the kernels read, to the device, on the context's stream
int upload_plan(vidc_ctx *ctx, DecPlanCache &c) {
    VIDC_TRY(upload(ctx, c.d_wl, c.plan.wl));
    VIDC_TRY(upload(ctx, c.d_scratch_off, c.plan.scratch_off));
    VIDC_TRY(upload(ctx, c.d_slots_off, c.plan.slots_off));
    return VIDC_OK;
}
}  // namespace

int vidc_roc_decode_all(vidc_ctx *ctx, const vidc_roc *r, uint64_t *d_out) {
    if (!ctx || !r || (r->ntotal && !d_out)) return VIDC_ERR_INVALID;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    std::shared_ptr<DecPlanCache> plan;
    {
        std::lock_guard<std::mutex> g(r->mu);
        plan = r->plan_all;
    }
    if (plan && plan->wide != ctx->wide) {
        // the cached plan is for the other stream mode (8 against 4 class streams): this call plans for its own context and
        // leaves the cache to the contexts of the mode that built it
        HostTrace tr("roc decode_all (plan of the other stream mode)");
        auto c = plan_ahead_build(r, ctx->wide);
        VIDC_HIP(hipSetDevice(ctx->device));
        VIDC_TRY(upload_plan(ctx, *c));
        const int st = decode_impl(ctx, r, c->plan, nullptr, d_out, nullptr, 0, c.get());
        if (st == VIDC_OK) {
            std::lock_guard<std::mutex> g(r->mu);
            if (r->plan_all == plan && ctx->wide) r->plan_all = c;  // (the wide plan is the better one to keep)
        }
        return st;
    }
    if (!plan) {
        HostTrace tr("roc decode_all");
        std::shared_ptr<DecPlanCache> c;
        {
            std::lock_guard<std::mutex> g(r->mu);
            c = std::move(r->plan_ahead);
        }
        if (c && c->wide != ctx->wide) c.reset();
        if (!c) c = plan_ahead_build(r, ctx->wide);
        tr.mark("plan");
        VIDC_HIP(hipSetDevice(ctx->device));
        VIDC_TRY(upload_plan(ctx, *c));
        tr.mark("plan upload");
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // another context may use the cached plan next
        std::lock_guard<std::mutex> g(r->mu);
        if (!r->plan_all) r->plan_all = c;
        plan = r->plan_all;
    }
    return decode_impl(ctx, r, plan->plan, nullptr, d_out, nullptr, 0, plan.get());
}

int vidc_roc_decode_lists(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *list_nos,
                          uint64_t *d_out, uint64_t *out_offsets) {
    if (!ctx || !r || (m && !list_nos) || !out_offsets) return VIDC_ERR_INVALID;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    std::vector<uint32_t> lists(m);
    std::vector<uint64_t> req_off(m + 1, 0);
    for (uint64_t i = 0; i < m; i++) {
        if (list_nos[i] >= r->nlist) { set_error("list number %llu out of range", (unsigned long long)list_nos[i]); return VIDC_ERR_INVALID; }
        lists[i] = (uint32_t)list_nos[i];
        req_off[i + 1] = req_off[i] + (r->offsets[lists[i] + 1] - r->offsets[lists[i]]);
    }
    std::memcpy(out_offsets, req_off.data(), (m + 1) * 8);
    PooledDecPlan p;
    plan_decode(r, lists, false, p, ctx->wide);
    std::vector<uint64_t> out_off(m);
    for (size_t k = 0; k < m; k++) out_off[k] = req_off[p.item[k]];  // work item k -> its slot in the request
    return decode_impl(ctx, r, p, out_off.data(), d_out, nullptr, 0);
}

int vidc_roc_decode_gather(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                           const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out) {
    if (!ctx || !r) return VIDC_ERR_INVALID;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    return vidc_decode_gather_impl(ctx, r->nlist, m, list_nos, n_items, item_slot, item_off, ids_out,
                                   [&](uint64_t l) { return r->offsets[l + 1] - r->offsets[l]; },
                                   [&](uint64_t *d, uint64_t *lo) { return vidc_roc_decode_lists(ctx, r, m, list_nos, d, lo); });
}

int vidc_roc_decode_rows(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *nodes, uint32_t K,
                         int32_t *d_out, uint32_t *counts) {
    if (!ctx || !r || (m && !d_out)) return VIDC_ERR_INVALID;
    if (K == 0) { set_error("K=0 unsupported"); return VIDC_ERR_UNSUPPORTED; }
    if (!nodes && m > r->nlist) { set_error("nodes == NULL selects nodes 0..m-1: m=%llu > %llu nodes", (unsigned long long)m, (unsigned long long)r->nlist); return VIDC_ERR_INVALID; }
    if (K > TINY_MAX) {  // wide rows: lists of any length through the per-list decoders, -1 padded rows
        VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
        std::vector<uint32_t> lists(m);
        for (uint64_t i = 0; i < m; i++) {
            const uint64_t node = nodes ? nodes[i] : i;
            if (node >= r->nlist) { set_error("node %llu out of range", (unsigned long long)node); return VIDC_ERR_INVALID; }
            lists[i] = (uint32_t)node;
            const uint64_t n = r->offsets[node + 1] - r->offsets[node];
            if (n > K) { set_error("node %u has %llu edges > K=%u", lists[i], (unsigned long long)n, K); return VIDC_ERR_INVALID; }
            if (counts) counts[i] = (uint32_t)n;
        }
        if (!m) return VIDC_OK;
        VIDC_HIP(hipSetDevice(ctx->device));
        VIDC_HIP(hipMemsetAsync(d_out, 0xff, m * (uint64_t)K * 4, ctx->stream));
        PooledDecPlan p;
        plan_decode(r, lists, false, p, ctx->wide, false, false, true);  // only the kernels that write int32 rows
        std::vector<uint64_t> out_off(m);
        for (size_t k = 0; k < m; k++) out_off[k] = (uint64_t)p.item[k] * K;
        return decode_impl(ctx, r, p, out_off.data(), nullptr, d_out, K);
    }
    const bool lean = r->rows && K >= r->K && !force_general() && lane_wanted(lane_policy(), m, LANE_MIN_TINY);
    if (lean && !nodes) {  // rows 0..m-1 of a graph object: nothing proportional to m is built on or leaves the host
        PooledDecPlan p;
        p.lean = true; p.tiny_lane = true; p.implicit = m;
        p.count[DC_TINY] = m;
        std::unique_lock<std::mutex> g(r->mu, std::defer_lock);
        if (m == r->nlist && m >= 65536) {  // the whole graph: rows of equal edge count share a wavefront (k_rows_order_*)
            g.lock();
            if (!r->row_order_ready) {
                // the first whole-graph decode of the object builds the order inside its own timed region (decode_impl) and publishes
                // it -- other contexts may use it -- once this call has synchronised; until then the object's lock stays with this call
                // (the per-workgroup histograms live behind the order in the object's own buffer: no scratch to hand back)
                VIDC_TRY(r->d_row_order.alloc(m + (uint64_t)VIDC_ORDER_BLOCKS * 65, ctx->dpool));
                p.order_build = true;
            } else {
                g.unlock();
            }
            p.order_dev = r->d_row_order.p;
        }
        VIDC_TRY(decode_impl(ctx, r, p, nullptr, nullptr, d_out, K));  // (ends with a synchronisation of the stream)
        if (p.order_build) { r->row_order_ready = true; g.unlock(); }
        if (counts) VIDC_TRY(fetch_sizes<uint32_t>(ctx, r->d_offsets.p, (const uint32_t *)nullptr, m, counts));
        return VIDC_OK;
    }
    if (!lean) VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    std::vector<uint32_t> lists(m);
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t node = nodes ? nodes[i] : i;
        if (node >= r->nlist) { set_error("node %llu out of range", (unsigned long long)node); return VIDC_ERR_INVALID; }
        lists[i] = (uint32_t)node;
        if (!lean) {
            uint64_t n = r->offsets[lists[i] + 1] - r->offsets[lists[i]];
            if (n > K) { set_error("node %u has %llu edges > K=%u", lists[i], (unsigned long long)n, K); return VIDC_ERR_INVALID; }
            if (counts) counts[i] = (uint32_t)n;
        }
    }
    PooledDecPlan p;
    plan_decode(r, lists, true, p, ctx->wide, lean);
    if (p.lean) {
        VIDC_TRY(decode_impl(ctx, r, p, nullptr, nullptr, d_out, K));
        if (counts && m) {  // edge counts of the requested nodes, gathered on the device
            Scratch s_wl;
            Pinned h_wl;
            VIDC_TRY(s_wl.get(ctx, m * 4));
            VIDC_TRY(h_wl.get(ctx, m * 4));
            std::memcpy(h_wl.p, lists.data(), m * 4);
            VIDC_HIP(hipMemcpyAsync(s_wl.p, h_wl.p, m * 4, hipMemcpyHostToDevice, ctx->stream));
            VIDC_TRY(fetch_sizes<uint32_t>(ctx, r->d_offsets.p, s_wl.as<uint32_t>(), m, counts));
        }
        return VIDC_OK;
    }
    std::vector<uint64_t> out_off(m);
    for (size_t k = 0; k < m; k++) out_off[k] = (uint64_t)p.item[k] * K;
    return decode_impl(ctx, r, p, out_off.data(), nullptr, d_out, K);
}

int vidc_roc_translate_labels_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                  uint64_t *d_invalid) {
    VIDC_TRY(req_check_labels(ctx, r, n, d_labels, d_ids));
    if (!n) return VIDC_OK;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    VIDC_HIP(hipSetDevice(ctx->device));
    const uint64_t nlist = r->nlist;
    Scratch s_mark, s_off, s_touched, s_t0, s_stage;
    Pinned h_back;
    VIDC_TRY(s_mark.get(ctx, 2 * (nlist + 1) * 4));   // mark | flag
    VIDC_TRY(s_off.get(ctx, 2 * (nlist + 1) * 8));    // stage_off | tpos
    VIDC_TRY(s_touched.get(ctx, (nlist + 1) * 4));
    uint32_t *mark = s_mark.as<uint32_t>(), *flag = mark + nlist + 1;
    uint64_t *stage_off = s_off.as<uint64_t>(), *tpos = stage_off + nlist + 1;
    VIDC_HIP(hipMemsetAsync(s_mark.p, 0, 2 * (nlist + 1) * 4, ctx->stream));  // (cached blocks hold stale marks, or poison)
    hipLaunchKernelGGL(k_req_roc_mark, req_grid(ctx, n), dim3(256), 0, ctx->stream, d_labels, n, r->d_offsets.p, nlist, mark, flag,
                       (unsigned long long *)d_invalid);
    VIDC_HIP(hipGetLastError());
    if (nlist) {
        Scan4 sc{};
        sc.in[0] = mark; sc.in[1] = flag; sc.out[0] = stage_off; sc.out[1] = tpos;
        VIDC_TRY(device_exscan4(ctx, sc, 2, (uint32_t)nlist, s_t0));
        hipLaunchKernelGGL(k_req_roc_touched, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, flag, tpos, nlist, s_touched.as<uint32_t>());
        VIDC_HIP(hipGetLastError());
    }
    // the touched list numbers come back once (count, then the numbers: 4 bytes per touched list, metadata)
    VIDC_TRY(h_back.get(ctx, 8 + (nlist + 1) * 4));
    uint64_t *h_cnt = h_back.as<uint64_t>();
    uint32_t *h_touched = (uint32_t *)(h_cnt + 1);
    *h_cnt = 0;
    if (nlist) VIDC_HIP(hipMemcpyAsync(h_cnt, tpos + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    const uint64_t cnt = *h_cnt;
    std::vector<uint32_t> lists(cnt);
    uint64_t total = 0;
    std::vector<uint64_t> req_off(cnt + 1, 0);
    if (cnt) {
        VIDC_HIP(hipMemcpyAsync(h_touched, s_touched.p, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
        for (uint64_t k = 0; k < cnt; k++) {  // (the same offsets k_req_roc_mark + the scan put into stage_off)
            lists[k] = h_touched[k];
            req_off[k + 1] = req_off[k] + (r->offsets[lists[k] + 1] - r->offsets[lists[k]]);
        }
        total = req_off[cnt];
    }
    VIDC_TRY(s_stage.get(ctx, (total ? total : 1) * 8));
    if (cnt) {
        PooledDecPlan p;
        plan_decode(r, lists, false, p, ctx->wide);
        std::vector<uint64_t> out_off(cnt);
        for (size_t k = 0; k < cnt; k++) out_off[k] = req_off[p.item[k]];  // work item k -> its place in the staging
        VIDC_TRY(decode_impl(ctx, r, p, out_off.data(), s_stage.as<uint64_t>(), nullptr, 0));
    }
    hipLaunchKernelGGL(k_req_roc_pick, req_grid(ctx, n), dim3(256), 0, ctx->stream, d_labels, n, r->d_offsets.p, nlist, stage_off,
                       s_stage.as<uint64_t>(), d_ids);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    return VIDC_OK;
}

// Append (include/vidc.h).  The batch is sorted by list on the device (append.h); the touched lists are marked and compacted there, and
// their numbers and add counts come back once (8 bytes per touched list, metadata).  The host sizes a staging CSR of the merged touched
// lists, the old ids are decoded into it, the batch ids are placed behind them, and encode_impl runs on the staging CSR alone: the
// small object of the touched lists, which the splice joins with the old one (flag / tpos are its RocSmallSlots).
int vidc_roc_append_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids, int precision_mode,
                        uint32_t flags, vidc_roc **out, int64_t *d_labels, uint64_t *d_invalid) {
    VIDC_TRY(append_check(ctx, r, out, n_add, d_list_nos, d_ids));
    if (r->rows) { set_error("roc append: graph objects are not appendable"); return VIDC_ERR_UNSUPPORTED; }
    if (!roc_precision_ok("", precision_mode)) return VIDC_ERR_INVALID;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc append");
    const uint64_t nlist = r->nlist;
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0;
    clear_chain_info(ctx);
    double kernel_ms = 0;
    AppendBatch b;
    std::unique_ptr<vidc_roc> small, nr;
    Scratch s_mark, s_off, s_touched, s_t0, s_stage;
    Pinned h_back;
    AppChunks ch_l;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    VIDC_TRY(append_sort_batch(ctx, nlist, r->d_offsets.p, n_add, d_list_nos, d_invalid, b));
    tr.mark("batch sorted by list");
    // the touched lists
    VIDC_TRY(s_mark.get(ctx, 2 * (nlist + 1) * 4));   // mark | flag
    VIDC_TRY(s_off.get(ctx, 2 * (nlist + 1) * 8));    // stage_off | tpos
    VIDC_TRY(s_touched.get(ctx, 2 * (nlist + 1) * 4));  // touched | added
    uint32_t *mark = s_mark.as<uint32_t>(), *flag = mark + nlist + 1;
    uint64_t *stage_off = s_off.as<uint64_t>(), *tpos = stage_off + nlist + 1;
    VIDC_TRY(h_back.get(ctx, 8 + (nlist + 1) * 8));
    uint64_t *h_cnt = h_back.as<uint64_t>();
    uint32_t *h_touched = (uint32_t *)(h_cnt + 1), *h_added = h_touched + nlist + 1;
    uint32_t *d_touched = s_touched.as<uint32_t>(), *d_added = d_touched + nlist + 1;
    h_cnt[0] = 0;
    if (nlist) {
        hipLaunchKernelGGL(k_app_roc_mark, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, r->d_offsets.p, (const uint64_t *)b.add_off, nlist, mark, flag);
        Scan4 sc{};
        sc.in[0] = mark; sc.in[1] = flag; sc.out[0] = stage_off; sc.out[1] = tpos;
        VIDC_TRY(device_exscan4(ctx, sc, 2, (uint32_t)nlist, s_t0));
        hipLaunchKernelGGL(k_app_roc_touched, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, flag, tpos, (const uint64_t *)b.add_off, nlist,
                           d_touched, d_added);
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(hipMemcpyAsync(h_cnt, tpos + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    const uint64_t cnt = h_cnt[0];
    if (cnt) {
        VIDC_HIP(hipMemcpyAsync(h_touched, d_touched, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipMemcpyAsync(h_added, d_added, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    }
    // staging CSR of the merged touched lists; host offsets of the new object
    std::vector<uint64_t> st_off(cnt + 1, 0);
    std::vector<uint32_t> dec_lists, dec_slot;  // touched lists that hold old ids, and their number among the touched ones
    for (uint64_t k = 0; k < cnt; k++) {
        const uint64_t l = h_touched[k], old_n = r->offsets[l + 1] - r->offsets[l], n = old_n + h_added[k];
        if (n > VIDC_ROC_MAX_LIST) {
            set_error("roc append: list %llu would hold %llu ids (limit %u)", (unsigned long long)l, (unsigned long long)n, VIDC_ROC_MAX_LIST);
            return VIDC_ERR_DOMAIN;
        }
        st_off[k + 1] = st_off[k] + n;
        if (old_n) { dec_lists.push_back((uint32_t)l); dec_slot.push_back((uint32_t)k); }
    }
    const uint64_t total = st_off[cnt];
    nr = roc_derived(ctx, nlist);
    nr->ntotal = r->ntotal + b.n_valid;
    {
        uint64_t shift = 0, k = 0;
        for (uint64_t l = 0; l < nlist; l++) {
            nr->offsets[l] = r->offsets[l] + shift;
            if (k < cnt && h_touched[k] == l) shift += h_added[k++];
        }
        nr->offsets[nlist] = r->offsets[nlist] + shift;
    }
    tr.mark("touched lists read back, staging sized");
    VIDC_TRY(s_stage.get(ctx, (total ? total : 1) * 8));
    VIDC_TRY(decode_into_staging(ctx, r, dec_lists, [&](uint32_t i) { return st_off[dec_slot[i]]; }, s_stage.as<uint64_t>(), kernel_ms));
    tr.mark("touched lists decoded");
    if (n_add) {
        hipLaunchKernelGGL(k_app_place, req_grid(ctx, n_add), dim3(256), 0, ctx->stream, b.keys, b.vals, (uint32_t)n_add, nlist, r->d_offsets.p,
                           (const uint64_t *)b.add_off, (const uint64_t *)stage_off, d_ids, s_stage.as<uint64_t>(), d_labels, false);
        VIDC_HIP(hipGetLastError());
    }
    if (cnt) {
        vidc_roc *sp = nullptr;
        VIDC_TRY(encode_impl(ctx, cnt, st_off.data(), s_stage.as<uint64_t>(), false, 0, 0, nullptr, precision_mode,
                             want_perm || d_labels ? VIDC_ROC_WANT_PERM : 0u, &sp));
        small.reset(sp);
        kernel_ms += ctx->last_kernel_ms;
    }
    tr.mark("touched lists encoded");
    EventTimer tm = EventTimer::started(ctx);
    if (d_labels && small) {  // a batch entry's offset: where the small object's permutation names it (sampling order)
        VIDC_TRY(app_chunks(ctx, small->d_offsets.p, cnt, total, ch_l));
        hipLaunchKernelGGL(k_app_labels_perm, app_chunk_grid(ctx, ch_l.bound), dim3(256), 0, ctx->stream, (const uint32_t *)small->d_perm.p,
                           (const uint64_t *)small->d_offsets.p, (const uint32_t *)d_touched, (const uint64_t *)r->d_offsets.p,
                           (const uint64_t *)b.add_off, b.vals, ch_l.items, ch_l.n_items, d_labels);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(roc_splice(ctx, r, small.get(), RocSmallSlots{flag, tpos}, nr.get(), want_perm, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    tr.mark("spliced");
    *out = nr.release();
    return VIDC_OK;
}

// Merge (include/vidc.h).  The lists are classified on the device (merge.h): a list without ids of `b` keeps a's stream, a list
// without ids of `a` keeps b's when nothing is shifted, every other list is re-encoded.  The numbers and merged sizes of the
// re-encoded lists come back once (8 bytes each, metadata); the host sizes a staging CSR of them, a's ids are decoded into it, b's
// into a staging of their own and from there behind a's with add_id added (k_mrg_copy_add, which also reduces the largest id for the
// domain check), and encode_impl runs on the staging CSR alone.  The splice is over {a, b, the small object} through the class table
// (RocMergeSlots).
int vidc_roc_merge_dev(vidc_ctx *ctx, const vidc_roc *a, const vidc_roc *b, uint64_t add_id, int precision_mode, uint32_t flags, vidc_roc **out,
                       int64_t *d_src) {
    VIDC_TRY(merge_check(ctx, a, b, out));
    if (!roc_precision_ok("roc merge: ", precision_mode)) return VIDC_ERR_INVALID;
    if (a->rows || b->rows) { set_error("roc merge: graph objects hold no lists to merge"); return VIDC_ERR_UNSUPPORTED; }
    VIDC_TRY(a->prec.size() == a->nlist ? ensure_offsets(a) : ensure_meta(a));
    if (b != a) VIDC_TRY(b->prec.size() == b->nlist ? ensure_offsets(b) : ensure_meta(b));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc merge");
    const uint64_t nlist = a->nlist;
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0, need_perm = want_perm || d_src;
    clear_chain_info(ctx);
    double kernel_ms = 0;
    std::unique_ptr<vidc_roc> small, nr;
    Scratch s_cls, s_off, s_touched, s_t0, s_stage, s_bstage, s_max;
    Pinned h_back;
    AppChunks ch_b;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    VIDC_TRY(s_cls.get(ctx, 5 * (nlist + 1) * 4));      // cls | flag | mark | bmark | slot
    VIDC_TRY(s_off.get(ctx, 4 * (nlist + 1) * 8));      // stage_off | tpos | bstage_off | dst_start
    VIDC_TRY(s_touched.get(ctx, 2 * (nlist + 1) * 4));  // touched | msize
    VIDC_TRY(s_max.get(ctx, 8));                        // largest id of b's re-encoded lists
    VIDC_TRY(h_back.get(ctx, 16 + (nlist + 1) * 8));
    uint32_t *cls = s_cls.as<uint32_t>(), *flag = cls + nlist + 1, *mark = flag + nlist + 1, *bmark = mark + nlist + 1, *slot = bmark + nlist + 1;
    uint64_t *stage_off = s_off.as<uint64_t>(), *tpos = stage_off + nlist + 1, *bstage_off = tpos + nlist + 1, *dst_start = bstage_off + nlist + 1;
    uint32_t *d_touched = s_touched.as<uint32_t>(), *d_msize = d_touched + nlist + 1;
    uint64_t *h_cnt = h_back.as<uint64_t>();  // re-encoded lists | largest id
    uint32_t *h_touched = (uint32_t *)(h_cnt + 2), *h_msize = h_touched + nlist + 1;
    h_cnt[0] = h_cnt[1] = 0;
    const uint64_t *a_off = a->d_offsets.p, *b_off = b->d_offsets.p;
    EventTimer tm = EventTimer::started(ctx);
    if (nlist) {
        hipLaunchKernelGGL(k_mrg_roc_classify, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, a_off, b_off, nlist, add_id != 0, cls, flag, mark, bmark);
        Scan4 sc{};
        sc.in[0] = mark; sc.in[1] = flag; sc.in[2] = bmark; sc.out[0] = stage_off; sc.out[1] = tpos; sc.out[2] = bstage_off;
        VIDC_TRY(device_exscan4(ctx, sc, 3, (uint32_t)nlist, s_t0));
        hipLaunchKernelGGL(k_mrg_roc_touched, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, (const uint32_t *)flag, (const uint64_t *)tpos,
                           (const uint32_t *)mark, (const uint64_t *)stage_off, a_off, nlist, d_touched, d_msize, slot, dst_start);
        VIDC_HIP(hipGetLastError());
        (void)tm.mark();
        VIDC_HIP(hipMemcpyAsync(h_cnt, tpos + nlist, 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        (void)tm.mark();
    }
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    kernel_ms += tm.elapsed();
    const uint64_t cnt = h_cnt[0];
    if (cnt) {
        VIDC_HIP(hipMemcpyAsync(h_touched, d_touched, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(hipMemcpyAsync(h_msize, d_msize, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    }
    // staging CSRs of the re-encoded lists: the merged lists, and b's decoded part of them
    std::vector<uint64_t> st_off(cnt + 1, 0), bst_off(cnt + 1, 0);
    std::vector<uint32_t> dec_a, dec_a_slot, dec_b;  // re-encoded lists that hold ids of a (and their number among the re-encoded); of b: all
    for (uint64_t k = 0; k < cnt; k++) {
        const uint64_t l = h_touched[k], a_n = a->offsets[l + 1] - a->offsets[l], b_n = b->offsets[l + 1] - b->offsets[l], n = h_msize[k];
        if (n != a_n + b_n) { set_error("roc merge: list %llu: the device and the host disagree about its size", (unsigned long long)l); return VIDC_ERR_INVALID; }
        if (n > VIDC_ROC_MAX_LIST) {
            set_error("roc merge: list %llu would hold %llu ids (limit %u)", (unsigned long long)l, (unsigned long long)n, VIDC_ROC_MAX_LIST);
            return VIDC_ERR_DOMAIN;
        }
        st_off[k + 1] = st_off[k] + n;
        bst_off[k + 1] = bst_off[k] + b_n;
        if (a_n) { dec_a.push_back((uint32_t)l); dec_a_slot.push_back((uint32_t)k); }
        dec_b.push_back((uint32_t)l);
    }
    const uint64_t total = st_off[cnt], btotal = bst_off[cnt];
    tr.mark("lists classified, re-encoded lists read back");
    if (cnt) {
        VIDC_TRY(s_stage.get(ctx, total * 8));
        VIDC_TRY(s_bstage.get(ctx, btotal * 8));
        VIDC_TRY(decode_into_staging(ctx, a, dec_a, [&](uint32_t i) { return st_off[dec_a_slot[i]]; }, s_stage.as<uint64_t>(), kernel_ms));
        VIDC_TRY(decode_into_staging(ctx, b, dec_b, [&](uint32_t i) { return bst_off[i]; }, s_bstage.as<uint64_t>(), kernel_ms));
        tr.mark("re-encoded lists decoded on both sides");
        (void)tm.start();
        VIDC_HIP(hipMemsetAsync(s_max.p, 0, 8, ctx->stream));
        VIDC_TRY(app_chunks(ctx, bstage_off, nlist, btotal, ch_b));
        hipLaunchKernelGGL(k_mrg_copy_add, app_chunk_grid(ctx, ch_b.bound), dim3(256), 0, ctx->stream, (const uint64_t *)s_bstage.as<uint64_t>(),
                           (const uint64_t *)bstage_off, (const uint64_t *)dst_start, s_stage.as<uint64_t>(), add_id, ch_b.items, ch_b.n_items,
                           s_max.as<unsigned long long>());
        VIDC_HIP(hipGetLastError());
        (void)tm.mark();
        VIDC_HIP(hipMemcpyAsync(h_cnt + 1, s_max.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
        kernel_ms += tm.elapsed();
        if (merge_shift_overflows(h_cnt[1], add_id, 31u)) {
            set_error("roc merge: id %llu + add_id %llu is outside [0, 2^31)", (unsigned long long)h_cnt[1], (unsigned long long)add_id);
            return VIDC_ERR_DOMAIN;
        }
        vidc_roc *sp = nullptr;
        VIDC_TRY(encode_impl(ctx, cnt, st_off.data(), s_stage.as<uint64_t>(), false, 0, 0, nullptr, precision_mode,
                             need_perm ? VIDC_ROC_WANT_PERM : 0u, &sp));
        small.reset(sp);
        kernel_ms += ctx->last_kernel_ms;
        tr.mark("re-encoded lists encoded");
    }
    // splice
    nr = roc_derived(ctx, nlist);
    nr->ntotal = a->ntotal + b->ntotal;
    for (uint64_t l = 0; l <= nlist; l++) nr->offsets[l] = a->offsets[l] + b->offsets[l];
    RocSrcs<3> S{};
    S.s[MRG_KEEP_A] = roc_src(a);
    S.s[MRG_KEEP_B] = roc_src(b);
    if (small) S.s[MRG_ENCODE] = roc_src(small.get());
    (void)tm.start();
    VIDC_TRY(roc_splice(ctx, S, RocMergeSlots{cls, tpos}, nr.get(), want_perm, MRG_ENCODE, small ? (const uint32_t *)small->d_perm.p : nullptr,
                        nullptr, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    // where every entry came from: the small object's permutation names the input position of a re-encoded list's entries, the kept
    // lists decode in their source's order
    VIDC_TRY(merge_write_src(ctx, nlist, nr->ntotal, a_off, b_off, nr->d_offsets.p, small ? (const uint32_t *)small->d_perm.p : nullptr,
                             small ? (const uint64_t *)small->d_offsets.p : nullptr, slot, d_src, kernel_ms));
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    tr.mark("spliced");
    *out = nr.release();
    return VIDC_OK;
}

// Remove (include/vidc.h).  The batch is sorted by (list, id) on the device (remove.h); the candidates are the non-empty lists a
// valid pair names, or every non-empty list in any-list mode (roc_candidate_pass with the batch's mark); encode_impl runs on the
// compacted survivors of the touched lists alone, and the splice joins that small object with the old one.
// (the body is vidc::roc_remove, which the sharded remove calls with the per-pair found bytes; common.h)
extern "C++" {
namespace vidc {
int roc_remove(vidc_ctx *ctx, const vidc_roc *r, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids, int precision_mode, uint32_t flags,
               vidc_roc **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid, uint8_t *d_pair_found) {
    VIDC_TRY(remove_check(ctx, r, out, n_rm, d_ids));
    if (!roc_precision_ok("roc remove: ", precision_mode)) return VIDC_ERR_INVALID;
    if (r->rows) { set_error("roc remove: graph objects hold no removable lists"); return VIDC_ERR_UNSUPPORTED; }
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc remove");
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0;
    clear_chain_info(ctx);
    double kernel_ms = 0;
    RemoveBatch b;
    std::unique_ptr<vidc_roc> small, nr = roc_derived(ctx, r->nlist);
    RocCandPass cp;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    EventTimer tm = EventTimer::started(ctx);
    VIDC_TRY(remove_sort_batch(ctx, r->nlist, n_rm, d_list_nos, d_ids, 32u, d_missing, d_invalid, b));
    if (d_removed && r->ntotal) VIDC_HIP(hipMemsetAsync(d_removed, 0, r->ntotal, ctx->stream));
    // (an empty batch has no candidate, in either mode)
    VIDC_TRY(roc_candidate_pass(ctx, r, n_rm != 0, b.any ? (const uint64_t *)nullptr : b.run_off,
                                [&](auto *d_stage, auto *d_seg, auto *d_cand, uint64_t cnt, uint64_t total, uint8_t *d_rm, RemoveMarked &mk) {
                                    return remove_mark(ctx, b, d_stage, d_seg, d_cand, cnt, total, d_rm, d_removed, (const uint64_t *)r->d_offsets.p,
                                                       d_missing, mk);
                                },
                                nr.get(), cp, tr, tm, kernel_ms));
    (void)tm.start();
    VIDC_TRY(remove_count_missing(ctx, b, d_missing));
    VIDC_TRY(remove_pair_found(ctx, b, d_pair_found));
    kernel_ms += tm.stop();
    if (cp.T) {
        vidc_roc *sp = nullptr;
        VIDC_TRY(encode_impl(ctx, cp.T, cp.ts_off.data(), cp.s_small_ids.as<uint64_t>(), false, 0, 0, nullptr, precision_mode,
                             want_perm ? VIDC_ROC_WANT_PERM : 0u, &sp));
        small.reset(sp);
        kernel_ms += ctx->last_kernel_ms;
    }
    tr.mark("touched lists encoded");
    (void)tm.start();
    VIDC_TRY(roc_splice(ctx, r, small.get(), cp.look(), nr.get(), want_perm, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    tr.mark("spliced");
    *out = nr.release();
    return VIDC_OK;
}

// ---- subset (vidc_roc_subset_dev).  lflag / ltpos of the splice from the classes of k_sub_bounds: a partial list takes list ppos[l]
// of the small object (ppos = exclusive scan of pflag), a list that keeps nothing takes the small object's trailing empty list
// (number ppos[nlist], the count of partial lists), a kept list stays with the source.
namespace {
__global__ void __launch_bounds__(256) k_sub_roc_slots(const uint32_t *__restrict__ cls, const uint64_t *__restrict__ ppos, uint64_t nlist,
                                                       uint32_t *__restrict__ lflag, uint64_t *__restrict__ ltpos) {
    const uint64_t np = ppos[nlist];
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < nlist; l += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cls[l];
        lflag[l] = c != SUBC_KEEP ? 1u : 0u;
        ltpos[l] = c == SUBC_PARTIAL ? ppos[l] : np;
    }
}
}  // namespace

// Subset (include/vidc.h).  Types 0 and 1 are a remove in any-list mode with the predicate mark of subset.h in place of the batch
// (roc_candidate_pass over every non-empty list).  Types 2 .. 4 need no id: k_sub_bounds classifies every list from the offsets, the
// host runs the same functions (subset_plan.h) on its mirror of the offsets and so knows the partial lists and every new size without
// a read-back; only the partial lists are decoded, sliced in staging and encoded.  The lists that keep nothing take the encoder's own
// empty list, one trailing list of the small object.
static int roc_subset(vidc_ctx *ctx, const vidc_roc *r, int type, uint64_t a1, uint64_t a2, int precision_mode, uint32_t flags, vidc_roc **out,
                      uint8_t *d_taken, uint64_t *n_taken) {
    VIDC_TRY(subset_check("roc", ctx, r, out, type, a1, a2));
    if (!roc_precision_ok("roc subset: ", precision_mode)) return VIDC_ERR_INVALID;
    if (r->rows) { set_error("roc subset: graph objects hold no lists to take a subset of"); return VIDC_ERR_UNSUPPORTED; }
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc subset");
    const uint64_t nlist = r->nlist, ntotal_old = r->ntotal;
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0;
    clear_chain_info(ctx);
    double kernel_ms = 0;
    std::unique_ptr<vidc_roc> small, nr = roc_derived(ctx, nlist);  // (the host offsets are filled in by either path)
    AppChunks ch_s, ch_t;
    RocCandPass cp;  // (the positional types leave ts_off, lflag / ltpos and s_small_ids in it as the pass does)
    Scratch s_lo, s_dst, s_off, s_cand, s_t0, s_stage, s_seg;
    Pinned h_seg, h_dst;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    EventTimer tm = EventTimer::started(ctx);
    uint64_t nsmall = 0;
    std::vector<uint64_t> &ts_off = cp.ts_off;
    if (subset_by_id(type)) {
        VIDC_TRY(roc_candidate_pass(ctx, r, ntotal_old != 0, nullptr,
                                    [&](auto *d_stage, auto *d_seg, auto *d_cand, uint64_t cnt, uint64_t total, uint8_t *d_rm, RemoveMarked &mk) {
                                        return subset_mark(ctx, type, a1, a2, d_stage, d_seg, d_cand, cnt, total, d_rm, d_taken,
                                                           (const uint64_t *)r->d_offsets.p, mk);
                                    },
                                    nr.get(), cp, tr, tm, kernel_ms));
        nsmall = cp.T;
    } else {
        Scratch &s_small_ids = cp.s_small_ids;
        VIDC_TRY(roc_small_slots_clear(ctx, nlist, cp));
        uint32_t *lflag = cp.s_lf.as<uint32_t>();
        uint64_t *ltpos = cp.s_lt.as<uint64_t>();
        // the host's half: the same bounds on the mirror of the offsets
        std::vector<uint32_t> part;  // the partial lists, ascending
        std::vector<uint64_t> seg(1, 0);
        bool any_empty = false;
        nr->offsets[0] = 0;
        for (uint64_t l = 0; l < nlist; l++) {
            const uint64_t n = r->offsets[l + 1] - r->offsets[l];
            uint64_t i1 = 0, i2 = 0;
            if (ntotal_old) subset_bounds(type, a1, a2, ntotal_old, l, r->offsets[l], r->offsets[l + 1], i1, i2);
            const uint32_t c = subset_roc_class(n, i2 - i1);
            if (c == SUBC_PARTIAL) {
                part.push_back((uint32_t)l);
                seg.push_back(seg.back() + n);
                ts_off.push_back(ts_off.back() + (i2 - i1));
            }
            any_empty |= c == SUBC_EMPTY;
            nr->offsets[l + 1] = nr->offsets[l] + (i2 - i1);
        }
        nr->ntotal = nr->offsets[nlist];
        const uint64_t np = part.size(), total = seg[np], small_total = ts_off[np];
        if (any_empty) ts_off.push_back(small_total);  // the trailing empty list
        nsmall = ts_off.size() - 1;
        if (nlist && ntotal_old) {
            VIDC_TRY(s_lo.get(ctx, 4 * (nlist + 1) * 4));  // lo | sizes | cls | pflag
            VIDC_TRY(s_off.get(ctx, (nlist + 1) * 8));     // ppos
            VIDC_TRY(s_cand.get(ctx, (nlist + 1) * 4));
            uint32_t *lo = s_lo.as<uint32_t>(), *sizes = lo + nlist + 1, *cls = sizes + nlist + 1, *pflag = cls + nlist + 1;
            uint64_t *ppos = s_off.as<uint64_t>();
            uint32_t *d_part = s_cand.as<uint32_t>();
            hipLaunchKernelGGL(k_sub_bounds, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, (const uint64_t *)r->d_offsets.p, nlist, type, a1, a2, lo,
                               sizes, cls, pflag);
            VIDC_HIP(hipGetLastError());
            VIDC_TRY(device_exscan(ctx, pflag, (uint32_t)nlist, ppos, s_t0));
            hipLaunchKernelGGL(k_req_roc_touched, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, (const uint32_t *)pflag, (const uint64_t *)ppos, nlist,
                               d_part);
            hipLaunchKernelGGL(k_sub_roc_slots, req_grid(ctx, nlist), dim3(256), 0, ctx->stream, (const uint32_t *)cls, (const uint64_t *)ppos, nlist,
                               lflag, ltpos);
            VIDC_HIP(hipGetLastError());
            if (d_taken) {
                VIDC_TRY(app_chunks(ctx, r->d_offsets.p, nlist, ntotal_old, ch_t));
                hipLaunchKernelGGL(k_sub_slice, app_chunk_grid(ctx, ch_t.bound), dim3(256), 0, ctx->stream, (const uint64_t *)nullptr,
                                   (const uint64_t *)r->d_offsets.p, (const uint32_t *)nullptr, (const uint32_t *)lo, (const uint32_t *)sizes, ch_t.items,
                                   ch_t.n_items, (const uint64_t *)nullptr, (uint64_t *)nullptr, d_taken, (const uint64_t *)r->d_offsets.p);
                VIDC_HIP(hipGetLastError());
            }
            kernel_ms += tm.stop();
            if (np) {
                VIDC_TRY(s_stage.get(ctx, total * 8));
                VIDC_TRY(s_seg.get(ctx, (np + 1) * 8));
                VIDC_TRY(s_dst.get(ctx, (np + 1) * 8));
                VIDC_TRY(h_seg.get(ctx, (np + 1) * 8));
                VIDC_TRY(h_dst.get(ctx, (np + 1) * 8));
                std::memcpy(h_seg.p, seg.data(), (np + 1) * 8);
                std::memcpy(h_dst.p, ts_off.data(), (np + 1) * 8);
                VIDC_HIP(hipMemcpyAsync(s_seg.p, h_seg.p, (np + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
                VIDC_HIP(hipMemcpyAsync(s_dst.p, h_dst.p, (np + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
                VIDC_TRY(decode_into_staging(ctx, r, part, [&](uint32_t i) { return seg[i]; }, s_stage.as<uint64_t>(), kernel_ms));
                tr.mark("partial lists decoded");
                VIDC_TRY(s_small_ids.get(ctx, (small_total ? small_total : 1) * 8));
                (void)tm.start();
                VIDC_TRY(app_chunks(ctx, s_seg.as<uint64_t>(), np, total, ch_s));
                hipLaunchKernelGGL(k_sub_slice, app_chunk_grid(ctx, ch_s.bound), dim3(256), 0, ctx->stream, (const uint64_t *)s_stage.as<uint64_t>(),
                                   (const uint64_t *)s_seg.as<uint64_t>(), (const uint32_t *)d_part, (const uint32_t *)lo, (const uint32_t *)sizes,
                                   ch_s.items, ch_s.n_items, (const uint64_t *)s_dst.as<uint64_t>(), s_small_ids.as<uint64_t>(), (uint8_t *)nullptr,
                                   (const uint64_t *)nullptr);
                VIDC_HIP(hipGetLastError());
                kernel_ms += tm.stop();
            }
        } else {
            kernel_ms += tm.stop();
        }
        if (nsmall && !s_small_ids.p) VIDC_TRY(s_small_ids.get(ctx, 8));
        tr.mark("bounds, partial lists sliced");
    }
    if (nsmall) {
        vidc_roc *sp = nullptr;
        VIDC_TRY(encode_impl(ctx, nsmall, ts_off.data(), cp.s_small_ids.as<uint64_t>(), false, 0, 0, nullptr, precision_mode,
                             want_perm ? VIDC_ROC_WANT_PERM : 0u, &sp));
        small.reset(sp);
        kernel_ms += ctx->last_kernel_ms;
    }
    tr.mark("re-encoded lists encoded");
    (void)tm.start();
    VIDC_TRY(roc_splice(ctx, r, small.get(), cp.look(), nr.get(), want_perm, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    tr.mark("spliced");
    if (n_taken) *n_taken = nr->ntotal;
    *out = nr.release();
    return VIDC_OK;
}

// A copy of an IVF object on another context (common.h): the device arrays through hipMemcpyAsync(hipMemcpyDefault) on dst's stream,
// into blocks of dst's cache; the host offsets with them, no planner hints.  Waits.  Its only caller is the sharded re-balance, for a
// source shard on another device than its destination: NEVER EXECUTED, every test machine has one GPU.
int roc_clone_to(vidc_ctx *dst, const vidc_roc *r, vidc_roc **out) {
    if (out) *out = nullptr;
    if (!dst || !r || !out) { set_error("roc clone: NULL context, object or out"); return VIDC_ERR_INVALID; }
    if (r->rows) { set_error("roc clone: graph objects are not cloned"); return VIDC_ERR_UNSUPPORTED; }
    VIDC_TRY(ensure_offsets(r));
    VIDC_HIP(hipSetDevice(dst->device));
    std::unique_ptr<vidc_roc> nr(new vidc_roc());
    nr->device = dst->device;
    nr->nlist = r->nlist;
    nr->ntotal = r->ntotal;
    nr->total_words = r->total_words;
    nr->compressed_bytes = r->compressed_bytes;
    nr->offsets = r->offsets;
    nr->offsets_host = true;
    StreamGuard guard(dst);
    auto copy = [&](auto &to, const auto &from, size_t count, size_t alloc_count) -> int {
        VIDC_TRY(to.alloc(alloc_count, dst->dpool));
        if (count) VIDC_HIP(hipMemcpyAsync(to.p, from.p, count * sizeof(*to.p), hipMemcpyDefault, dst->stream));
        return VIDC_OK;
    };
    const size_t nl = r->nlist;
    VIDC_TRY(copy(nr->d_offsets, r->d_offsets, nl + 1, nl + 1));
    VIDC_TRY(copy(nr->d_word_off, r->d_word_off, nl + 1, nl + 1));
    VIDC_TRY(copy(nr->d_heads, r->d_heads, nl, nl));
    VIDC_TRY(copy(nr->d_prec, r->d_prec, nl, nl));
    VIDC_TRY(copy(nr->d_nwords, r->d_nwords, nl, nl));
    VIDC_TRY(copy(nr->d_draws, r->d_draws, nl, nl));
    VIDC_TRY(copy(nr->d_words, r->d_words, r->total_words, r->total_words + 16));  // + padding: see finish_complete
    if (r->d_perm.p) VIDC_TRY(copy(nr->d_perm, r->d_perm, r->ntotal, r->ntotal ? r->ntotal : 1));
    VIDC_HIP(vidc::vidc_stream_wait(dst->stream));
    guard.disarm();
    *out = nr.release();
    return VIDC_OK;
}
}  // namespace vidc
}
int vidc_roc_remove_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids, int precision_mode,
                        uint32_t flags, vidc_roc **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid) {
    return roc_remove(ctx, r, n_rm, d_list_nos, d_ids, precision_mode, flags, out, d_removed, d_missing, d_invalid, nullptr);
}

int vidc_roc_subset_dev(vidc_ctx *ctx, const vidc_roc *r, int subset_type, uint64_t a1, uint64_t a2, int precision_mode, uint32_t flags,
                        vidc_roc **out, uint8_t *d_taken, uint64_t *n_taken) {
    return vidc::roc_subset(ctx, r, subset_type, a1, a2, precision_mode, flags, out, d_taken, n_taken);
}

// Locate (include/vidc.h).  The batch is sorted as a remove sorts it and the same candidates are decoded (roc_decode_candidates), in
// ascending list order, and marked (locate.h).  The offsets are positions in sampling order, the order decode_lists and
// translate_labels use.
int vidc_roc_locate_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, int64_t *d_labels,
                        uint64_t *d_missing, uint64_t *d_invalid) {
    VIDC_TRY(locate_check(ctx, r, n, d_ids, d_labels));
    if (r->rows) { set_error("roc locate: graph objects hold no lists to locate in"); return VIDC_ERR_UNSUPPORTED; }
    if (!n) return VIDC_OK;
    VIDC_TRY(r->prec.size() == r->nlist ? ensure_offsets(r) : ensure_meta(r));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc locate");
    double kernel_ms = 0;
    LocateBatch b;
    AppChunks ch;
    RocCandPass cp;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    EventTimer tm = EventTimer::started(ctx);
    VIDC_TRY(locate_sort_batch(ctx, r->nlist, n, d_list_nos, d_ids, 32u, d_missing, d_invalid, b));
    VIDC_TRY(roc_decode_candidates(ctx, r, true, b.batch.any ? (const uint64_t *)nullptr : b.batch.run_off, cp, tr, tm, kernel_ms));
    (void)tm.start();
    if (cp.cnt) VIDC_TRY(locate_mark(ctx, b, cp.s_stage.as<uint64_t>(), cp.s_seg.as<uint64_t>(), cp.s_cand.as<uint32_t>(), cp.cnt, cp.total, ch));
    VIDC_TRY(locate_labels(ctx, b, d_labels, d_missing));
    ctx->last_kernel_ms = kernel_ms + tm.stop();
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));
    guard.disarm();
    tr.mark("candidates marked, labels written");
    return VIDC_OK;
}

// Regroup (include/vidc.h): the splice as a call of its own, over up to VIDC_SHARDS_MAX sources.  The (source, list) table is checked
// on the host and uploaded (12 bytes per list; RocRegroupTable).  No ANS step runs.
int vidc_roc_regroup(vidc_ctx *ctx, int nsrc, const vidc_roc *const *srcs, uint64_t m, const uint32_t *src_no, const uint64_t *list_no,
                     uint32_t flags, vidc_roc **out) {
    if (out) *out = nullptr;
    if (!ctx || !srcs || !out || (m && (!src_no || !list_no))) {
        set_error("roc regroup: NULL context, sources, out or table");
        return VIDC_ERR_INVALID;
    }
    if (nsrc < 1 || nsrc > VIDC_SHARDS_MAX) {
        set_error("roc regroup: nsrc %d outside 1 .. %d", nsrc, VIDC_SHARDS_MAX);
        return VIDC_ERR_INVALID;
    }
    if (m >= 0xffffffffull) { set_error("roc regroup: too many lists"); return VIDC_ERR_INVALID; }
    bool used[VIDC_SHARDS_MAX] = {};
    for (uint64_t j = 0; j < m; j++) {
        if (src_no[j] >= (uint32_t)nsrc) {
            set_error("roc regroup: list %llu names source %u of %d", (unsigned long long)j, src_no[j], nsrc);
            return VIDC_ERR_INVALID;
        }
        if (!srcs[src_no[j]]) {
            set_error("roc regroup: list %llu names source %u, which is NULL", (unsigned long long)j, src_no[j]);
            return VIDC_ERR_INVALID;
        }
        used[src_no[j]] = true;
    }
    // (from here on the sources are looked into)
    for (int k = 0; k < nsrc; k++)
        if (srcs[k] && srcs[k]->device != ctx->device) {
            set_error("roc regroup: source %d lives on device %d, the context on device %d", k, srcs[k]->device, ctx->device);
            return VIDC_ERR_INVALID;
        }
    for (uint64_t j = 0; j < m; j++)
        if (list_no[j] >= srcs[src_no[j]]->nlist) {
            set_error("roc regroup: list %llu names list %llu of source %u, which holds %llu", (unsigned long long)j,
                      (unsigned long long)list_no[j], src_no[j], (unsigned long long)srcs[src_no[j]]->nlist);
            return VIDC_ERR_INVALID;
        }
    for (int k = 0; k < nsrc; k++)
        if (srcs[k] && srcs[k]->rows) { set_error("roc regroup: source %d is a graph object", k); return VIDC_ERR_UNSUPPORTED; }
    for (int k = 0; k < nsrc; k++)
        if (used[k]) VIDC_TRY(ensure_offsets(srcs[k]));
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc regroup");
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0;
    std::unique_ptr<vidc_roc> nr = roc_derived(ctx, m);
    nr->offsets[0] = 0;
    for (uint64_t j = 0; j < m; j++) {
        const std::vector<uint64_t> &so = srcs[src_no[j]]->offsets;
        nr->offsets[j + 1] = nr->offsets[j] + (so[list_no[j] + 1] - so[list_no[j]]);
    }
    nr->ntotal = nr->offsets[m];
    Scratch s_tab;
    Pinned h_tab;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    VIDC_TRY(h_tab.get(ctx, m * 12 + 8));
    VIDC_TRY(s_tab.get(ctx, m * 12 + 8));
    uint64_t *h_list_no = h_tab.as<uint64_t>();  // list_no[m] | src_no[m]
    const uint64_t *d_list_no = s_tab.as<uint64_t>();
    const uint32_t *d_src_no = (const uint32_t *)(d_list_no + m);
    if (m) {
        std::memcpy(h_list_no, list_no, m * 8);
        std::memcpy(h_list_no + m, src_no, m * 4);
        VIDC_HIP(hipMemcpyAsync(s_tab.p, h_list_no, m * 12, hipMemcpyHostToDevice, ctx->stream));
    }
    RocSrcs<VIDC_SHARDS_MAX> S{};
    for (int k = 0; k < nsrc; k++)
        if (used[k]) S.s[k] = roc_src(srcs[k]);
    double kernel_ms = 0;
    EventTimer tm = EventTimer::started(ctx);
    VidcPhaseTimer copy_timer(ctx);  // (the word copy alone: VIDC_PHASE_ROC_REGROUP_COPY)
    // the convention of the append and the remove: a permutation of a derived object is over the positions of what the old lists
    // decode to -- the identity
    VIDC_TRY(roc_splice(ctx, S, RocRegroupTable{d_src_no, d_list_no}, nr.get(), want_perm, 0u, nullptr, &copy_timer, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    ctx->phase_ms[VIDC_PHASE_ROC_REGROUP_COPY] = copy_timer.collect();
    tr.mark("streams copied");
    *out = nr.release();
    return VIDC_OK;
}

// Update rows (include/vidc.h): the splice over {old object, the encoded batch rows}, with the slot table of rows_update.h built on the
// device (RocUpdateSlots).  The m batch rows are encoded by the rows path into a temporary object (every one of them, so every one is
// checked).  The object has no host mirror of its offsets: the edge total comes back with the splice's totals.  A row's stream depends
// on its multiset and precision alone: an untouched row keeps its words.
int vidc_roc_update_rows_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const int64_t *d_nodes, const int32_t *d_rows, uint64_t N_new,
                             int precision_mode, vidc_roc **out, uint64_t *d_invalid) {
    if (out) *out = nullptr;
    VIDC_TRY(rows_upd_check("roc", ctx, r, out, m, d_nodes, d_rows, r ? r->nlist : 0, N_new));
    if (!roc_precision_ok("roc update_rows: ", precision_mode)) return VIDC_ERR_INVALID;
    if (!r->rows) {
        if (r->K > TINY_MAX) set_error("roc update_rows: wide rows (K = %u > 64) are CSR objects: not supported", r->K);
        else set_error("roc update_rows: not a graph object (build it with vidc_roc_encode_rows)");
        return VIDC_ERR_UNSUPPORTED;
    }
    VIDC_HIP(hipSetDevice(ctx->device));
    HostTrace tr("roc update_rows");
    const uint64_t N_old = r->nlist;
    double kernel_ms = 0;
    std::unique_ptr<vidc_roc> tmp;
    if (m) {
        vidc_roc *t = nullptr;
        VIDC_TRY(vidc_roc_encode_rows(ctx, m, r->K, d_rows, precision_mode, 0, &t));
        tmp.reset(t);
        kernel_ms += ctx->last_kernel_ms;
    }
    tr.mark("batch rows encoded");
    std::unique_ptr<vidc_roc> nr = roc_derived(ctx, N_new, /*host_offsets=*/false);
    nr->rows = true;
    nr->K = r->K;
    Scratch s_slot;
    RocSpliceScratch sp_scratch;
    StreamGuard guard(ctx);  // (an early return waits for what is in flight before the blocks above go back)
    RocSrcs<2> S{};
    S.s[0] = roc_src(r);
    if (tmp) S.s[1] = roc_src(tmp.get());
    EventTimer tm = EventTimer::started(ctx);
    VIDC_TRY(rows_upd_slots(ctx, m, d_nodes, N_new, s_slot, d_invalid));
    VIDC_TRY(roc_splice(ctx, S, RocUpdateSlots{s_slot.as<uint32_t>(), N_old}, nr.get(), false, 0u, nullptr, nullptr, sp_scratch, tm, kernel_ms));
    VIDC_HIP(vidc::vidc_stream_wait(ctx->stream));  // (the scratch blocks go back to the context's cache)
    guard.disarm();
    ctx->last_kernel_ms = kernel_ms;
    tr.mark("streams copied");
    *out = nr.release();
    return VIDC_OK;
}

int vidc_roc_decode_rows_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const int64_t *d_nodes, uint32_t K, int32_t *d_out,
                             uint32_t *d_counts, uint64_t *d_invalid) {
    VIDC_TRY(req_check_rows(ctx, r, m, d_nodes, d_out));
    if (K == 0) { set_error("K=0 unsupported"); return VIDC_ERR_UNSUPPORTED; }  // (as vidc_roc_decode_rows)
    if (!m) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    const bool lean = K <= TINY_MAX && r->rows && K >= r->K && r->nlist && !force_general() && lane_wanted(lane_policy(), m, LANE_MIN_TINY);
    if (!lean)  // the plan of these shapes is built from the node numbers on the host
        return req_rows_via_host(ctx, r->nlist, m, d_nodes, K, d_out, d_counts, d_invalid,
                                 [&](const uint64_t *hn, uint32_t *hc) { return vidc_roc_decode_rows(ctx, r, m, hn, K, d_out, hc); });
    // lean lane path: the sanitized nodes are the decoder's work list, in request order; counts from the offsets, on the device
    Scratch s_wl;
    VIDC_TRY(s_wl.get(ctx, m * 4));
    hipLaunchKernelGGL(k_req_nodes_sanitize<uint32_t>, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, r->nlist,
                       s_wl.as<uint32_t>(), (unsigned long long *)d_invalid);
    if (d_counts)
        hipLaunchKernelGGL(k_gather_sizes<uint32_t>, dim3((uint32_t)std::min<uint64_t>((m + 255) / 256, 4096)), dim3(256), 0, ctx->stream,
                           r->d_offsets.p, s_wl.as<uint32_t>(), m, d_counts);
    VIDC_HIP(hipGetLastError());
    PooledDecPlan p;
    p.lean = true; p.tiny_lane = true; p.implicit = m;
    p.count[DC_TINY] = m;
    p.order_dev = s_wl.as<uint32_t>();
    p.order_req = true;
    VIDC_TRY(decode_impl(ctx, r, p, nullptr, nullptr, d_out, K));  // (ends with a synchronisation of the stream)
    hipLaunchKernelGGL(k_req_rows_fixup, req_grid(ctx, m), dim3(256), 0, ctx->stream, d_nodes, m, r->nlist, K, d_out, d_counts);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

}  // extern "C"
