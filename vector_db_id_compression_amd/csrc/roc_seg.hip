// roc_seg.hip -- vidc_rocseg (include/vidc.h): ROC lists cut by value range into segments, every segment an independent ANS chain over a
// smaller universe.  The plan is host code (roc_seg_plan.h); the inner object is an ordinary vidc_roc over the (list, segment) pairs,
// built and served through the public ROC entry points with VIDC_PREC_EXACT, so a segment IS what the single-object encoder builds from
// its rebased ids.  What is new on the device: the stable multisplit (k_rocseg_count, one scan, k_rocseg_scatter), the inner offsets
// gathered from that scan, the base fix-up behind a decode (k_rocseg_fix), the label rewrite and its base add (k_rocseg_labels,
// k_rocseg_add_base) and the permutation compose (k_rocseg_compose_perm).  No atomic decides a position: the histogram of pass 1 counts
// with LDS atomics (a sum), pass 2 ranks by ballot and keeps its running counts in wave-private LDS.
#include <mutex>

#include "common.h"
#include "host_call.h"
#include "requests.h"
#include "roc_seg_plan.h"
#include "scan.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::rocseg;

namespace {

// ------------------------------------------------------------------------------------------------------------------ kernels
// largest id of the call (universe_bits == 0): *out is zeroed by the caller
__global__ void __launch_bounds__(256) k_rocseg_max(const uint64_t *__restrict__ ids, uint64_t n, unsigned long long *out) {
    unsigned long long m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) m = ids[i] > m ? ids[i] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(m, o, 64);
        m = w > m ? w : m;
    }
    if (dev::lane_id() == 0 && m) atomicMax(out, m);
}

// segment of an id: x >> shift, clamped into the list's S segments (an id >= 2^B raises the domain flag; the clamp keeps both passes
// inside the list's own table entries and positions whatever the ids hold)
__device__ __forceinline__ uint32_t seg_key(uint64_t x, uint32_t shift, uint32_t S) {
    const uint64_t key = x >> shift;
    return key < S ? (uint32_t)key : S - 1u;
}

// Pass 1, a wavefront per chunk of SEG_CHUNK ids: table[tbl_base + s * nchunks + c] = ids of chunk c of the list that fall into segment
// s (one entry, the chunk's length, for a list that is not split); *flag |= 1 for an id >= 2^B.  chunks / lists come from the host plan:
// chunk.list < nlist and chunk.start < n of that list by construction (rocseg::make_plan).
__global__ void __launch_bounds__(256) k_rocseg_count(const uint64_t *__restrict__ ids, const ListSeg *__restrict__ lists,
                                                      const SplitChunk *__restrict__ chunks, uint64_t nchunks, uint32_t B,
                                                      uint32_t *__restrict__ table, uint32_t *flag) {
    __shared__ uint32_t hist[4][MAX_SEGS];
    const uint32_t lane = dev::lane_id(), w = threadIdx.x >> 6;
    bool bad = false;
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + w; c < nchunks; c += (uint64_t)gridDim.x * 4u) {
        const SplitChunk ch = chunks[c];
        const ListSeg L = lists[ch.list];
        const uint32_t left = L.n - ch.start, nc = left < SEG_CHUNK ? left : SEG_CHUNK;
        const uint32_t S = 1u << L.k, cl = ch.start / SEG_CHUNK;
        const uint64_t *src = ids + L.off + ch.start;
        if (L.k == 0) {
            for (uint32_t j = lane; j < nc; j += 64u) bad |= (src[j] >> B) != 0;
            if (lane == 0) table[L.tbl_base + cl] = nc;
            continue;
        }
        for (uint32_t s = lane; s < S; s += 64u) hist[w][s] = 0;
        dev::wave_lds_sync();
        for (uint32_t j = lane; j < nc; j += 64u) {
            const uint64_t x = src[j];
            bad |= (x >> B) != 0;
            atomicAdd(&hist[w][seg_key(x, L.shift, S)], 1u);
        }
        dev::wave_lds_sync();
        for (uint32_t s = lane; s < S; s += 64u) table[L.tbl_base + (uint64_t)s * L.nchunks + cl] = hist[w][s];
        dev::wave_lds_sync();
    }
    if (__ballot(bad) && lane == 0) atomicOr(flag, 1u);
}

// Pass 2, the same chunks: scan[] = the exclusive scan of the table = the first output position of (list, segment, chunk).  Inside a
// chunk the ids are taken 64 at a time in input order; a lane's rank among the lanes of its round with the same key comes from ballots
// over the k key bits, the count of earlier rounds from the wavefront's own LDS row, which the lowest lane of every key group advances.
// dst[pos] = the rebased id, src_pos[pos] (may be NULL) = its position inside the outer list.
__global__ void __launch_bounds__(256) k_rocseg_scatter(const uint64_t *__restrict__ ids, const ListSeg *__restrict__ lists,
                                                        const SplitChunk *__restrict__ chunks, uint64_t nchunks,
                                                        const uint64_t *__restrict__ scan, uint64_t *__restrict__ dst,
                                                        uint32_t *__restrict__ src_pos) {
    __shared__ uint32_t cnt[4][MAX_SEGS];
    const uint32_t lane = dev::lane_id(), w = threadIdx.x >> 6;
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + w; c < nchunks; c += (uint64_t)gridDim.x * 4u) {
        const SplitChunk ch = chunks[c];
        const ListSeg L = lists[ch.list];
        const uint32_t left = L.n - ch.start, nc = left < SEG_CHUNK ? left : SEG_CHUNK;
        const uint32_t S = 1u << L.k, cl = ch.start / SEG_CHUNK;
        const uint64_t *src = ids + L.off + ch.start;
        if (L.k == 0) {  // not split: a plain copy (scan[tbl_base + cl] == L.off + ch.start)
            uint64_t *d = dst + L.off + ch.start;
            for (uint32_t j = lane; j < nc; j += 64u) {
                d[j] = src[j];
                if (src_pos) src_pos[L.off + ch.start + j] = ch.start + j;
            }
            continue;
        }
        const uint64_t low = (1ull << L.shift) - 1ull;
        for (uint32_t s = lane; s < S; s += 64u) cnt[w][s] = 0;
        dev::wave_lds_sync();
        for (uint32_t j0 = 0; j0 < nc; j0 += 64u) {  // (j0, nc, k: wavefront-uniform)
            const uint32_t j = j0 + lane;
            const bool active = j < nc;
            const uint64_t x = active ? src[j] : 0;
            const uint32_t key = seg_key(x, L.shift, S);
            uint64_t peers = __ballot(active);
            for (uint32_t b = 0; b < L.k; b++) {
                const bool bit = (key >> b) & 1u;
                const uint64_t bal = __ballot(active && bit);
                peers &= bit ? bal : ~bal;
            }
            const uint32_t rank = dev::mbcnt(peers);
            const uint32_t before = cnt[w][key];
            dev::wave_lds_sync();
            if (active && rank == 0) cnt[w][key] = before + dev::popc64(peers);
            dev::wave_lds_sync();
            if (active) {
                const uint64_t pos = scan[L.tbl_base + (uint64_t)key * L.nchunks + cl] + before + rank;
                dst[pos] = x & low;
                if (src_pos) src_pos[pos] = ch.start + j;
            }
        }
    }
}

// list of an inner list number: the last l with lists[l].seg_first <= i (i < the inner list count)
__device__ __forceinline__ uint32_t list_of_inner(const ListSeg *__restrict__ lists, uint32_t nlist, uint32_t i) {
    uint32_t lo = 0, hi = nlist;  // lists[lo].seg_first <= i < lists[hi].seg_first (hi == nlist: the end)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (lists[mid].seg_first <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// inner_off[i] = the first position of inner list i: the scan entry of its chunk 0 (an empty list owns no entry: tbl_base names the
// next list's first, or the total)
__global__ void __launch_bounds__(256) k_rocseg_inner_offsets(const ListSeg *__restrict__ lists, uint32_t nlist, const uint64_t *__restrict__ scan,
                                                              uint64_t n_inner, uint64_t ntotal, uint64_t *__restrict__ inner_off) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_inner; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == n_inner) { inner_off[i] = ntotal; continue; }
        const ListSeg L = lists[list_of_inner(lists, nlist, (uint32_t)i)];
        inner_off[i] = scan[L.tbl_base + (i - L.seg_first) * L.nchunks];
    }
}

// the last i in [lo, hi) with off[i] <= g (off[lo] <= g < off[hi])
__device__ __forceinline__ uint64_t inner_of_pos(const uint64_t *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t g) {
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// perm[g] = src_pos[first position of g's inner list + inner_perm[g]]
__global__ void __launch_bounds__(256) k_rocseg_compose_perm(const uint64_t *__restrict__ inner_off, uint64_t n_inner, uint64_t ntotal,
                                                             const uint32_t *__restrict__ inner_perm, const uint32_t *__restrict__ src_pos,
                                                             uint32_t *__restrict__ perm) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ntotal; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = inner_of_pos(inner_off, 0, n_inner, g);
        perm[g] = src_pos[inner_off[i] + inner_perm[g]];
    }
}

// Base fix-up, a wavefront per chunk: out[start .. start + count) |= base (chunks from the host: rocseg::push_fix_chunks)
__global__ void __launch_bounds__(256) k_rocseg_fix(uint64_t *__restrict__ out, const FixChunk *__restrict__ chunks, uint64_t nchunks) {
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < nchunks; c += (uint64_t)gridDim.x * 4u) {
        const FixChunk ch = chunks[c];
        uint64_t *d = out + ch.start;
        for (uint32_t j = lane; j < ch.count; j += 64u) d[j] |= (uint64_t)ch.base;
    }
}

// Labels: list << 32 | off of the segmented object -> the inner object's label and the base of its segment.  A negative label stays
// negative; a list >= nlist or an offset >= the list's size becomes (inner list count) << 32, which the inner call answers with -1 and
// counts.
__global__ void __launch_bounds__(256) k_rocseg_labels(const int64_t *__restrict__ labels, uint64_t n, const ListSeg *__restrict__ lists,
                                                       uint64_t nlist, const uint64_t *__restrict__ inner_off, uint64_t n_inner,
                                                       int64_t *__restrict__ inner_labels, uint32_t *__restrict__ bases) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t list, off;
        int64_t out = -1;
        uint32_t base = 0;
        if (req_label(labels[i], list, off)) {
            out = (int64_t)(n_inner << 32);
            if (list < nlist) {
                const ListSeg L = lists[list];
                if (off < L.n) {
                    const uint64_t g = L.off + off;
                    const uint64_t s = inner_of_pos(inner_off, L.seg_first, (uint64_t)L.seg_first + (1ull << L.k), g);
                    out = (int64_t)(s << 32 | (g - inner_off[s]));
                    base = (uint32_t)((s - L.seg_first) << L.shift);
                }
            }
        }
        inner_labels[i] = out;
        bases[i] = base;
    }
}
__global__ void __launch_bounds__(256) k_rocseg_add_base(int64_t *__restrict__ ids, const uint32_t *__restrict__ bases, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t v = ids[i];
        if (v >= 0) ids[i] = v | (int64_t)bases[i];
    }
}

inline dim3 chunk_grid(const vidc_ctx *c, uint64_t nchunks) {
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nchunks + 3) / 4, (uint64_t)c->num_cu * 16)));
}

template <typename T>
int upload(vidc_ctx *ctx, DevBuf<T> &dst, const std::vector<T> &src) {
    VIDC_TRY(dst.alloc(src.size(), ctx->dpool));
    if (!src.empty()) VIDC_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return VIDC_OK;
}

}  // namespace

struct vidc_rocseg {
    vidc_roc *inner = nullptr;
    uint64_t nlist = 0, ntotal = 0, n_inner = 0, meta_segs = 0;
    uint32_t T = 0, B = 0;
    int device = 0;
    std::vector<uint64_t> seg_first;  // nlist + 1
    std::vector<uint8_t> shift;       // nlist
    DevBuf<ListSeg> d_lists;          // nlist (tbl_base is the encoder's own: unused afterwards)
    DevBuf<uint64_t> d_inner_off;     // n_inner + 1
    DevBuf<uint32_t> d_perm;          // ntotal, objects encoded with VIDC_ROC_WANT_PERM
    // the base fix-up of decode_all, made on first use
    mutable std::mutex mu;
    mutable bool fix_ready = false;
    mutable uint64_t n_fix = 0;
    mutable DevBuf<FixChunk> d_fix;
    ~vidc_rocseg() {
        if (inner) vidc_roc_destroy(inner);
    }
};

namespace {

int run_fix(vidc_ctx *ctx, uint64_t *d_out, const FixChunk *d_chunks, uint64_t n) {
    if (!n) return VIDC_OK;
    hipLaunchKernelGGL(k_rocseg_fix, chunk_grid(ctx, n), dim3(256), 0, ctx->stream, d_out, d_chunks, n);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}

// host offsets of the inner object (its list_info sizes, summed)
int inner_offsets_host(const vidc_roc *inner, uint64_t n_inner, std::vector<uint64_t> &off, std::vector<uint32_t> *prec) {
    std::vector<uint32_t> sizes(n_inner ? n_inner : 1);
    if (prec) prec->assign(n_inner ? n_inner : 1, 0);
    VIDC_TRY(vidc_roc_list_info(inner, sizes.data(), prec ? prec->data() : nullptr, nullptr, nullptr, nullptr));
    off.assign(n_inner + 1, 0);
    for (uint64_t i = 0; i < n_inner; i++) off[i + 1] = off[i] + sizes[i];
    return VIDC_OK;
}

int ensure_fix(vidc_ctx *ctx, const vidc_rocseg *s) {
    std::lock_guard<std::mutex> g(s->mu);
    if (s->fix_ready) return VIDC_OK;
    std::vector<uint64_t> off;
    VIDC_TRY(inner_offsets_host(s->inner, s->n_inner, off, nullptr));
    const std::vector<FixChunk> chunks = fix_chunks_all(s->seg_first, s->shift, off);
    VIDC_TRY(upload(ctx, s->d_fix, chunks));
    VIDC_HIP(vidc_stream_wait(ctx->stream));  // (the vector dies here)
    s->n_fix = chunks.size();
    s->fix_ready = true;
    return VIDC_OK;
}

int encode_body(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, uint64_t ntotal, const uint64_t *d_ids, uint32_t T, uint32_t B,
                uint32_t flags, vidc_rocseg **out) {
    for (uint64_t l = 0; l < nlist; l++)
        if (offsets[l + 1] < offsets[l]) { set_error("rocseg encode: offsets not monotone at list %llu", (unsigned long long)l); return VIDC_ERR_INVALID; }
    if (nlist >= 0xffffffffull || ntotal >= 0xffffffffull) { set_error("rocseg encode: too many lists or ids"); return VIDC_ERR_INVALID; }
    SegPlan plan;  // (its vectors are the sources of uploads: it outlives the guard's wait)
    std::unique_ptr<vidc_rocseg> s(new vidc_rocseg());
    DevBuf<SplitChunk> d_chunks;
    Scratch s_table, s_scan, s_tmp, s_rebased, s_srcpos;
    Scratch s_small;  // [0]: the largest id, [1]: the domain flag (low word)
    Pinned h_small;
    VIDC_TRY(s_small.get(ctx, 16));
    VIDC_TRY(h_small.get(ctx, 16));
    StreamGuard guard(ctx);  // (behind every block the kernels below use)
    VIDC_HIP(hipMemsetAsync(s_small.p, 0, 16, ctx->stream));
    EventTimer t = EventTimer::started(ctx);
    if (!B) {
        uint64_t mx = 0;
        if (ntotal) {
            hipLaunchKernelGGL(k_rocseg_max, req_grid(ctx, ntotal), dim3(256), 0, ctx->stream, d_ids, ntotal, s_small.as<unsigned long long>());
            VIDC_HIP(hipGetLastError());
            VIDC_HIP(hipMemcpyAsync(h_small.p, s_small.p, 8, hipMemcpyDeviceToHost, ctx->stream));
            VIDC_HIP(vidc_stream_wait(ctx->stream));
            mx = *h_small.as<uint64_t>();
        }
        if (mx >> 31) { set_error("rocseg encode: id %llu >= 2^31", (unsigned long long)mx); return VIDC_ERR_DOMAIN; }
        B = std::max(1u, bit_width(mx));
    }
    uint64_t bad = 0;
    switch (make_plan(offsets, nlist, T, B, plan, &bad)) {
    case PLAN_OK: break;
    case PLAN_TOO_MANY_SEGS:
        set_error("rocseg encode: list %llu (%llu ids) needs more than %u segments of %u ids", (unsigned long long)bad,
                  (unsigned long long)(offsets[bad + 1] - offsets[bad]), MAX_SEGS, T);
        return VIDC_ERR_DOMAIN;
    case PLAN_LIST_TOO_LONG: set_error("rocseg encode: list %llu is too long", (unsigned long long)bad); return VIDC_ERR_DOMAIN;
    default: set_error("rocseg encode: the segment table is too long (list %llu)", (unsigned long long)bad); return VIDC_ERR_OVERFLOW;
    }
    s->nlist = nlist; s->ntotal = ntotal; s->n_inner = plan.n_inner; s->meta_segs = plan.meta_segs;
    s->T = T; s->B = B; s->device = ctx->device;
    const uint64_t nchunks = plan.chunks.size();
    VIDC_TRY(upload(ctx, s->d_lists, plan.lists));
    VIDC_TRY(upload(ctx, d_chunks, plan.chunks));
    VIDC_TRY(s->d_inner_off.alloc(plan.n_inner + 1, ctx->dpool));
    VIDC_TRY(s_table.get(ctx, (plan.table_len + 1) * 4));
    VIDC_TRY(s_scan.get(ctx, (plan.table_len + 1) * 8));
    VIDC_TRY(s_rebased.get(ctx, (ntotal + 1) * 8));
    const bool want_perm = (flags & VIDC_ROC_WANT_PERM) != 0;
    if (want_perm) VIDC_TRY(s_srcpos.get(ctx, (ntotal + 1) * 4));
    uint32_t *flag = s_small.as<uint32_t>() + 2;
    if (nchunks) {
        hipLaunchKernelGGL(k_rocseg_count, chunk_grid(ctx, nchunks), dim3(256), 0, ctx->stream, d_ids, s->d_lists.p, d_chunks.p, nchunks, B,
                           s_table.as<uint32_t>(), flag);
        VIDC_HIP(hipGetLastError());
    }
    VIDC_TRY(device_exscan(ctx, s_table.as<uint32_t>(), (uint32_t)plan.table_len, s_scan.as<uint64_t>(), s_tmp));
    if (nchunks) {
        hipLaunchKernelGGL(k_rocseg_scatter, chunk_grid(ctx, nchunks), dim3(256), 0, ctx->stream, d_ids, s->d_lists.p, d_chunks.p, nchunks,
                           s_scan.as<uint64_t>(), s_rebased.as<uint64_t>(), want_perm ? s_srcpos.as<uint32_t>() : nullptr);
        VIDC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rocseg_inner_offsets, req_grid(ctx, plan.n_inner + 1), dim3(256), 0, ctx->stream, s->d_lists.p, (uint32_t)nlist,
                       s_scan.as<uint64_t>(), plan.n_inner, ntotal, s->d_inner_off.p);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(hipMemcpyAsync(h_small.p, s_small.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_TRY(t.finish());
    double part_ms = ctx->last_kernel_ms;
    if (h_small.as<uint32_t>()[2]) { set_error("rocseg encode: an id >= 2^%u (universe_bits)", B); return VIDC_ERR_DOMAIN; }
    VIDC_TRY(vidc_roc_encode_dev(ctx, plan.n_inner, s->d_inner_off.p, ntotal, s_rebased.as<uint64_t>(), VIDC_PREC_EXACT,
                                 want_perm ? VIDC_ROC_WANT_PERM : 0u, &s->inner));
    const double inner_ms = ctx->last_kernel_ms;
    if (want_perm) {
        VIDC_TRY(s->d_perm.alloc(ntotal, ctx->dpool));
        if (ntotal) {
            EventTimer t2 = EventTimer::started(ctx);
            hipLaunchKernelGGL(k_rocseg_compose_perm, req_grid(ctx, ntotal), dim3(256), 0, ctx->stream, s->d_inner_off.p, plan.n_inner, ntotal,
                               vidc_roc_perm_dev(s->inner), s_srcpos.as<uint32_t>(), s->d_perm.p);
            VIDC_HIP(hipGetLastError());
            VIDC_TRY(t2.finish());
            part_ms += ctx->last_kernel_ms;
        }
    }
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    guard.disarm();
    s->seg_first = std::move(plan.seg_first);
    s->shift = std::move(plan.shift);
    ctx->phase_ms[VIDC_PHASE_ROCSEG_PARTITION] = part_ms;
    ctx->last_kernel_ms = part_ms + inner_ms;
    *out = s.release();
    return VIDC_OK;
}

// the refusals every encode makes before any device work; T: 0 -> the default
int encode_args(const vidc_ctx *ctx, const void *offsets, uint64_t ntotal, const uint64_t *d_ids, uint32_t &T, uint32_t B, vidc_rocseg **out) {
    if (out) *out = nullptr;
    if (!ctx || !offsets || !out || (ntotal && !d_ids)) { set_error("rocseg encode: NULL context, offsets, ids or out"); return VIDC_ERR_INVALID; }
    if (!T) T = VIDC_ROCSEG_DEFAULT_IDS;
    if (!valid_seg_ids(T)) { set_error("rocseg encode: seg_ids %u is not a power of two in [%u, %u]", T, MIN_IDS, MAX_IDS); return VIDC_ERR_INVALID; }
    if (B > 31) { set_error("rocseg encode: universe_bits %u > 31", B); return VIDC_ERR_INVALID; }
    return VIDC_OK;
}

}  // namespace

static_assert(VIDC_ROCSEG_MAX_SEGS == MAX_SEGS, "vidc.h and roc_seg_plan.h disagree");
static_assert(sizeof(ListSeg) == 32 && sizeof(FixChunk) == 16, "device records");

extern "C" {

int vidc_rocseg_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, uint32_t seg_ids, uint32_t universe_bits,
                       uint32_t flags, vidc_rocseg **out) {
    // (ntotal is not known before offsets is: the ids are checked behind it)
    VIDC_TRY(encode_args(ctx, offsets, 0, nullptr, seg_ids, universe_bits, out));
    if (offsets[0] != 0) { set_error("rocseg encode: offsets[0] must be 0"); return VIDC_ERR_INVALID; }
    if (offsets[nlist] && !d_ids) { set_error("rocseg encode: NULL ids"); return VIDC_ERR_INVALID; }
    VIDC_HIP(hipSetDevice(ctx->device));
    return encode_body(ctx, nlist, offsets, offsets[nlist], d_ids, seg_ids, universe_bits, flags, out);
}

int vidc_rocseg_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids, uint32_t seg_ids,
                           uint32_t universe_bits, uint32_t flags, vidc_rocseg **out) {
    VIDC_TRY(encode_args(ctx, d_offsets, ntotal, d_ids, seg_ids, universe_bits, out));
    if (nlist >= 0xffffffffull) { set_error("rocseg encode: too many lists"); return VIDC_ERR_INVALID; }
    VIDC_HIP(hipSetDevice(ctx->device));
    std::vector<uint64_t> off(nlist + 1);
    VIDC_HIP(hipMemcpyAsync(off.data(), d_offsets, (nlist + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    if (off[0] != 0 || off[nlist] != ntotal) {
        set_error("rocseg encode: bad device offsets (offsets[0] must be 0, offsets[nlist] == ntotal)");
        return VIDC_ERR_INVALID;
    }
    return encode_body(ctx, nlist, off.data(), ntotal, d_ids, seg_ids, universe_bits, flags, out);
}

void vidc_rocseg_destroy(vidc_rocseg *s) { delete s; }

uint64_t vidc_rocseg_nlist(const vidc_rocseg *s) { return s ? s->nlist : 0; }
uint64_t vidc_rocseg_ntotal(const vidc_rocseg *s) { return s ? s->ntotal : 0; }
uint64_t vidc_rocseg_compressed_bytes(const vidc_rocseg *s) { return s ? vidc_roc_compressed_bytes(s->inner) + 4 * s->meta_segs : 0; }
uint32_t vidc_rocseg_seg_ids(const vidc_rocseg *s) { return s ? s->T : 0; }
uint32_t vidc_rocseg_universe_bits(const vidc_rocseg *s) { return s ? s->B : 0; }
const vidc_roc *vidc_rocseg_inner(const vidc_rocseg *s) { return s ? s->inner : nullptr; }
uint64_t vidc_rocseg_last_decode_handed_back(const vidc_rocseg *s) { return s ? vidc_roc_last_decode_handed_back(s->inner) : 0; }

int vidc_rocseg_seg_info(const vidc_rocseg *s, uint64_t *seg_first, uint8_t *shift) {
    if (!s) { set_error("rocseg seg_info: NULL object"); return VIDC_ERR_INVALID; }
    if (seg_first) std::memcpy(seg_first, s->seg_first.data(), (s->nlist + 1) * 8);
    if (shift && s->nlist) std::memcpy(shift, s->shift.data(), s->nlist);
    return VIDC_OK;
}

int vidc_rocseg_wrap(vidc_ctx *ctx, vidc_roc *inner, uint64_t nlist, const uint64_t *seg_first, const uint8_t *shift, uint32_t seg_ids,
                     uint32_t universe_bits, vidc_rocseg **out) {
    if (out) *out = nullptr;
    if (!ctx || !inner || !out || !seg_first || (nlist && !shift)) { set_error("rocseg wrap: NULL context, inner object, map or out"); return VIDC_ERR_INVALID; }
    if (!valid_seg_ids(seg_ids) || universe_bits < 1 || universe_bits > 31 || nlist >= 0xffffffffull) {
        set_error("rocseg wrap: seg_ids %u / universe_bits %u / nlist out of range", seg_ids, universe_bits);
        return VIDC_ERR_INVALID;
    }
    const uint64_t n_inner = vidc_roc_nlist(inner);
    if (n_inner >= 0x7fffffffull) { set_error("rocseg wrap: too many inner lists"); return VIDC_ERR_INVALID; }
    std::vector<uint64_t> off;
    std::vector<uint32_t> prec;
    VIDC_TRY(inner_offsets_host(inner, n_inner, off, &prec));
    if (const uint64_t bad = check_map(nlist, seg_first, shift, universe_bits, n_inner, prec.data())) {
        if (bad > nlist) set_error("rocseg wrap: seg_first must run from 0 to the inner object's %llu lists", (unsigned long long)n_inner);
        else set_error("rocseg wrap: the map of list %llu does not fit (segment count, shift or an inner precision)", (unsigned long long)(bad - 1));
        return VIDC_ERR_INVALID;
    }
    VIDC_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<vidc_rocseg> s(new vidc_rocseg());
    s->nlist = nlist; s->ntotal = vidc_roc_ntotal(inner); s->n_inner = n_inner;
    s->T = seg_ids; s->B = universe_bits; s->device = ctx->device;
    s->seg_first.assign(seg_first, seg_first + nlist + 1);
    s->shift.assign(shift, shift + nlist);
    std::vector<ListSeg> lists(nlist);
    for (uint64_t l = 0; l < nlist; l++) {
        const uint64_t a = off[seg_first[l]], b = off[seg_first[l + 1]], S = seg_first[l + 1] - seg_first[l];
        ListSeg &L = lists[l];
        L.off = a; L.tbl_base = 0; L.seg_first = (uint32_t)seg_first[l]; L.n = (uint32_t)(b - a);
        L.nchunks = (uint32_t)((b - a + SEG_CHUNK - 1) / SEG_CHUNK);
        L.k = (uint8_t)(universe_bits - shift[l]); L.shift = shift[l]; L.pad = 0;
        if (S > 1) s->meta_segs += S;
    }
    StreamGuard guard(ctx);
    VIDC_TRY(upload(ctx, s->d_lists, lists));
    VIDC_TRY(upload(ctx, s->d_inner_off, off));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    guard.disarm();
    s->inner = inner;
    *out = s.release();
    return VIDC_OK;
}

int vidc_rocseg_decode_all(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t *d_out) {
    if (!ctx || !s || (s->ntotal && !d_out)) { set_error("rocseg decode_all: NULL context, object or output"); return VIDC_ERR_INVALID; }
    VIDC_HIP(hipSetDevice(ctx->device));
    VIDC_TRY(ensure_fix(ctx, s));
    VIDC_TRY(vidc_roc_decode_all(ctx, s->inner, d_out));
    const double inner_ms = ctx->last_kernel_ms;
    EventTimer t = EventTimer::started(ctx);
    VIDC_TRY(run_fix(ctx, d_out, s->d_fix.p, s->n_fix));
    VIDC_TRY(t.finish());
    ctx->last_kernel_ms += inner_ms;
    return VIDC_OK;
}

int vidc_rocseg_decode_lists(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t m, const uint64_t *list_nos, uint64_t *d_out, uint64_t *out_offsets) {
    if (!ctx || !s || (m && !list_nos) || !out_offsets) { set_error("rocseg decode_lists: NULL context, object or array"); return VIDC_ERR_INVALID; }
    for (uint64_t j = 0; j < m; j++)
        if (list_nos[j] >= s->nlist) { set_error("rocseg decode_lists: list number %llu out of range", (unsigned long long)list_nos[j]); return VIDC_ERR_INVALID; }
    const std::vector<uint64_t> inner = expand_request(s->seg_first, m, list_nos);
    if (inner.empty()) {  // (m == 0: every list has a segment)
        out_offsets[0] = 0;
        return VIDC_OK;
    }
    std::vector<uint64_t> inner_out(inner.size() + 1, 0);
    VIDC_HIP(hipSetDevice(ctx->device));
    VIDC_TRY(vidc_roc_decode_lists(ctx, s->inner, inner.size(), inner.data(), d_out, inner_out.data()));
    const double inner_ms = ctx->last_kernel_ms;
    const std::vector<FixChunk> chunks = collapse_request(s->seg_first, s->shift, m, list_nos, inner_out, out_offsets);
    DevBuf<FixChunk> d_chunks;
    StreamGuard guard(ctx);
    VIDC_TRY(upload(ctx, d_chunks, chunks));
    EventTimer t = EventTimer::started(ctx);
    VIDC_TRY(run_fix(ctx, d_out, d_chunks.p, chunks.size()));
    VIDC_TRY(t.finish());
    guard.disarm();
    ctx->last_kernel_ms += inner_ms;
    return VIDC_OK;
}

int vidc_rocseg_translate_labels_dev(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t n, const int64_t *d_labels, int64_t *d_ids, uint64_t *d_invalid) {
    VIDC_TRY(req_check_labels(ctx, s, n, d_labels, d_ids));
    if (!n) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    Scratch s_labels, s_bases;
    VIDC_TRY(s_labels.get(ctx, n * 8));
    VIDC_TRY(s_bases.get(ctx, n * 4));
    StreamGuard guard(ctx);
    EventTimer t = EventTimer::started(ctx);
    hipLaunchKernelGGL(k_rocseg_labels, req_grid(ctx, n), dim3(256), 0, ctx->stream, d_labels, n, s->d_lists.p, s->nlist, s->d_inner_off.p,
                       s->n_inner, s_labels.as<int64_t>(), s_bases.as<uint32_t>());
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t.finish());
    double ms = ctx->last_kernel_ms;
    VIDC_TRY(vidc_roc_translate_labels_dev(ctx, s->inner, n, s_labels.as<int64_t>(), d_ids, d_invalid));
    ms += ctx->last_kernel_ms;
    EventTimer t2 = EventTimer::started(ctx);
    hipLaunchKernelGGL(k_rocseg_add_base, req_grid(ctx, n), dim3(256), 0, ctx->stream, d_ids, s_bases.as<uint32_t>(), n);
    VIDC_HIP(hipGetLastError());
    VIDC_TRY(t2.finish());
    guard.disarm();
    ctx->last_kernel_ms += ms;
    return VIDC_OK;
}

int vidc_rocseg_perm(vidc_ctx *ctx, const vidc_rocseg *s, uint32_t *perm_host) {
    if (!ctx || !s || !perm_host) { set_error("rocseg perm: NULL context, object or output"); return VIDC_ERR_INVALID; }
    if (!s->d_perm.p) { set_error("rocseg perm: the object was not encoded with VIDC_ROC_WANT_PERM"); return VIDC_ERR_INVALID; }
    if (!s->ntotal) return VIDC_OK;
    VIDC_HIP(hipSetDevice(ctx->device));
    VIDC_HIP(hipMemcpyAsync(perm_host, s->d_perm.p, s->ntotal * 4, hipMemcpyDeviceToHost, ctx->stream));
    VIDC_HIP(vidc_stream_wait(ctx->stream));
    return VIDC_OK;
}

}  // extern "C"
