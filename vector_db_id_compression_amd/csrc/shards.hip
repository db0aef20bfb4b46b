// shards.hip -- vidc_shards (include/vidc.h): one CSR set of lists cut over several contexts of one process.  The plan is host code
// (shard_plan.h); the shards are ordinary vidc_packed / vidc_ef / vidc_roc objects built and served through the public entry points, so a
// shard IS what the single-object encoder builds from its cut CSR.  What is new on the device: the segmented copy k_shard_copy<T, INV>
// (ids: cut, inverse cut, placement of decode_lists results; bytes: the shards' removed masks -> the global mask of a remove), the route
// k_shard_route<LABELS> (labels of translate_labels, pairs of append and remove) and the three joins (translate's ids, the append's
// labels, the remove's found bytes -> the missing count).  Append and remove are one skeleton (update_impl); the byte offsets of their
// scratch blocks come from shardplan::update_blocks; a shard on another device is served through one helper (FarStage, and DecodedIds
// for the decodes; the encoder's cut keeps its own copy), a path that has never executed.  The re-balance (vidc_rebalance_sharded) adds no
// kernel here: packed bits and Elias-Fano go through decode_all and encode_impl, ROC through vidc_roc_regroup per new shard (roc.hip).
#include <thread>

#include "common.h"
#include "host_call.h"
#include "requests.h"
#include "shard_plan.h"
#include "wave.h"

using namespace vidc;
using namespace vidc::shardplan;

namespace {

// ------------------------------------------------------------------------------------------------------------------ kernels
// Segmented copy, a wavefront per chunk of SHARD_COPY_UNIT elements of T (uint64_t: ids; uint8_t: the removed mask of a sharded remove):
// dst[seg.dst_start ..] = src[seg.src_start ..] (INV: the segment table read the other way round -- the inverse of the cut).  16-byte
// accesses where the two runs share their alignment mod 16, behind a head of less than 16 bytes (at most one id, at most 15 mask
// bytes) and in front of a tail of less than 16; accesses of one element otherwise.  chunks / segs come from the host plan: chunk.seg <
// the table's length and chunk.start < seg.count by construction (shardplan::build_copy_chunks).
template <typename T, bool INV>
__global__ void __launch_bounds__(256) k_shard_copy(const T *__restrict__ src, T *__restrict__ dst, const Segment *__restrict__ segs,
                                                    const CopyChunk *__restrict__ chunks, uint64_t nchunks) {
    constexpr uint32_t PER16 = 16u / (uint32_t)sizeof(T);
    const uint32_t lane = dev::lane_id();
    for (uint64_t c = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); c < nchunks; c += (uint64_t)gridDim.x * 4u) {
        const CopyChunk ch = chunks[c];
        const Segment sg = segs[ch.seg];
        const uint64_t left = sg.count - ch.start;
        const uint32_t nc = (uint32_t)(left < SHARD_COPY_UNIT ? left : SHARD_COPY_UNIT);
        const T *s = src + (INV ? sg.dst_start : sg.src_start) + ch.start;
        T *d = dst + (INV ? sg.src_start : sg.dst_start) + ch.start;
        if ((((uintptr_t)s ^ (uintptr_t)d) & 15u) == 0u) {
            uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u) / (uint32_t)sizeof(T);
            head = head < nc ? head : nc;
            if (lane < head) d[lane] = s[lane];
            const uint32_t nv = (nc - head) / PER16;  // (= (nc - head) * sizeof(T) / 16)
            const uint4 *sv = (const uint4 *)(s + head);
            uint4 *dv = (uint4 *)(d + head);
            for (uint32_t j = lane; j < nv; j += 64u) dv[j] = sv[j];
            for (uint32_t j = head + nv * PER16 + lane; j < nc; j += 64u) d[j] = s[j];
        } else {
            for (uint32_t j = lane; j < nc; j += 64u) d[j] = s[j];
        }
    }
}

constexpr uint32_t NO_OWNER = 0xffu;

// Route.  LABELS (translate_labels): req[i] is a label, local[s * n + i] = local_no << 32 | offset if shard s owns label i's list, else
// -1 (the shards' own translate gives -1 for a negative label and does not count it); the offset is checked by the owner.  !LABELS (the
// pairs of an append or a remove): req[i] is a list number, local[s * n + i] = its local number if shard s owns it, else -1 (the shards'
// own calls skip a negative list number and do not count it).  owner[i] = the owning shard, NO_OWNER for a negative request or a list >=
// nlist (the latter counted in *invalid).
template <bool LABELS>
__global__ void __launch_bounds__(256) k_shard_route(const int64_t *__restrict__ req, uint64_t n, const uint64_t *__restrict__ map, uint64_t nlist,
                                                     uint32_t nshards, int64_t *__restrict__ local, uint8_t *__restrict__ owner,
                                                     unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + dev::lane_id();
        const int64_t r = i < n ? req[i] : -1;
        uint64_t list = (uint64_t)r, off = 0;
        const bool pos = LABELS ? req_label(r, list, off) : r >= 0;
        const bool ok = pos && list < nlist;
        const uint64_t e = ok ? map[list] : 0;
        const uint32_t own = ok ? (uint32_t)(e >> 32) : NO_OWNER;
        if (i < n) {
            const int64_t mine = (int64_t)(LABELS ? (e & 0xffffffffull) << 32 | off : e & 0xffffffffull);
            for (uint32_t s = 0; s < nshards; s++) local[(uint64_t)s * n + i] = s == own ? mine : -1;
            owner[i] = (uint8_t)own;
        }
        req_count_invalid(pos && !ok, invalid);
    }
}

// Label join: ids[i] = the owner's answer, or -1; *invalid += the shards' own counts (offsets >= the list's size)
__global__ void __launch_bounds__(256) k_shard_join(const int64_t *__restrict__ answers, const uint8_t *__restrict__ owner, uint64_t n,
                                                    uint32_t nshards, int64_t *__restrict__ ids, const unsigned long long *__restrict__ shard_invalid,
                                                    unsigned long long *invalid) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t o = owner[i];
        ids[i] = o < nshards ? answers[(uint64_t)o * n + i] : -1;
    }
    if (invalid && blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long sum = 0;
        for (uint32_t s = 0; s < nshards; s++) sum += shard_invalid[s];
        if (sum) atomicAdd(invalid, sum);
    }
}

// Label join of an append: labels[i] = GLOBAL list number << 32 | the offset of the owner's label, or -1 for a skipped pair
__global__ void __launch_bounds__(256) k_shard_join_labels(const int64_t *__restrict__ list_nos, const int64_t *__restrict__ shard_labels,
                                                           const uint8_t *__restrict__ owner, uint64_t n, uint32_t nshards,
                                                           int64_t *__restrict__ labels) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t o = owner[i];
        const int64_t lab = o < nshards ? shard_labels[(uint64_t)o * n + i] : -1;
        labels[i] = lab >= 0 ? (int64_t)((uint64_t)list_nos[i] << 32 | ((uint64_t)lab & 0xffffffffull)) : -1;
    }
}

// Found join of a remove: *missing += the valid pairs (owner == NULL, any-list mode: every pair; else owner[i] != NO_OWNER) that no shard
// found.  found[s * n + i]: shard s's byte for pair i (a shard that does not own the pair's list saw list -1 and answered 0; a shard
// without an object left the zeros of the memset).
__global__ void __launch_bounds__(256) k_shard_join_found(const uint8_t *__restrict__ found, const uint8_t *__restrict__ owner, uint64_t n,
                                                          uint32_t nshards, unsigned long long *missing) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (i0: wavefront-uniform)
        const uint64_t i = i0 + dev::lane_id();
        const bool valid = i < n && (!owner || owner[i] != NO_OWNER);
        uint32_t any = 0;
        if (valid)
            for (uint32_t s = 0; s < nshards; s++) any |= found[(uint64_t)s * n + i];
        req_count_invalid(valid && !any, missing);
    }
}

inline dim3 copy_grid(const vidc_ctx *c, uint64_t nchunks) {
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nchunks + 3) / 4, (uint64_t)c->num_cu * 16)));
}

// ------------------------------------------------------------------------------------------- the codecs behind one switch
int codec_encode(int kind, vidc_ctx *c, uint64_t nlist, const uint64_t *off, const uint64_t *d_ids, int param, uint32_t flags, void **out) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_encode(c, nlist, off, d_ids, param, (vidc_packed **)out);
    case VIDC_KIND_EF: return vidc_ef_encode(c, nlist, off, d_ids, flags, (vidc_ef **)out);
    default: return vidc_roc_encode(c, nlist, off, d_ids, param, flags, (vidc_roc **)out);
    }
}
void codec_destroy(int kind, void *o) {
    if (!o) return;
    switch (kind) {
    case VIDC_KIND_PACKED: vidc_packed_destroy((vidc_packed *)o); break;
    case VIDC_KIND_EF: vidc_ef_destroy((vidc_ef *)o); break;
    default: vidc_roc_destroy((vidc_roc *)o); break;
    }
}
uint64_t codec_bytes(int kind, const void *o) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_compressed_bytes((const vidc_packed *)o);
    case VIDC_KIND_EF: return vidc_ef_compressed_bytes((const vidc_ef *)o);
    default: return vidc_roc_compressed_bytes((const vidc_roc *)o);
    }
}
int codec_decode_all(int kind, vidc_ctx *c, const void *o, uint64_t *d_out) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_decode_all(c, (const vidc_packed *)o, d_out);
    case VIDC_KIND_EF: return vidc_ef_decode_all(c, (const vidc_ef *)o, d_out);
    default: return vidc_roc_decode_all(c, (const vidc_roc *)o, d_out);
    }
}
int codec_decode_lists(int kind, vidc_ctx *c, const void *o, uint64_t m, const uint64_t *lists, uint64_t *d_out, uint64_t *out_off) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_decode_lists(c, (const vidc_packed *)o, m, lists, d_out, out_off);
    case VIDC_KIND_EF: return vidc_ef_decode_lists(c, (const vidc_ef *)o, m, lists, d_out, out_off);
    default: return vidc_roc_decode_lists(c, (const vidc_roc *)o, m, lists, d_out, out_off);
    }
}
int codec_decode_gather(int kind, vidc_ctx *c, const void *o, uint64_t m, const uint64_t *lists, uint64_t n, const uint64_t *slot,
                        const uint64_t *off, int64_t *out) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_decode_gather(c, (const vidc_packed *)o, m, lists, n, slot, off, out);
    case VIDC_KIND_EF: return vidc_ef_decode_gather(c, (const vidc_ef *)o, m, lists, n, slot, off, out);
    default: return vidc_roc_decode_gather(c, (const vidc_roc *)o, m, lists, n, slot, off, out);
    }
}
int codec_translate(int kind, vidc_ctx *c, const void *o, uint64_t n, const int64_t *d_labels, int64_t *d_ids, uint64_t *d_invalid) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_translate_labels_dev(c, (const vidc_packed *)o, n, d_labels, d_ids, d_invalid);
    case VIDC_KIND_EF: return vidc_ef_translate_labels_dev(c, (const vidc_ef *)o, n, d_labels, d_ids, d_invalid);
    default: return vidc_roc_translate_labels_dev(c, (const vidc_roc *)o, n, d_labels, d_ids, d_invalid);
    }
}
int codec_append(int kind, vidc_ctx *c, const void *o, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, int param, uint32_t flags,
                 void **out, int64_t *d_labels, uint64_t *d_invalid) {
    switch (kind) {
    case VIDC_KIND_PACKED: return vidc_packed_append_dev(c, (const vidc_packed *)o, n, d_list_nos, d_ids, param, (vidc_packed **)out, d_labels, d_invalid);
    case VIDC_KIND_EF: return vidc_ef_append_dev(c, (const vidc_ef *)o, n, d_list_nos, d_ids, flags, (vidc_ef **)out, d_labels, d_invalid);
    default: return vidc_roc_append_dev(c, (const vidc_roc *)o, n, d_list_nos, d_ids, param, flags, (vidc_roc **)out, d_labels, d_invalid);
    }
}
int codec_remove(int kind, vidc_ctx *c, const void *o, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, int param, uint32_t flags,
                 void **out, uint8_t *d_removed, uint64_t *d_invalid, uint8_t *d_pair_found) {
    switch (kind) {
    case VIDC_KIND_PACKED: return packed_remove(c, (const vidc_packed *)o, n, d_list_nos, d_ids, (vidc_packed **)out, d_removed, nullptr, d_invalid, d_pair_found);
    case VIDC_KIND_EF: return ef_remove(c, (const vidc_ef *)o, n, d_list_nos, d_ids, flags, (vidc_ef **)out, d_removed, nullptr, d_invalid, d_pair_found);
    default: return roc_remove(c, (const vidc_roc *)o, n, d_list_nos, d_ids, param, flags, (vidc_roc **)out, d_removed, nullptr, d_invalid, d_pair_found);
    }
}
// the sizes of an object's nl lists, through the codecs' host-side accessors (metadata mirrored on first use)
int codec_list_sizes(int kind, vidc_ctx *c, const void *o, uint64_t nl, std::vector<uint64_t> &sizes) {
    sizes.assign(nl, 0);
    if (kind == VIDC_KIND_PACKED) {
        std::vector<uint64_t> off(nl + 1);
        VIDC_TRY(vidc_packed_offsets(c, (const vidc_packed *)o, off.data()));
        for (uint64_t l = 0; l < nl; l++) sizes[l] = off[l + 1] - off[l];
        return VIDC_OK;
    }
    std::vector<uint32_t> n32(nl ? nl : 1);
    VIDC_TRY(kind == VIDC_KIND_EF ? vidc_ef_list_info((const vidc_ef *)o, n32.data(), nullptr, nullptr)
                                  : vidc_roc_list_info((const vidc_roc *)o, n32.data(), nullptr, nullptr, nullptr, nullptr));
    for (uint64_t l = 0; l < nl; l++) sizes[l] = n32[l];
    return VIDC_OK;
}

}  // namespace

struct vidc_shards {
    int kind = 0, param = 0;
    uint32_t flags = 0;
    vidc_ctx *home = nullptr;
    std::vector<vidc_ctx *> ctxs;
    std::vector<void *> objs;  // NULL: the shard owns no list
    ShardPlan plan;
    // on the home device: the map, and per shard the cut's segment and chunk tables
    DevBuf<uint64_t> d_map;
    std::vector<DevBuf<Segment>> d_cut;
    std::vector<DevBuf<CopyChunk>> d_cut_chunks;
    std::vector<uint64_t> n_cut_chunks;
    // ordering between the home stream and the shard streams: ev_home is recorded on the home stream (home device), ev_shard[s] on
    // shard s's stream (its device); timing disabled
    hipEvent_t ev_home = nullptr;
    std::vector<hipEvent_t> ev_shard;
    bool same_device(int s) const { return ctxs[(size_t)s]->device == home->device; }
    ~vidc_shards() {
        for (size_t i = 0; i < objs.size(); i++) codec_destroy(kind, objs[i]);
        if (ev_home) (void)hipEventDestroy(ev_home);
        for (hipEvent_t e : ev_shard)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

// One host thread per involved shard (the per-shard calls wait): f(shard) -> status.  The status of the lowest-numbered failing shard is
// returned and vidc_last_error carries "shard i: " + that shard's message (the message is thread-local: it is fetched in the worker).
template <typename F>
int fan_out(const std::vector<int> &shards, F &&f) {
    const size_t k = shards.size();
    std::vector<int> st(k, VIDC_OK);
    std::vector<std::string> msg(k);
    auto run = [&](size_t i) {
        st[i] = f(shards[i]);
        if (st[i] != VIDC_OK) msg[i] = vidc_last_error();
    };
    if (k == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        th.reserve(k);
        for (size_t i = 0; i < k; i++) th.emplace_back(run, i);
        for (auto &t : th) t.join();
    }
    for (size_t i = 0; i < k; i++)
        if (st[i] != VIDC_OK) {
            set_error("shard %d: %s", shards[i], msg[i].c_str());
            return st[i];
        }
    return VIDC_OK;
}

// waits for the streams of the shards a call touched when the scope is left (an early return must not hand staging back while work on
// it is in flight); the home stream has its own StreamGuard
struct ShardStreamsGuard {
    const vidc_shards *s;
    std::vector<int> which;
    explicit ShardStreamsGuard(const vidc_shards *s_) : s(s_) {}
    ~ShardStreamsGuard() {
        for (int i : which) {
            vidc_ctx *c = s->ctxs[(size_t)i];
            if (hipSetDevice(c->device) == hipSuccess) (void)vidc_stream_wait(c->stream);
        }
        (void)hipSetDevice(s->home->device);
    }
};

// segments (+ their chunk table) uploaded into scratch of the home context and copied on the home stream.  The host vectors must live
// until the home stream has been waited for.
struct StagedCopy {
    Scratch s_seg, s_chunk;
    std::vector<CopyChunk> chunks;
};
template <bool INV, typename T>
int launch_copy(vidc_ctx *home, const T *src, T *dst, const Segment *d_segs, const CopyChunk *d_chunks, uint64_t nchunks) {
    if (!nchunks) return VIDC_OK;
    hipLaunchKernelGGL((k_shard_copy<T, INV>), copy_grid(home, nchunks), dim3(256), 0, home->stream, src, dst, d_segs, d_chunks, nchunks);
    VIDC_HIP(hipGetLastError());
    return VIDC_OK;
}
int staged_copy(vidc_ctx *home, const uint64_t *src, uint64_t *dst, const std::vector<Segment> &segs, StagedCopy &sc) {
    if (segs.empty()) return VIDC_OK;
    sc.chunks = build_copy_chunks(segs);
    VIDC_TRY(sc.s_seg.get(home, segs.size() * sizeof(Segment)));
    VIDC_TRY(sc.s_chunk.get(home, sc.chunks.size() * sizeof(CopyChunk)));
    VIDC_HIP(hipMemcpyAsync(sc.s_seg.p, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice, home->stream));
    VIDC_HIP(hipMemcpyAsync(sc.s_chunk.p, sc.chunks.data(), sc.chunks.size() * sizeof(CopyChunk), hipMemcpyHostToDevice, home->stream));
    return launch_copy<false>(home, src, dst, sc.s_seg.as<Segment>(), sc.s_chunk.as<CopyChunk>(), sc.chunks.size());
}

int check_request(const vidc_ctx *home, const vidc_shards *s, const char *what) {
    if (!home || !s) {
        set_error("%s: NULL context or object", what);
        return VIDC_ERR_INVALID;
    }
    if (home != s->home) {
        set_error("%s: not the home context the object was built with", what);
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}

// the argument checks of the two encode calls: before any device work
int check_encode(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, const uint64_t *offsets, const uint64_t *d_ids, uint64_t nlist,
                 vidc_shards **out, bool ids_needed) {
    if (out) *out = nullptr;
    if (!home || !shard_ctxs || !offsets || !out || (ids_needed && !d_ids)) {
        set_error("shards encode: NULL argument");
        return VIDC_ERR_INVALID;
    }
    if (nshards < 1 || nshards > VIDC_SHARDS_MAX) {
        set_error("shards encode: nshards %d outside 1 .. %d", nshards, VIDC_SHARDS_MAX);
        return VIDC_ERR_INVALID;
    }
    for (int i = 0; i < nshards; i++) {
        if (!shard_ctxs[i]) {
            set_error("shards encode: shard context %d is NULL", i);
            return VIDC_ERR_INVALID;
        }
        for (int j = 0; j < i; j++)
            if (shard_ctxs[j] == shard_ctxs[i]) {
                set_error("shards encode: shard contexts %d and %d are the same context", j, i);
                return VIDC_ERR_INVALID;
            }
    }
    if (kind < VIDC_KIND_PACKED || kind > VIDC_KIND_WT) {
        set_error("shards encode: unknown kind %d", kind);
        return VIDC_ERR_INVALID;
    }
    if (kind == VIDC_KIND_WT) {
        set_error("shards encode: the wavelet tree cannot be sharded (a shard's ids are not a permutation of 0 .. n - 1)");
        return VIDC_ERR_UNSUPPORTED;
    }
    if (nlist >= (1ull << 32)) {
        set_error("shards encode: nlist must be below 2^32");
        return VIDC_ERR_INVALID;
    }
    return VIDC_OK;
}

// What every new object sets up, from encode and from append alike.  The events: one on the home device, one per shard on its device.
int create_events(vidc_shards *S) {
    const int nshards = (int)S->ctxs.size();
    S->ev_shard.assign((size_t)nshards, nullptr);
    for (int s = 0; s < nshards; s++) {
        VIDC_HIP(hipSetDevice(S->ctxs[(size_t)s]->device));
        VIDC_HIP(hipEventCreateWithFlags(&S->ev_shard[(size_t)s], hipEventDisableTiming));
    }
    VIDC_HIP(hipSetDevice(S->home->device));
    VIDC_HIP(hipEventCreateWithFlags(&S->ev_home, hipEventDisableTiming));
    return VIDC_OK;
}
// The map and, per shard that owns a list, the cut's segment and chunk tables of S->plan: allocated from the home context's cache and
// uploaded on the home stream (current device: home).  The host vectors in `t` must live until the home stream has been waited for.
struct PlanTables {
    std::vector<uint64_t> map;
    std::vector<std::vector<CopyChunk>> chunks;
};
int upload_plan(vidc_shards *S, PlanTables &t) {
    const ShardPlan &P = S->plan;
    vidc_ctx *home = S->home;
    const size_t ns = (size_t)P.nshards;
    t.map.resize(P.nlist);
    for (uint64_t l = 0; l < P.nlist; l++) t.map[l] = P.packed(l);
    t.chunks.assign(ns, {});
    VIDC_TRY(S->d_map.alloc(P.nlist, home->dpool));
    if (P.nlist) VIDC_HIP(hipMemcpyAsync(S->d_map.p, t.map.data(), P.nlist * 8, hipMemcpyHostToDevice, home->stream));
    S->d_cut.resize(ns);
    S->d_cut_chunks.resize(ns);
    S->n_cut_chunks.assign(ns, 0);
    for (size_t i = 0; i < ns; i++) {
        if (P.lists[i].empty()) continue;
        t.chunks[i] = build_copy_chunks(P.cut[i]);
        S->n_cut_chunks[i] = t.chunks[i].size();
        VIDC_TRY(S->d_cut[i].alloc(P.cut[i].size(), home->dpool));
        VIDC_TRY(S->d_cut_chunks[i].alloc(t.chunks[i].size(), home->dpool));
        if (!P.cut[i].empty()) {
            VIDC_HIP(hipMemcpyAsync(S->d_cut[i].p, P.cut[i].data(), P.cut[i].size() * sizeof(Segment), hipMemcpyHostToDevice, home->stream));
            VIDC_HIP(hipMemcpyAsync(S->d_cut_chunks[i].p, t.chunks[i].data(), t.chunks[i].size() * sizeof(CopyChunk), hipMemcpyHostToDevice, home->stream));
        }
    }
    return VIDC_OK;
}

// host offsets (checked: start at 0, monotone) -> the object
int encode_impl(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, int param, uint32_t flags, uint64_t nlist,
                const uint64_t *offsets, const uint64_t *d_ids, vidc_shards **out) {
    if (offsets[0] != 0) {
        set_error("shards encode: offsets[0] must be 0");
        return VIDC_ERR_INVALID;
    }
    for (uint64_t l = 0; l < nlist; l++)
        if (offsets[l + 1] < offsets[l]) {
            set_error("shards encode: offsets decrease at list %llu", (unsigned long long)l);
            return VIDC_ERR_INVALID;
        }
    if (offsets[nlist] && !d_ids) {
        set_error("shards encode: NULL argument");
        return VIDC_ERR_INVALID;
    }
    std::unique_ptr<vidc_shards> S(new vidc_shards());
    S->kind = kind;
    S->flags = flags;
    S->home = home;
    S->ctxs.assign(shard_ctxs, shard_ctxs + nshards);
    S->objs.assign((size_t)nshards, nullptr);
    S->plan = make_plan(offsets, nlist, nshards);
    const ShardPlan &P = S->plan;
    S->param = kind == VIDC_KIND_PACKED && param == 0 ? vidc_packed_bits_for(P.ntotal) : param;  // (one width for every shard)
    VIDC_TRY(create_events(S.get()));

    PlanTables tables;
    std::vector<Scratch> cut_home((size_t)nshards), cut_shard((size_t)nshards);  // the shards' contiguous ids
    std::vector<int> involved;
    ShardStreamsGuard sguard(S.get());
    StreamGuard hguard(home);
    VIDC_TRY(upload_plan(S.get(), tables));
    for (int s = 0; s < nshards; s++) {
        const size_t i = (size_t)s;
        if (P.lists[i].empty()) continue;
        involved.push_back(s);
        // a shard on the home device: the cut writes the block its encoder reads
        VIDC_TRY((S->same_device(s) ? cut_shard[i] : cut_home[i]).get(S->same_device(s) ? S->ctxs[i] : home, (P.load[i] ? P.load[i] : 2) * 8));
    }
    // the cut: one launch per shard on the home stream; its kernel time is the home context's last_kernel_ms (unless a shard's encode
    // runs on the home context as well and overwrites it)
    EventTimer cut_timer(home);
    VIDC_HIP(cut_timer.start());
    for (int s : involved) {
        const size_t i = (size_t)s;
        uint64_t *dst = (S->same_device(s) ? cut_shard[i] : cut_home[i]).as<uint64_t>();
        VIDC_TRY(launch_copy<false>(home, d_ids, dst, S->d_cut[i].p, S->d_cut_chunks[i].p, S->n_cut_chunks[i]));
    }
    VIDC_HIP(cut_timer.mark());
    // every shard's encode waits anyway: the cut is waited for here, once, before the shard threads start
    VIDC_HIP(vidc_stream_wait(home->stream));
    home->last_kernel_ms = cut_timer.elapsed();
    hguard.disarm();
    sguard.which = involved;
    vidc_shards *Sp = S.get();
    int st = involved.empty() ? VIDC_OK : fan_out(involved, [&](int s) -> int {
        const size_t i = (size_t)s;
        vidc_ctx *c = Sp->ctxs[i];
        VIDC_HIP(hipSetDevice(c->device));
        if (!Sp->same_device(s)) {
            VIDC_TRY(cut_shard[i].get(c, (P.load[i] ? P.load[i] : 2) * 8));
            if (P.load[i]) VIDC_HIP(hipMemcpyAsync(cut_shard[i].p, cut_home[i].p, P.load[i] * 8, hipMemcpyDefault, c->stream));
        }
        VIDC_TRY(codec_encode(kind, c, P.lists[i].size(), P.local_offsets[i].data(), cut_shard[i].as<uint64_t>(), Sp->param, flags, &Sp->objs[i]));
        VIDC_HIP(vidc_stream_wait(c->stream));
        return VIDC_OK;
    });
    // (the guard waits for the shard streams -- a failing shard's siblings have finished -- and goes back to the home device)
    if (st != VIDC_OK) return st;  // ~vidc_shards destroys what was built
    *out = S.release();
    return VIDC_OK;
}

std::vector<int> shards_with_ids(const vidc_shards *s) {
    std::vector<int> v;
    for (int i = 0; i < s->plan.nshards; i++)
        if (s->objs[(size_t)i] && s->plan.load[(size_t)i]) v.push_back(i);
    return v;
}
std::vector<int> shards_with_objects(const vidc_shards *s) {
    std::vector<int> v;
    for (int i = 0; i < s->plan.nshards; i++)
        if (s->objs[(size_t)i]) v.push_back(i);
    return v;
}

// ------------------------------------------------------------------------------------------------- a shard on another device
// Both helpers do nothing for a shard on the home device, which reads and writes the home context's blocks in place.  Their other
// branches have never executed: every test machine has one GPU.

// One shard's arrays of a routed call (translate_labels, append, remove).  For a shard elsewhere a block of the shard's own cache stands
// in, at the offsets of an UpdateBlocks: in() copies into it on the shard's stream at once, out() hands out a part of it and flush()
// enqueues the copies back.  A failed HIP call stays in `st` (and in vidc_last_error) and the later calls do nothing, so the caller
// looks at `st` once, before it uses the pointers.
struct FarStage {
    struct Back { void *home; const void *far; size_t bytes; };
    vidc_ctx *c = nullptr;
    Scratch blk;  // empty: the shard is on the home device
    Back back[4] = {};
    int nback = 0, st = VIDC_OK;
    // sets the current device to the shard's
    int open(const vidc_shards *s, int sh, size_t bytes) {
        c = s->ctxs[(size_t)sh];
        VIDC_HIP(hipSetDevice(c->device));
        if (!s->same_device(sh)) st = blk.get(c, bytes);
        return st;
    }
    int copy(void *dst, const void *src, size_t bytes) {
        if (bytes) VIDC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
        return VIDC_OK;
    }
    int zero(void *p, size_t bytes) {
        VIDC_HIP(hipMemsetAsync(p, 0, bytes, c->stream));
        return VIDC_OK;
    }
    // the pointer the shard's call reads: home (NULL stays NULL), or its copy at `off` of the far block
    template <typename T>
    const T *in(const T *home, size_t off, size_t bytes) {
        if (!blk.p || !home) return home;
        T *far = (T *)(blk.as<uint8_t>() + off);
        if (st == VIDC_OK) st = copy(far, home, bytes);
        return far;
    }
    // the pointer the shard's call writes: home (NULL stays NULL), or `off` of the far block, copied back by flush()
    template <typename T>
    T *out(T *home, size_t off, size_t bytes) {
        if (!blk.p || !home) return home;
        back[nback++] = Back{home, blk.as<uint8_t>() + off, bytes};
        return (T *)(blk.as<uint8_t>() + off);
    }
    // the shard's invalid counter: the home one (the caller zeroed it), or the far block's first word, zeroed here
    uint64_t *counter(unsigned long long *home) {
        if (blk.p && st == VIDC_OK) st = zero(blk.p, 8);
        return out((uint64_t *)home, 0, 8);
    }
    int flush() {
        for (int k = 0; k < nback && st == VIDC_OK; k++) st = copy(back[k].home, back[k].far, back[k].bytes);
        return st;
    }
};

// The ids a shard decodes: `decode(c, dst)` enqueues the shard's decode of n_ids ids into a block of its own cache; a shard elsewhere
// copies them to a block of the home cache on its stream; the shard's stream is waited for.  ids(): what the home stream reads.
struct DecodedIds {
    Scratch shard, home;
    const uint64_t *ids() const { return (home.p ? home : shard).as<uint64_t>(); }
    template <typename Decode>
    int run(const vidc_shards *s, int sh, uint64_t n_ids, Decode &&decode) {
        vidc_ctx *c = s->ctxs[(size_t)sh];
        VIDC_HIP(hipSetDevice(c->device));
        VIDC_TRY(shard.get(c, n_ids * 8));
        VIDC_TRY(decode(c, shard.as<uint64_t>()));
        if (!s->same_device(sh)) {
            VIDC_HIP(hipSetDevice(s->home->device));
            VIDC_TRY(home.get(s->home, n_ids * 8));
            VIDC_HIP(hipSetDevice(c->device));
            VIDC_HIP(hipMemcpyAsync(home.p, shard.p, n_ids * 8, hipMemcpyDefault, c->stream));
        }
        VIDC_HIP(vidc_stream_wait(c->stream));
        return VIDC_OK;
    }
};

// ------------------------------------------------------------------------------------------- append and remove: one skeleton
struct UpdateNames {  // the error prefix and the VIDC_TRACE phases
    const char *call, *a_shard, *shards_done, *tail_enqueued;
};
// The route kernel writes every shard's full-length local list numbers (a remove in any-list mode routes nothing), every shard that
// holds an object runs its own call on them (one host thread each, behind a host wait for the route), the tail kernels join the shards'
// answers.  The new plan keeps the owner of every list; its offsets are the new shard objects' own list sizes scattered through the map.
// new_param, flags: the new object's.  d_list_nos: routed if n != 0 and it is not NULL.  shard_call(i, f, base, inv, &new object): shard
// i's own call; f is open on the shard, base is the home block (offsets: B), inv the shard's invalid counter.  tail(base) enqueues the
// tail kernels on the home stream; has_tail: there are any (last_kernel_ms = the route's time + theirs).
template <typename ShardCall, typename Tail>
int update_impl(vidc_ctx *home, const vidc_shards *s, const UpdateNames &nm, int new_param, uint32_t flags, uint64_t n, const int64_t *d_list_nos,
                uint64_t *d_invalid, const UpdateBlocks &B, bool has_tail, ShardCall &&shard_call, Tail &&tail, vidc_shards **out) {
    HostTrace tr(nm.call);
    const ShardPlan &P = s->plan;
    const uint32_t ns = (uint32_t)P.nshards;
    const bool route = n && d_list_nos;
    const std::vector<int> involved = shards_with_objects(s);
    std::unique_ptr<vidc_shards> N(new vidc_shards());
    N->kind = s->kind;
    N->flags = flags;
    N->home = home;
    N->ctxs = s->ctxs;
    N->objs.assign((size_t)ns, nullptr);
    N->param = new_param;
    VIDC_HIP(hipSetDevice(home->device));
    PlanTables tables;
    Scratch blk;
    Pinned h_inv;
    std::vector<FarStage> far((size_t)ns);
    std::vector<std::vector<uint64_t>> sizes((size_t)ns);
    ShardStreamsGuard sguard(s);
    StreamGuard hguard(home, false);
    VIDC_TRY(blk.get(home, B.total));
    VIDC_TRY(h_inv.get(home, (size_t)ns * 8));
    uint8_t *base = blk.as<uint8_t>();
    unsigned long long *sh_inv = blk.as<unsigned long long>();
    hguard.arm();
    EventTimer timer(home);
    VIDC_HIP(hipMemsetAsync(sh_inv, 0, (size_t)ns * 8, home->stream));
    if (B.found_bytes) VIDC_HIP(hipMemsetAsync(base + B.found, 0, B.found_bytes, home->stream));  // (a shard without an object answers nothing)
    double kernel_ms = 0;
    if (route) {
        VIDC_HIP(timer.start());
        hipLaunchKernelGGL(k_shard_route<false>, req_grid(home, n), dim3(256), 0, home->stream, d_list_nos, n, (const uint64_t *)s->d_map.p, P.nlist,
                           ns, (int64_t *)(base + B.local), base + B.owner, (unsigned long long *)d_invalid);
        VIDC_HIP(hipGetLastError());
        VIDC_HIP(timer.mark());
    }
    // every shard's call waits anyway: the route (and the caller's batch) is waited for here, once, before the shard threads start
    VIDC_HIP(vidc_stream_wait(home->stream));
    if (route) kernel_ms = timer.elapsed();
    hguard.disarm();
    tr.mark("routed, waited");
    sguard.which = involved;
    vidc_shards *Np = N.get();
    const int st = involved.empty() ? VIDC_OK : fan_out(involved, [&](int sh) -> int {
        const size_t i = (size_t)sh;
        FarStage &f = far[i];
        VIDC_TRY(f.open(s, sh, B.f_total[i]));
        VIDC_TRY(shard_call(i, f, base, f.counter(sh_inv + i), &Np->objs[i]));
        VIDC_TRY(f.flush());
        VIDC_HIP(vidc_stream_wait(f.c->stream));
        HostTrace ts(nm.a_shard);
        const int rc = codec_list_sizes(s->kind, f.c, Np->objs[i], P.lists[i].size(), sizes[i]);
        ts.mark("list sizes to the host");
        return rc;
    });
    tr.mark(nm.shards_done);
    // (the guard waits for the shard streams -- a failing shard's siblings have finished -- and goes back to the home device)
    if (st != VIDC_OK) return st;  // ~vidc_shards destroys what was built
    VIDC_HIP(hipSetDevice(home->device));
    std::vector<uint64_t> off(P.nlist + 1, 0);
    for (uint64_t l = 0; l < P.nlist; l++) off[l + 1] = off[l] + sizes[(size_t)P.owner[l]][P.local_no[l]];
    N->plan = make_plan_for_owner(off.data(), P.nlist, P.nshards, P.owner);
    tr.mark("plan");
    VIDC_TRY(create_events(N.get()));
    hguard.arm();
    if (has_tail) VIDC_HIP(timer.start());
    VIDC_TRY(tail(base));
    if (has_tail) VIDC_HIP(timer.mark());
    unsigned long long *h = h_inv.as<unsigned long long>();
    VIDC_HIP(hipMemcpyAsync(h, sh_inv, (size_t)ns * 8, hipMemcpyDeviceToHost, home->stream));
    VIDC_TRY(upload_plan(N.get(), tables));
    tr.mark(nm.tail_enqueued);
    VIDC_HIP(vidc_stream_wait(home->stream));
    hguard.disarm();
    tr.mark("waited");
    if (has_tail) kernel_ms += timer.elapsed();
    home->last_kernel_ms = kernel_ms;  // (route + tail)
    for (uint32_t i = 0; i < ns; i++)
        if (h[i]) {  // every local number a shard sees is valid or negative
            set_error("%s: internal error, shard %u counted %llu list numbers outside its lists", nm.call, i, h[i]);
            return VIDC_ERR_INVALID;
        }
    *out = N.release();
    return VIDC_OK;
}

}  // namespace

extern "C" {

int vidc_shards_encode(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, int param, uint32_t flags, uint64_t nlist,
                       const uint64_t *offsets, const uint64_t *d_ids, vidc_shards **out) {
    VIDC_TRY(check_encode(home, nshards, shard_ctxs, kind, offsets, d_ids, nlist, out, false));
    return encode_impl(home, nshards, shard_ctxs, kind, param, flags, nlist, offsets, d_ids, out);
}

int vidc_shards_encode_dev(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, int param, uint32_t flags, uint64_t nlist,
                           const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids, vidc_shards **out) {
    VIDC_TRY(check_encode(home, nshards, shard_ctxs, kind, d_offsets, d_ids, nlist, out, ntotal != 0));
    VIDC_HIP(hipSetDevice(home->device));
    std::vector<uint64_t> off(nlist + 1);
    VIDC_HIP(hipMemcpyAsync(off.data(), d_offsets, (nlist + 1) * 8, hipMemcpyDeviceToHost, home->stream));
    VIDC_HIP(vidc_stream_wait(home->stream));
    if (off[nlist] != ntotal) {
        set_error("shards encode: d_offsets[nlist] = %llu, ntotal = %llu", (unsigned long long)off[nlist], (unsigned long long)ntotal);
        return VIDC_ERR_INVALID;
    }
    return encode_impl(home, nshards, shard_ctxs, kind, param, flags, nlist, off.data(), d_ids, out);
}

void vidc_shards_destroy(vidc_shards *s) { delete s; }

int vidc_shards_count(const vidc_shards *s) { return s ? s->plan.nshards : 0; }
int vidc_shards_kind(const vidc_shards *s) { return s ? s->kind : -1; }
uint64_t vidc_shards_nlist(const vidc_shards *s) { return s ? s->plan.nlist : 0; }
uint64_t vidc_shards_ntotal(const vidc_shards *s) { return s ? s->plan.ntotal : 0; }
uint64_t vidc_shards_compressed_bytes(const vidc_shards *s) {
    uint64_t b = 0;
    if (!s) return 0;
    // (Elias-Fano reports stream BITS / 8: the shards' bits are summed before the division, so that the figure is the unsharded object's)
    for (void *o : s->objs)
        if (o) b += s->kind == VIDC_KIND_EF ? ef_stream_bits((const vidc_ef *)o) : codec_bytes(s->kind, o);
    return s->kind == VIDC_KIND_EF ? b / 8 : b;
}
int vidc_shards_map(const vidc_shards *s, int32_t *owner, uint32_t *local_no) {
    if (!s) return VIDC_ERR_INVALID;
    if (owner) std::copy(s->plan.owner.begin(), s->plan.owner.end(), owner);
    if (local_no) std::copy(s->plan.local_no.begin(), s->plan.local_no.end(), local_no);
    return VIDC_OK;
}
int vidc_shards_offsets(const vidc_shards *s, uint64_t *offsets) {
    if (!s || !offsets) return VIDC_ERR_INVALID;
    std::copy(s->plan.offsets.begin(), s->plan.offsets.end(), offsets);
    return VIDC_OK;
}
const void *vidc_shards_shard(const vidc_shards *s, int i) { return s && i >= 0 && i < s->plan.nshards ? s->objs[(size_t)i] : nullptr; }
vidc_ctx *vidc_shards_shard_ctx(const vidc_shards *s, int i) { return s && i >= 0 && i < s->plan.nshards ? s->ctxs[(size_t)i] : nullptr; }

int vidc_shards_decode_all(vidc_ctx *home, const vidc_shards *s, uint64_t *d_out) {
    VIDC_TRY(check_request(home, s, "shards decode_all"));
    const ShardPlan &P = s->plan;
    if (!P.ntotal) return VIDC_OK;
    if (!d_out) { set_error("shards decode_all: NULL output"); return VIDC_ERR_INVALID; }
    const std::vector<int> involved = shards_with_ids(s);
    std::vector<DecodedIds> dec((size_t)P.nshards);
    ShardStreamsGuard sguard(s);
    StreamGuard hguard(home, false);
    sguard.which = involved;
    // the shards decode concurrently
    VIDC_TRY(fan_out(involved, [&](int sh) -> int {
        const size_t i = (size_t)sh;
        return dec[i].run(s, sh, P.load[i], [&](vidc_ctx *c, uint64_t *dst) { return codec_decode_all(s->kind, c, s->objs[i], dst); });
    }));
    VIDC_HIP(hipSetDevice(home->device));
    hguard.arm();
    EventTimer uncut_timer(home);
    VIDC_HIP(uncut_timer.start());
    for (int sh : involved) {
        const size_t i = (size_t)sh;
        VIDC_TRY(launch_copy<true>(home, dec[i].ids(), d_out, s->d_cut[i].p, s->d_cut_chunks[i].p, s->n_cut_chunks[i]));
    }
    VIDC_TRY(uncut_timer.finish());  // (the call's wait; last_kernel_ms = the inverse cut)
    hguard.disarm();
    return VIDC_OK;
}

int vidc_shards_decode_lists(vidc_ctx *home, const vidc_shards *s, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                             uint64_t *out_offsets) {
    VIDC_TRY(check_request(home, s, "shards decode_lists"));
    if (!m) {
        if (out_offsets) out_offsets[0] = 0;
        return VIDC_OK;
    }
    if (!list_nos || !out_offsets) { set_error("shards decode_lists: NULL array"); return VIDC_ERR_INVALID; }
    const ShardPlan &P = s->plan;
    ListsRoute R;
    uint64_t bad = 0;
    if (!route_lists(P, m, list_nos, R, &bad)) {
        set_error("shards decode_lists: list number %llu (request entry %llu) out of range", (unsigned long long)list_nos[bad], (unsigned long long)bad);
        return VIDC_ERR_INVALID;
    }
    std::copy(R.out_offsets.begin(), R.out_offsets.end(), out_offsets);
    if (!R.out_offsets[m]) return VIDC_OK;
    if (!d_out) { set_error("shards decode_lists: NULL output"); return VIDC_ERR_INVALID; }
    std::vector<int> involved;
    for (int sh = 0; sh < P.nshards; sh++)
        if (R.staged[(size_t)sh]) involved.push_back(sh);
    std::vector<DecodedIds> dec((size_t)P.nshards);
    std::vector<StagedCopy> copies((size_t)P.nshards);
    ShardStreamsGuard sguard(s);
    StreamGuard hguard(home, false);
    sguard.which = involved;
    VIDC_TRY(fan_out(involved, [&](int sh) -> int {
        const size_t i = (size_t)sh;
        std::vector<uint64_t> off(R.local_lists[i].size() + 1);
        return dec[i].run(s, sh, R.staged[i], [&](vidc_ctx *c, uint64_t *dst) {
            return codec_decode_lists(s->kind, c, s->objs[i], R.local_lists[i].size(), R.local_lists[i].data(), dst, off.data());
        });
    }));
    VIDC_HIP(hipSetDevice(home->device));
    hguard.arm();
    for (int sh : involved) VIDC_TRY(staged_copy(home, dec[(size_t)sh].ids(), d_out, R.place[(size_t)sh], copies[(size_t)sh]));
    VIDC_HIP(vidc_stream_wait(home->stream));
    hguard.disarm();
    return VIDC_OK;
}

int vidc_shards_translate_labels_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                     uint64_t *d_invalid) {
    VIDC_TRY(check_request(home, s, "shards translate_labels"));
    if (n && (!d_labels || !d_ids)) { set_error("shards translate_labels: NULL array"); return VIDC_ERR_INVALID; }
    if (!n) return VIDC_OK;
    if (n >= (1ull << 32)) { set_error("shards translate_labels: n must be below 2^32"); return VIDC_ERR_INVALID; }
    const ShardPlan &P = s->plan;
    const uint32_t ns = (uint32_t)P.nshards;
    const std::vector<int> involved = shards_with_objects(s);
    VIDC_HIP(hipSetDevice(home->device));
    const UpdateBlocks B = update_blocks(ns, n, true, true, nullptr, false, true);
    Scratch blk;
    std::vector<FarStage> far((size_t)ns);
    ShardStreamsGuard sguard(s);
    StreamGuard hguard(home, false);
    VIDC_TRY(blk.get(home, B.total));
    unsigned long long *sh_inv = blk.as<unsigned long long>();
    int64_t *local = (int64_t *)(blk.as<uint8_t>() + B.local), *answers = (int64_t *)(blk.as<uint8_t>() + B.answers);
    uint8_t *owner = blk.as<uint8_t>() + B.owner;
    hguard.arm();
    VIDC_HIP(hipMemsetAsync(sh_inv, 0, (size_t)ns * 8, home->stream));
    hipLaunchKernelGGL(k_shard_route<true>, req_grid(home, n), dim3(256), 0, home->stream, d_labels, n, (const uint64_t *)s->d_map.p, P.nlist, ns,
                       local, owner, (unsigned long long *)d_invalid);
    VIDC_HIP(hipGetLastError());
    sguard.which = involved;
    auto shard_call = [&](int sh) -> int {
        const size_t i = (size_t)sh;
        FarStage &f = far[i];
        VIDC_TRY(f.open(s, sh, B.f_total[i]));
        const int64_t *lab = f.in((const int64_t *)local + i * n, B.f_local, n * 8);
        int64_t *ans = f.out(answers + i * n, B.f_answers, n * 8);
        uint64_t *inv = f.counter(sh_inv + i);
        VIDC_TRY(f.st);
        VIDC_TRY(codec_translate(s->kind, f.c, s->objs[i], n, lab, ans, inv));
        return f.flush();
    };
    if (s->kind == VIDC_KIND_ROC) {
        // ROC's translate plans on the host and waits: one thread per shard, behind a host wait for the route
        VIDC_HIP(vidc_stream_wait(home->stream));
        VIDC_TRY(fan_out(involved, [&](int sh) -> int {
            VIDC_TRY(shard_call(sh));
            VIDC_HIP(vidc_stream_wait(s->ctxs[(size_t)sh]->stream));
            return VIDC_OK;
        }));
        VIDC_HIP(hipSetDevice(home->device));
    } else {
        // enqueue-only per-shard calls, from this thread: route -> ev_home -> every shard stream -> ev_shard -> the home stream
        VIDC_HIP(hipEventRecord(s->ev_home, home->stream));
        for (int sh : involved) {
            vidc_ctx *c = s->ctxs[(size_t)sh];
            VIDC_HIP(hipSetDevice(c->device));
            VIDC_HIP(hipStreamWaitEvent(c->stream, s->ev_home, 0));
            const int st = shard_call(sh);
            if (st != VIDC_OK) {
                const std::string msg = vidc_last_error();
                set_error("shard %d: %s", sh, msg.c_str());
                return st;
            }
            VIDC_HIP(hipEventRecord(s->ev_shard[(size_t)sh], c->stream));
        }
        VIDC_HIP(hipSetDevice(home->device));
        for (int sh : involved) VIDC_HIP(hipStreamWaitEvent(home->stream, s->ev_shard[(size_t)sh], 0));
    }
    hipLaunchKernelGGL(k_shard_join, req_grid(home, n), dim3(256), 0, home->stream, (const int64_t *)answers, (const uint8_t *)owner, n, ns, d_ids,
                       (const unsigned long long *)sh_inv, (unsigned long long *)d_invalid);
    VIDC_HIP(hipGetLastError());
    VIDC_HIP(vidc_stream_wait(home->stream));
    hguard.disarm();
    sguard.which.clear();  // (the join waited for every shard stream's event)
    return VIDC_OK;
}

int vidc_shards_decode_gather(vidc_ctx *home, const vidc_shards *s, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                              const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out) {
    VIDC_TRY(check_request(home, s, "shards decode_gather"));
    if (!n_items) return VIDC_OK;
    if (!m || !list_nos || !item_slot || !item_off || !ids_out) { set_error("shards decode_gather: NULL array or no list"); return VIDC_ERR_INVALID; }
    const ShardPlan &P = s->plan;
    GatherRoute R;
    uint64_t bad = 0;
    const int rc = route_gather(P, m, list_nos, n_items, item_slot, item_off, R, &bad);
    if (rc == 1) {
        set_error("decode_gather: list number %llu out of range", (unsigned long long)list_nos[bad]);
        return VIDC_ERR_INVALID;
    }
    if (rc == 2) {
        set_error("decode_gather: item %llu = (slot %llu, offset %llu) is outside its list", (unsigned long long)bad,
                  (unsigned long long)item_slot[bad], (unsigned long long)item_off[bad]);
        return VIDC_ERR_INVALID;
    }
    std::vector<int> involved;
    for (int sh = 0; sh < P.nshards; sh++)
        if (!R.item_index[(size_t)sh].empty()) involved.push_back(sh);
    std::vector<std::vector<int64_t>> got((size_t)P.nshards);
    ShardStreamsGuard sguard(s);
    sguard.which = involved;
    VIDC_TRY(fan_out(involved, [&](int sh) -> int {
        const size_t i = (size_t)sh;
        vidc_ctx *c = s->ctxs[i];
        VIDC_HIP(hipSetDevice(c->device));
        got[i].resize(R.item_index[i].size());
        return codec_decode_gather(s->kind, c, s->objs[i], R.local_lists[i].size(), R.local_lists[i].data(), R.item_index[i].size(),
                                   R.item_slot[i].data(), R.item_off[i].data(), got[i].data());
    }));
    for (int sh : involved) {
        const size_t i = (size_t)sh;
        for (size_t k = 0; k < got[i].size(); k++) ids_out[R.item_index[i][k]] = got[i][k];
    }
    return VIDC_OK;
}

int vidc_sharded_loads(const vidc_shards *s, uint64_t *loads) {
    if (!s || !loads) {
        set_error("sharded loads: NULL object or array");
        return VIDC_ERR_INVALID;
    }
    std::copy(s->plan.load.begin(), s->plan.load.end(), loads);
    return VIDC_OK;
}

// Append (include/vidc.h), through update_impl: every shard appends the pairs whose lists it owns, the join kernel turns the owners'
// labels into global ones.
int vidc_sharded_append_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids, int param,
                            uint32_t flags, vidc_shards **out, int64_t *d_labels, uint64_t *d_invalid) {
    if (out) *out = nullptr;
    if (!home || !s || !out || (n_add && (!d_list_nos || !d_ids))) {
        set_error("sharded append: NULL context, object, out or array");
        return VIDC_ERR_INVALID;
    }
    if (n_add >= 0xffffffffull) { set_error("sharded append: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    VIDC_TRY(check_request(home, s, "sharded append"));
    const uint64_t n = n_add;
    const uint32_t ns = (uint32_t)s->plan.nshards;
    const bool want_labels = n && d_labels;
    const UpdateBlocks B = update_blocks(ns, n, true, want_labels, nullptr, false, true);
    const UpdateNames nm = {"sharded append", "sharded append, a shard", "shards appended, sizes read", "join, tables enqueued"};
    const int new_param = s->kind == VIDC_KIND_EF || (s->kind == VIDC_KIND_PACKED && param == 0) ? s->param : param;
    return update_impl(
        home, s, nm, new_param, flags, n, d_list_nos, d_invalid, B, want_labels,
        [&](size_t i, FarStage &f, uint8_t *base, uint64_t *inv, void **obj) -> int {
            const int64_t *ln = f.in(n ? (const int64_t *)(base + B.local) + i * n : nullptr, B.f_local, n * 8);
            const uint64_t *ids = f.in(n ? d_ids : nullptr, B.f_ids, n * 8);
            int64_t *lab = f.out(want_labels ? (int64_t *)(base + B.answers) + i * n : nullptr, B.f_answers, n * 8);
            VIDC_TRY(f.st);
            return codec_append(s->kind, f.c, s->objs[i], n, ln, ids, param, flags, obj, lab, inv);
        },
        [&](uint8_t *base) -> int {
            if (!want_labels) return VIDC_OK;
            hipLaunchKernelGGL(k_shard_join_labels, req_grid(home, n), dim3(256), 0, home->stream, d_list_nos, (const int64_t *)(base + B.answers),
                               (const uint8_t *)(base + B.owner), n, ns, d_labels);
            VIDC_HIP(hipGetLastError());
            return VIDC_OK;
        },
        out);
}

// Remove (include/vidc.h), through update_impl: pairs mode routes as the append does, any-list mode hands every shard the caller's ids;
// every shard answers with its removed mask in its own decode_all order and one found byte per pair.  The byte inverse cut with the OLD
// plan makes the global mask, the found join the missing count.
int vidc_remove_sharded_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids, int param,
                            uint32_t flags, vidc_shards **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid) {
    if (out) *out = nullptr;
    if (!home || !s || !out || (n_rm && !d_ids)) {
        set_error("sharded remove: NULL context, object, out or id array");
        return VIDC_ERR_INVALID;
    }
    if (n_rm >= 0xffffffffull) { set_error("sharded remove: a batch holds fewer than 2^32 - 1 pairs"); return VIDC_ERR_INVALID; }
    VIDC_TRY(check_request(home, s, "sharded remove"));
    const ShardPlan &P = s->plan;
    const uint64_t n = n_rm;
    const uint32_t ns = (uint32_t)P.nshards;
    const bool pairs = n && d_list_nos, want_found = n && d_missing;
    const UpdateBlocks B = update_blocks(ns, n, pairs, false, d_removed ? P.load.data() : nullptr, want_found, pairs);
    const UpdateNames nm = {"sharded remove", "sharded remove, a shard", "shards removed, sizes read", "mask, join, tables enqueued"};
    return update_impl(
        home, s, nm, s->kind == VIDC_KIND_ROC ? param : s->param, flags, n, d_list_nos, d_invalid, B, (d_removed && P.ntotal) || want_found,
        [&](size_t i, FarStage &f, uint8_t *base, uint64_t *inv, void **obj) -> int {
            const int64_t *ln = f.in(pairs ? (const int64_t *)(base + B.local) + i * n : nullptr, B.f_local, n * 8);
            const uint64_t *ids = f.in(n ? d_ids : nullptr, B.f_ids, n * 8);
            uint8_t *mask = f.out(d_removed ? base + B.mask[i] : nullptr, B.f_mask, P.load[i]);
            uint8_t *fnd = f.out(want_found ? base + B.found + i * n : nullptr, B.f_found, n);
            VIDC_TRY(f.st);
            return codec_remove(s->kind, f.c, s->objs[i], n, ln, ids, param, flags, obj, mask, inv, fnd);
        },
        [&](uint8_t *base) -> int {
            if (d_removed)  // the OLD plan: the masks are in the old shards' decode_all order (a shard without an object has no chunk)
                for (size_t i = 0; i < ns; i++)
                    VIDC_TRY(launch_copy<true>(home, (const uint8_t *)(base + B.mask[i]), d_removed, s->d_cut[i].p, s->d_cut_chunks[i].p, s->n_cut_chunks[i]));
            if (!want_found) return VIDC_OK;
            hipLaunchKernelGGL(k_shard_join_found, req_grid(home, n), dim3(256), 0, home->stream, (const uint8_t *)(base + B.found),
                               (const uint8_t *)(pairs ? base + B.owner : nullptr), n, ns, (unsigned long long *)d_missing);
            VIDC_HIP(hipGetLastError());
            return VIDC_OK;
        },
        out);
}

}  // extern "C"

namespace {

struct RocDelete {
    void operator()(vidc_roc *r) const { vidc_roc_destroy(r); }
};
using RocPtr = std::unique_ptr<vidc_roc, RocDelete>;

// The ROC re-balance: every list's stream moves to its new owner unchanged.  One host thread per new shard that owns lists runs
// vidc_roc_regroup on its context with the old shard objects as sources.  An old shard on another device than the destination is not
// a source as it is: it first regroups the lists bound for that destination into a temporary object on its own context (one host
// thread per such old shard, before the destinations start: a context serves one call at a time), the destination clones the
// temporary object into its own cache (roc_clone_to) and names the clone's lists 0, 1, ... in its table.  That branch has never
// executed: every test machine has one GPU.
int rebalance_roc(vidc_ctx *home, const vidc_shards *s, uint32_t flags, vidc_shards **out) {
    HostTrace tr("sharded rebalance (roc)");
    const ShardPlan &P = s->plan;
    const int ns = P.nshards;
    std::unique_ptr<vidc_shards> N(new vidc_shards());
    N->kind = s->kind;
    N->flags = flags;
    N->home = home;
    N->ctxs = s->ctxs;
    N->objs.assign((size_t)ns, nullptr);
    N->param = s->param;
    N->plan = make_plan(P.offsets.data(), P.nlist, ns);
    const ShardPlan &NP = N->plan;
    std::vector<RegroupRows> rows = regroup_plan(P, NP);
    VIDC_TRY(create_events(N.get()));
    std::vector<int> involved, far_sources;
    for (int d = 0; d < ns; d++)
        if (!NP.lists[(size_t)d].empty()) involved.push_back(d);
    auto near = [&](int k, int d) { return s->ctxs[(size_t)k]->device == s->ctxs[(size_t)d]->device; };
    // far[k][d]: old shard k's lists bound for new shard d, in d's local order (empty: none, or the two share a device)
    std::vector<std::vector<std::vector<uint64_t>>> far((size_t)ns, std::vector<std::vector<uint64_t>>((size_t)ns));
    std::vector<std::vector<RocPtr>> temp((size_t)ns);
    for (int k = 0; k < ns; k++) temp[(size_t)k].resize((size_t)ns);
    for (int d : involved) {
        RegroupRows &R = rows[(size_t)d];
        for (size_t j = 0; j < R.src_no.size(); j++) {
            const int k = (int)R.src_no[j];
            if (near(k, d)) continue;
            std::vector<uint64_t> &f = far[(size_t)k][(size_t)d];
            f.push_back(R.list_no[j]);
            R.list_no[j] = f.size() - 1;  // (its number in the temporary object)
        }
    }
    for (int k = 0; k < ns; k++)
        for (int d = 0; d < ns; d++)
            if (!far[(size_t)k][(size_t)d].empty() && (far_sources.empty() || far_sources.back() != k)) far_sources.push_back(k);
    ShardStreamsGuard sguard(s);
    if (!far_sources.empty()) {
        sguard.which = far_sources;
        VIDC_TRY(fan_out(far_sources, [&](int k) -> int {
            const size_t i = (size_t)k;
            vidc_ctx *c = s->ctxs[i];
            VIDC_HIP(hipSetDevice(c->device));
            const vidc_roc *src = (const vidc_roc *)s->objs[i];
            for (int d = 0; d < ns; d++) {
                const std::vector<uint64_t> &f = far[i][(size_t)d];
                if (f.empty()) continue;
                const std::vector<uint32_t> zeros(f.size(), 0u);
                vidc_roc *t = nullptr;
                VIDC_TRY(vidc_roc_regroup(c, 1, &src, f.size(), zeros.data(), f.data(), 0u, &t));
                temp[i][(size_t)d].reset(t);
            }
            return VIDC_OK;
        }));
        tr.mark("far sources regrouped");
    }
    sguard.which = involved;
    vidc_shards *Np = N.get();
    const int st = involved.empty() ? VIDC_OK : fan_out(involved, [&](int d) -> int {
        const size_t i = (size_t)d;
        vidc_ctx *c = Np->ctxs[i];
        VIDC_HIP(hipSetDevice(c->device));
        const vidc_roc *srcs[VIDC_SHARDS_MAX] = {};
        RocPtr clones[VIDC_SHARDS_MAX];
        for (int k = 0; k < ns; k++) {
            if (near(k, d)) {
                srcs[k] = (const vidc_roc *)s->objs[(size_t)k];  // (NULL for a shard without lists: no row names it)
            } else if (temp[(size_t)k][i]) {
                vidc_roc *cl = nullptr;
                VIDC_TRY(roc_clone_to(c, temp[(size_t)k][i].get(), &cl));
                clones[k].reset(cl);
                srcs[k] = cl;
            }
        }
        const RegroupRows &R = rows[i];
        return vidc_roc_regroup(c, ns, srcs, R.src_no.size(), R.src_no.data(), R.list_no.data(), flags & VIDC_ROC_WANT_PERM,
                                (vidc_roc **)&Np->objs[i]);
    });
    tr.mark("shards regrouped");
    // (the guard waits for the shard streams -- a failing shard's siblings have finished -- and goes back to the home device)
    if (st != VIDC_OK) return st;  // ~vidc_shards destroys what was built
    VIDC_HIP(hipSetDevice(home->device));
    PlanTables tables;
    StreamGuard hguard(home);
    VIDC_TRY(upload_plan(N.get(), tables));
    VIDC_HIP(vidc_stream_wait(home->stream));
    hguard.disarm();
    // no kernel runs on the home stream; a home context that is also a shard context keeps its regroup's time
    if (std::find(s->ctxs.begin(), s->ctxs.end(), home) == s->ctxs.end()) home->last_kernel_ms = 0;
    *out = N.release();
    return VIDC_OK;
}

// Packed bits and Elias-Fano: decode_all into a block of the home cache, then the encoder's body on the object's own offsets -- the new
// map is the one make_plan chooses there, and a shard is what the single-object encoder builds from its cut.
int rebalance_rebuild(vidc_ctx *home, const vidc_shards *s, uint32_t flags, vidc_shards **out) {
    const ShardPlan &P = s->plan;
    VIDC_HIP(hipSetDevice(home->device));
    Scratch ids;
    VIDC_TRY(ids.get(home, (P.ntotal ? P.ntotal : 2) * 8));
    VIDC_TRY(vidc_shards_decode_all(home, s, ids.as<uint64_t>()));  // (waits)
    return encode_impl(home, P.nshards, s->ctxs.data(), s->kind, s->param, flags, P.nlist, P.offsets.data(), ids.as<uint64_t>(), out);
}

}  // namespace

extern "C" {

// Re-balance (include/vidc.h): the new map is make_plan's on the object's own offsets; moved_ids is host arithmetic on the two maps.
int vidc_rebalance_sharded(vidc_ctx *home, const vidc_shards *s, uint32_t flags, vidc_shards **out, uint64_t *moved_ids) {
    if (out) *out = nullptr;
    if (!home || !s || !out) {
        set_error("sharded rebalance: NULL context, object or out");
        return VIDC_ERR_INVALID;
    }
    VIDC_TRY(check_request(home, s, "sharded rebalance"));
    VIDC_TRY(s->kind == VIDC_KIND_ROC ? rebalance_roc(home, s, flags, out) : rebalance_rebuild(home, s, flags, out));
    if (moved_ids) *moved_ids = shardplan::moved_ids(s->plan, (*out)->plan);
    return VIDC_OK;
}

int vidc_shards_perm(vidc_ctx *home, const vidc_shards *s, uint32_t *perm_host) {
    VIDC_TRY(check_request(home, s, "shards perm"));
    const bool has = (s->kind == VIDC_KIND_ROC && (s->flags & VIDC_ROC_WANT_PERM)) || (s->kind == VIDC_KIND_EF && (s->flags & VIDC_EF_WANT_PERM));
    if (!has) { set_error("shards perm: the object was built without a permutation"); return VIDC_ERR_INVALID; }
    const ShardPlan &P = s->plan;
    if (!P.ntotal) return VIDC_OK;
    if (!perm_host) { set_error("shards perm: NULL output"); return VIDC_ERR_INVALID; }
    const std::vector<int> involved = shards_with_ids(s);
    ShardStreamsGuard sguard(s);
    sguard.which = involved;
    // a list's entries are positions inside the list: the shards' permutations go to their lists' places unchanged
    return fan_out(involved, [&](int sh) -> int {
        const size_t i = (size_t)sh;
        vidc_ctx *c = s->ctxs[i];
        VIDC_HIP(hipSetDevice(c->device));
        std::vector<uint32_t> p(P.load[i]);
        VIDC_TRY(s->kind == VIDC_KIND_ROC ? vidc_roc_perm(c, (const vidc_roc *)s->objs[i], p.data()) : vidc_ef_perm(c, (const vidc_ef *)s->objs[i], p.data()));
        for (const Segment &sg : P.cut[i]) std::copy(p.begin() + (ptrdiff_t)sg.dst_start, p.begin() + (ptrdiff_t)(sg.dst_start + sg.count), perm_host + sg.src_start);
        return VIDC_OK;
    });
}

}  // extern "C"
