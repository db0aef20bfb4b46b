// roc_dec_plan.h -- the planning half of the ROC decoder's host call (roc.hip: plan_decode / decode_impl): which kernel class takes
// which work item, in which order, where every item's scratch and member slots lie, and which hardware queue runs which class.  Host
// code only, no HIP include, nothing that touches a stream, no getenv: tests/roc_dec_plan_test.cpp builds it with g++.  roc.hip fills
// DecLimits from the kernel headers' macros and DecPolicy from the environment and the context, at the points where it always read
// them.  The sizes of an item's scratch and slots are the kernels' own (roc_sizing.h).
#pragma once
#include "roc_enc_plan.h"
#include "roc_sizing.h"

namespace vidc {

// work items grouped by kernel class, each with private scratch
// general decoder classes by LDS footprint of the fine prefix rows (2^fb u32, fb = lg(n) - 3): occupancy, not
// arithmetic, bounds the general decoder when a batch has many mid-size lists
// (DC_LANE .. the last class: kernels that may hand a list back with VIDC_ST_RETRY)
enum DecClass { DC_TINY = 0, DC_U18, DC_U20, DC_GSMALL, DC_G8K, DC_G16K, DC_GMID, DC_GHUGE, DC_LANE, DC_LANE64, DC_LANE128, DC_B2, DC_B2T, DC_B2S, DC_B2L, DC_B2M,
                DC_GRP0, DC_GRP2, DC_GRP3, DC_GRP4,   // row-per-list decoder by bucket bits 8 + F (roc_grp.h)
                DC_LANEP, DC_LANEQ, DC_COUNT };        // 257..512 / 513..1024 ids on a pair / quad of lanes, ids in registers (k_roc_decode_lane_reg<.., 2 / 4>)
// the classes' names in VIDC_DEC_SCHED
constexpr const char *DEC_CLASS_NAMES[DC_COUNT] = {"TINY", "U18", "U20", "GSMALL", "G8K", "G16K", "GMID", "GHUGE", "LANE", "LANE64", "LANE128", "B2", "B2T", "B2S",
                                                   "B2L", "B2M", "GRP0", "GRP2", "GRP3", "GRP4", "LANEP", "LANEQ"};
inline int dec_class_by_name(const std::string &t) {
    for (int c = 0; c < DC_COUNT; c++) if (t == DEC_CLASS_NAMES[c]) return c;
    return -1;
}
// class boundaries and caps that belong to no kernel header
constexpr uint64_t DEC_G8K_MAX = 8192, DEC_G16K_MAX = 16384, DEC_GMID_MAX = 32768;
constexpr uint64_t B2_MIN_LIST = 4096, B2_MAX_LIST = 98304;
constexpr size_t B2_CAP = 1024;      // chains of k_roc_decode_b2 per call (four per CU of an MI355X: 1 MiB of member rows each)
constexpr size_t B2_TOP_CAP = 5120;  // ... of a call with more long chains than that: every list beyond 16 384 ids (comment at promote_b2)

// gen_small_max: decoder, fb <= 9 -> 2 KiB of LDS (full occupancy)
struct DecLimits {
    uint64_t tiny_max, gen_small_max, u_min_list, r2_min_list, lane_reg_max, lane_pair_max, lane_quad_max, lane_max, lane_max128, lane_max64,
             b2l_max_list, b2l_mid_list, b2l_load, lane_min_lists, lane_min_lists64, lane_min_tiny;
};
// The switches a plan reads (the environment is read once per plan, not once per list: three getenv per list were 1 ms of a
// 65 536-list plan).  The per-call arguments of plan_decode (only_general, allow_lane) are already folded into f_general / lpol.
// (256 buckets for the 257..1024-id lists too, 128 buckets for the bucket-row lists of up to 1024 ids: measured no better, HISTORY.md)
struct DecPolicy {
    bool f_general = false, wide = false, no_length_classes = false, old_u = false, no_r2 = false;
    LanePolicy lpol = LANE_AUTO;
    GrpPolicy gpol{};
    bool pair = true;    // lists of pair_min+1 .. 512 ids: the register decoder on lane pairs (VIDC_NO_LANE_PAIR=1: the bucket-row decoder)
    // VIDC_PAIR_MIN=n (64 .. 256): lists of n+1 .. 256 ids on lane pairs too -- 32 lists per wavefront, i.e. two wavefronts
    // per SIMD where a call of 65 536 lists has one (measurements: DESIGN section 12)
    uint64_t pair_min = 256;
    // quads of lanes for 513..1024 ids: opt-in.  Measured slower than the bucket rows: 65 536 x 1024 ids decode in 5.6 instead of
    // 4.1 ms -- 16 lists per 256-VGPR wavefront means two rounds of wavefronts per SIMD --, S2 84 instead of 78 ms
    bool quad = false;
    bool nb128 = true;   // lists of 1025..2048 ids on 128 buckets (VIDC_NO_LANE128=1: 256, as before round 4)
    uint32_t lane_align = 16;  // VIDC_LANE_ALIGN=4 / 16: bucket rows of the lane decoders on 16- / 64-byte boundaries
};
// what the planner reads of the compressed object.  umax: the HEURISTIC maxima (n_umax of them; 0 = unknown); nwords: null while the
// word counts are not on the host; order_desc: every list longest first (n_order of them), where the encoder built that order
struct DecView {
    const uint64_t *offsets = nullptr;
    const uint32_t *prec = nullptr, *umax = nullptr;
    size_t n_umax = 0;
    const uint32_t *nwords = nullptr;
    const uint32_t *order_desc = nullptr;
    size_t n_order = 0;
    uint64_t order_max_n = 0;
};
struct DecPlan {
    std::vector<uint32_t> wl;        // list numbers, grouped by class, longest first inside a class
    std::vector<uint32_t> item;      // index of each work item in the caller's request
    size_t count[DC_COUNT] = {};
    uint64_t sum_n[DC_COUNT] = {}, max_n[DC_COUNT] = {};
    std::vector<uint64_t> scratch_off, slots_off;
    uint64_t scratch_words = 0, slots_words = 0;
    bool lean = false;               // graph rows, lane decoder: item k == request k, no scratch / offset arrays
    bool tiny_lane = false;          // DC_TINY items run on the lane-per-list kernel
    bool gsmall_lrows = false;       // DC_GSMALL items keep their member rows in LDS (33 KiB each: only for few lists)
    uint32_t lane_align = 4;         // slots a bucket row of the lane decoders is aligned / padded to (roc_lane_cap_nb)
    uint64_t implicit = 0;           // lean plan without a work list: items are rows 0..implicit-1
    const uint32_t *order_dev = nullptr;  // ... or every row of the object in this device-resident order, each to its OWN output row
    bool order_build = false;        // ... which this call builds first (k_rows_order_*, inside the call's timed region)
    bool order_req = false;          // ... or order_dev is a work list in request order: item k -> output row k (device node requests)
};
// the work items of every class while a plan is built: indices into the caller's request
struct DecWorkLists { std::vector<uint32_t> cls[DC_COUNT]; };

inline DecClass grp_dec_class(uint64_t n) {
    const uint32_t f = dev::roc_grp_dec_fbits((uint32_t)n);
    return f == 0 ? DC_GRP0 : (f == 2 ? DC_GRP2 : (f == 3 ? DC_GRP3 : DC_GRP4));
}
// Kernel families of a call, from its class sizes (the encoder's rule, enc_families): lane / lane64 the mid-size policies, tiny_lane
// the tiny class on the lane-per-list kernel, grp the row-per-list kernels.
struct DecUse { bool lane = false, lane64 = false, tiny_lane = false, grp = false; };
struct DecCounts { uint64_t tiny = 0, mid = 0, mid64 = 0, grp = 0; };
// wide: the context that will run the plan has a stream per kernel class (8 hardware queues): the row-per-list kernels are only
// planned then, like the encoder only takes them then (their octaves must overlap)
inline DecUse dec_families(const DecCounts &n, bool rows_flavour, uint64_t nlists, bool allow_b2, const DecPolicy &p, const DecLimits &lim) {
    DecUse u;
    u.grp = allow_b2 && !p.f_general && !rows_flavour && n.grp && n.grp >= p.gpol.min_lists && (p.wide || p.gpol.min_lists == 0);
    u.lane = lane_wanted(p.lpol, n.mid, lim.lane_min_lists);
    u.lane64 = lane_wanted(p.lpol, n.mid64, lim.lane_min_lists64);
    u.tiny_lane = lane_wanted(p.lpol, rows_flavour ? nlists : n.tiny, lim.lane_min_tiny);
    return u;
}
// The class of a list of n ids with precision P: the one cascade.
inline DecClass dec_class(uint64_t n, uint32_t P, const DecUse &use, const DecPolicy &p, const DecLimits &lim) {
    if (n <= lim.tiny_max) return DC_TINY;
    const bool grp_ok = use.grp && n >= p.gpol.dec_min_n && n <= p.gpol.dec_max_n && P <= 32;
    if (grp_ok && p.gpol.min_lists == 0) return grp_dec_class(n);  // VIDC_FORCE_GRP: ahead of every other family
    if (!p.f_general && n >= lim.u_min_list) {
        if (P <= 18) return DC_U18;
        if (P <= 20) return DC_U20;
    }
    if (grp_ok) return grp_dec_class(n);
    if (use.lane && p.pair && n > p.pair_min && n <= lim.lane_pair_max) return DC_LANEP;
    if (use.lane && p.quad && n > lim.lane_pair_max && n <= lim.lane_quad_max) return DC_LANEQ;
    if (use.lane && n <= lim.lane_max) return DC_LANE;
    if (use.lane64 && p.nb128 && n > lim.lane_max && n <= lim.lane_max128) return DC_LANE128;
    if (use.lane64 && n > lim.lane_max && n <= lim.lane_max64) return DC_LANE64;
    if (n <= lim.gen_small_max) return DC_GSMALL;
    if (n <= DEC_G8K_MAX) return DC_G8K;
    if (n <= DEC_G16K_MAX) return DC_G16K;
    if (n <= DEC_GMID_MAX) return DC_GMID;
    return DC_GHUGE;
}

// The by-length route.  The whole object (`lists` is 0 .. nlist-1), no list beyond the lane classes, and the encoder left its lists
// ordered by length (v.order_desc): the class of a list is a function of its length (dec_class looks at the precision only for
// lists of more than 4096 ids), so every class is one or two runs of that order, cut out between binary searches at the upper ends
// of the intervals on which dec_class is constant.  Replaces three passes over the lists (counts, classification with a push_back
// per list, sortedness) of a 65 536-list plan.  False (and `w` untouched) where the route does not apply: a family that some list
// needs is not wanted, or the row-per-list kernels are in reach.  The tiny class comes back in request order, like the per-list loop's.
inline bool classify_dec_by_length(const DecView &v, size_t nlists, bool allow_b2, const DecPolicy &p, const DecLimits &lim, DecUse &use,
                                   DecWorkLists &w) {
    if (p.f_general || p.no_length_classes || v.n_order != nlists || v.order_max_n > lim.lane_max64) return false;
    const uint32_t *order = v.order_desc;
    const size_t nl = nlists;
    auto first_le = [&](uint64_t bound) {  // first position of the order whose list has at most `bound` ids
        size_t lo = 0, hi = nl;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (v.offsets[order[mid] + 1] - v.offsets[order[mid]] > bound) lo = mid + 1; else hi = mid; }
        return lo;
    };
    const size_t e_lane = first_le(lim.lane_max), e_tiny = first_le(lim.tiny_max);
    DecCounts n;
    n.mid64 = e_lane; n.mid = e_tiny - e_lane; n.tiny = nl - e_tiny;
    const DecUse u = dec_families(n, false, nl, false, p, lim);
    const bool grp_in_reach = allow_b2 && p.gpol.dec_min_n <= v.order_max_n && p.gpol.min_lists != ~0ull;  // (VIDC_FORCE_GRP / VIDC_GRP_DEC_MINN)
    if (!((u.lane || !n.mid) && (u.lane64 || !n.mid64)) || grp_in_reach) return false;
    use = u;
    uint64_t cuts[] = {lim.lane_max64, lim.lane_max128, lim.lane_max, lim.lane_quad_max, lim.lane_pair_max, p.pair_min, lim.tiny_max};
    std::sort(std::begin(cuts), std::end(cuts), std::greater<uint64_t>());
    const size_t ncuts = sizeof(cuts) / sizeof(cuts[0]);
    size_t pos = 0;
    for (size_t c = 0; c < ncuts && pos < nl; c++) {
        const uint64_t hi = cuts[c], lo = c + 1 < ncuts ? cuts[c + 1] : 0;  // interval (lo, hi]
        if (hi == lo) continue;
        const size_t end = !lo ? nl : lo == lim.lane_max ? e_lane : lo == lim.tiny_max ? e_tiny : first_le(lo);  // (the last interval also takes the empty lists)
        if (end > pos) {
            std::vector<uint32_t> &dst = w.cls[dec_class(hi, 0, u, p, lim)];
            dst.insert(dst.end(), order + pos, order + end);
            pos = end;
        }
    }
    std::vector<uint32_t> &tiny = w.cls[DC_TINY];
    if (tiny.size() == nl) std::iota(tiny.begin(), tiny.end(), 0u);
    else std::sort(tiny.begin(), tiny.end());
    return true;
}

// a class longest first: counting sort by length (stable); nothing to do for equal-sized lists or a class that came longest first
template <class Len>
inline void sort_class_desc(std::vector<uint32_t> &items, Len &&len) {
    if (items.size() < 2) return;
    uint64_t maxlen = 0, prev = ~0ull;
    bool sorted_already = true;
    for (uint32_t i : items) {
        const uint64_t n = len(i);
        maxlen = std::max<uint64_t>(maxlen, n);
        sorted_already &= n <= prev;
        prev = n;
    }
    if (sorted_already) return;
    std::vector<uint32_t> start(maxlen + 2, 0), sorted(items.size());
    for (uint32_t i : items) start[maxlen - len(i) + 1]++;
    for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
    for (uint32_t i : items) sorted[start[maxlen - len(i)]++] = i;
    items.swap(sorted);
}
// The per-list route: counts, families, one dec_class per work item, every class but the tiny one longest first.
// lists[i] = list number of request item i (a list may appear more than once).  rows_flavour: every item is a tiny one.
inline void classify_dec_per_list(const DecView &v, const std::vector<uint32_t> &lists, bool rows_flavour, bool allow_b2, const DecPolicy &p,
                                  const DecLimits &lim, DecUse &use, DecWorkLists &w) {
    DecCounts cnt;
    for (uint32_t l : lists) {
        const uint64_t n = v.offsets[l + 1] - v.offsets[l];
        cnt.tiny += n <= lim.tiny_max;
        cnt.mid += n > lim.tiny_max && n <= lim.lane_max;
        cnt.mid64 += n > lim.lane_max && n <= lim.lane_max64;
        cnt.grp += n >= p.gpol.dec_min_n && n <= p.gpol.dec_max_n;
    }
    use = dec_families(cnt, rows_flavour, lists.size(), allow_b2, p, lim);
    // (the classes that can hold most lists of a big call grow once, not by doubling)
    if (lists.size() >= 4096) for (int c : {(int)DC_TINY, (int)DC_LANE, (int)DC_GSMALL}) w.cls[c].reserve(lists.size());
    for (uint32_t i = 0; i < lists.size(); i++) {
        const uint32_t l = lists[i];
        w.cls[rows_flavour ? DC_TINY : dec_class(v.offsets[l + 1] - v.offsets[l], v.prec[l], use, p, lim)].push_back(i);
    }
    auto len = [&](uint32_t i) { return v.offsets[lists[i] + 1] - v.offsets[lists[i]]; };
    for (int c = 0; c < DC_COUNT; c++)
        if (c != DC_TINY) sort_class_desc(w.cls[c], len);
}

// buckets of k_roc_decode_b2<32 .. 256> for a short list (r2_min_list < n <= b2l_max_list), or 0: the bucket count follows the
// expected load -- ids are spread over (max id >> shift) + 1 buckets, half of them in the worst case when the maximum is unknown
// (imported streams); at <= b2l_load ids per bucket a 64-member row practically never overflows
inline uint32_t b2_buckets_for(uint64_t n, uint32_t P, uint32_t umax, const DecLimits &lim) {
    if (n <= lim.r2_min_list || n > lim.b2l_max_list || P > 31) return 0u;
    for (uint32_t bk : {32u, 64u, 128u, 256u}) {
        const uint32_t bbits = bk == 32u ? 5u : (bk == 64u ? 6u : (bk == 128u ? 7u : 8u)), bsh = P > bbits ? P - bbits : 0u;
        const uint32_t mx = umax ? umax : ((P ? (1u << (P - 1u)) : 1u));
        const uint64_t eff = std::min<uint64_t>(bk, (uint64_t)(mx >> bsh) + 1u);
        if (n <= lim.b2l_load * eff) return bk;
    }
    return 0u;
}
// The longest general chains (precision above 20 bits) take k_roc_decode_b2 under the rule of the encoder's
// k_roc_encode_r2: only when every chain at least half as long as the longest one gets it (<= B2_CAP of them).
// (the general classes of `w` are sorted longest first)
inline void promote_b2(DecWorkLists &w, const DecView &v, const std::vector<uint32_t> &lists, const DecPolicy &p, const DecLimits &lim) {
    if (p.f_general || p.old_u || p.no_r2) return;
    std::vector<uint32_t> *cls = w.cls;
    auto len = [&](uint32_t i) { return v.offsets[lists[i] + 1] - v.offsets[lists[i]]; };
    const int order_[4] = {DC_GHUGE, DC_GMID, DC_G16K, DC_G8K};
    uint64_t n_top = 0;
    for (int c : order_)
        if (!cls[c].empty()) { n_top = len(cls[c][0]); break; }
    size_t n_long = 0;
    bool stop = false;
    for (int c : order_) {
        for (uint32_t i : cls[c]) {
            if (2 * len(i) < n_top || n_long > B2_CAP) { stop = true; break; }
            n_long++;
        }
        if (stop) break;
    }
    size_t b2_cap = B2_CAP;
    // More long chains than the cap (S2: 1754 lists of 32 769..65 536 ids and 2666 of 16 385..32 768): round 3 gave the `cap`
    // longest ones to this kernel and left the rest on the general decoder, whose step under load is ~1.1 us against ~0.65
    // here.  Measured in round 4 (S2 decode, kernels): 1024 chains 77-79 ms, all 1754 lists beyond 32 768 ids 74, these and
    // the 2666 lists of 16 385..32 768 ids 71-73; the lists of 8193..16 384 ids too (instead of the row-per-list kernel): 80-90.
    // So every list beyond 16 384 ids takes it, up to B2_TOP_CAP chains (20 per CU of an MI355X: 8 KiB of LDS each).
    const bool top_only = n_top && n_long > b2_cap;
    if (top_only) b2_cap = B2_TOP_CAP;
    if (n_top && (n_long <= b2_cap || top_only))
        for (int c : order_) {  // longest first; a list that does not qualify stays where it is
            if (top_only && c != DC_GHUGE && c != DC_GMID) break;
            std::vector<uint32_t> keep;
            for (uint32_t i : cls[c]) {
                const uint32_t P = v.prec[lists[i]];
                // (beyond ~100 000 ids a 64-member row overflows too often: average bucket load n / 4096)
                // (shorter than B2_MIN_LIST: the general decoder keeps the member rows of such a list in LDS, while 1 MiB of
                // sparse rows per list -- 1 GiB for a thousand lists -- makes every step of this kernel an HBM miss:
                // 1024 x 977 ids decoded in 0.53 instead of 0.50 ms)
                if (cls[DC_B2].size() < b2_cap && len(i) <= B2_MAX_LIST && len(i) > B2_MIN_LIST && P >= 12 && P <= 31) cls[DC_B2].push_back(i);
                else keep.push_back(i);
            }
            cls[c].swap(keep);
        }
    // short lists (257..4096 ids) of a call with few lists: the same loop with 32 .. 256 buckets and their 64-member rows in
    // LDS (8.3 / 16.5 / 33 / 66 KiB per chain) -- if the chains taken so far and all of these fit at 150 KiB of LDS and 16
    // wavefronts (128 VGPRs each) per CU: 1024 chains of 33 KiB, 4096 of 8.3 KiB on 256 CUs.
    auto buckets_for = [&](uint32_t i) {
        const uint32_t l = lists[i];
        return b2_buckets_for(len(i), v.prec[l], l < v.n_umax ? v.umax[l] : 0u, lim);
    };
    size_t units = 0, n_el = 0;  // (units of 8.25 KiB of LDS: 18 per CU; a chain with its rows in memory takes one)
    bool longer_left = false;   // a longer chain that stays on the general kernel decides the call anyway
    for (int c : order_) longer_left |= !cls[c].empty();
    for (uint32_t i : cls[DC_GSMALL]) {
        const uint32_t bk = buckets_for(i);
        units += bk / 32u;
        n_el += bk != 0;
        longer_left |= !bk && len(i) > lim.b2l_mid_list;
    }
    if (n_el && !longer_left && cls[DC_B2].size() + units <= b2_cap * 9 / 2 && cls[DC_B2].size() + n_el <= b2_cap * 4) {
        std::vector<uint32_t> keep;
        for (uint32_t i : cls[DC_GSMALL]) {
            const uint32_t bk = buckets_for(i);
            if (bk == 32u) cls[DC_B2T].push_back(i);
            else if (bk == 64u) cls[DC_B2S].push_back(i);
            else if (bk == 128u) cls[DC_B2L].push_back(i);
            else if (bk == 256u) cls[DC_B2M].push_back(i);
            else keep.push_back(i);
        }
        cls[DC_GSMALL].swap(keep);
    }
}

// words of member slots that one item of class c takes, and what its slot range is aligned to (0: the item has no slots and its
// slot offset is 0)
struct DecSlots { uint64_t words, align; };
inline DecSlots dec_item_slots(int c, uint64_t n, uint32_t P, bool gsmall_lrows, uint32_t lane_align) {
    switch (c) {
        case DC_LANEP: case DC_LANEQ: return {0, 0};  // no scratch of any kind
        case DC_LANE: return {64ull * dev::roc_lane_cap_nb<64>((uint32_t)n, lane_align), lane_align};  // rows are read as uint4
        case DC_LANE64: return {256ull * dev::roc_lane_cap_nb<256>((uint32_t)n, lane_align), lane_align};
        case DC_LANE128: return {128ull * dev::roc_lane_cap_nb<128>((uint32_t)n, lane_align), lane_align};
        case DC_GRP0: case DC_GRP2: case DC_GRP3: case DC_GRP4: return {dev::roc_grp_dec_slots((uint32_t)n), 16};  // member rows of 32 .. 96 u32: 64-byte aligned
        case DC_U18: case DC_U20: return {n, 1};  // duplicate side list
        case DC_B2: return {4096ull * 64ull, 64};  // 4096 rows of 64 members
        case DC_GSMALL: if (gsmall_lrows) return {n, 1};  // overflow list only: the member rows are in LDS
            [[fallthrough]];
        case DC_G8K: case DC_G16K: case DC_GMID: case DC_GHUGE:
            return {((uint64_t)1 << dev::roc_dec_fine_bits((uint32_t)n, P > 32 ? 32 : P)) * dev::roc_dec_cap((uint32_t)n) + n, 1};
        default: return {0, 1};  // DC_TINY, DC_B2T .. DC_B2M: everything in registers / LDS
    }
}
// One pass per class over its work items: work list, per-class totals, scratch / slot offsets (65 536 lists: the two passes with
// push_back this replaces were half of the planner's time).  p.wl / item / scratch_off / slots_off are the caller's (pooled) vectors.
inline void dec_layout(const DecWorkLists &w, const DecView &v, const std::vector<uint32_t> &lists, uint32_t lane_align, DecPlan &p) {
    // LDS member rows for the short general lists only while all of them are resident at four per CU: beyond that the 33 KiB
    // per wavefront cost more in occupancy than the global rows cost in traffic (6000 x 300 ids: 0.86 vs 0.3 ms)
    p.gsmall_lrows = w.cls[DC_GSMALL].size() <= B2_CAP;
    p.lane_align = lane_align;
    size_t total_items = 0;
    for (int c = 0; c < DC_COUNT; c++) total_items += w.cls[c].size();
    p.item.resize(total_items); p.wl.resize(total_items); p.scratch_off.resize(total_items); p.slots_off.resize(total_items);
    uint64_t so = 0, sl = 0;
    size_t k = 0;
    for (int c = 0; c < DC_COUNT; c++) {
        p.count[c] = w.cls[c].size();
        uint64_t sum_n = 0, max_n = 0;
        // re-spill scratch of the decoder stack (roc_dec_stack_cap); the lane-per-list decoders keep what they push in LDS
        const bool stack_scratch = c != DC_LANE && c != DC_LANE64 && c != DC_LANE128 && c < DC_GRP0;
        for (const uint32_t i : w.cls[c]) {
            const uint32_t l = lists[i];
            const uint64_t n = v.offsets[l + 1] - v.offsets[l];
            p.item[k] = i;
            p.wl[k] = l;
            sum_n += n;
            max_n = std::max(max_n, n);
            p.scratch_off[k] = so;
            if (stack_scratch) so += dev::roc_dec_stack_cap((uint32_t)n, v.nwords ? v.nwords[l] : 0u);
            const DecSlots s = dec_item_slots(c, n, v.prec[l], p.gsmall_lrows, lane_align);
            if (s.align > 1) sl = (sl + s.align - 1) & ~(s.align - 1);
            p.slots_off[k] = s.align ? sl : 0;
            sl += s.words;
            k++;
        }
        p.sum_n[c] = sum_n;
        p.max_n[c] = max_n;
    }
    p.scratch_words = so;
    p.slots_words = sl;
}

// graph rows with the lane-per-row decoder: request order, no scratch, implicit output offsets
inline bool plan_decode_lean(const std::vector<uint32_t> &lists, bool rows_flavour, const DecPolicy &p, const DecLimits &lim, DecPlan &out) {
    out.wl.clear(); out.item.clear(); out.scratch_off.clear(); out.slots_off.clear();
    out.scratch_words = 0; out.slots_words = 0;
    for (int c = 0; c < DC_COUNT; c++) { out.count[c] = 0; out.sum_n[c] = 0; out.max_n[c] = 0; }
    out.tiny_lane = out.lean = rows_flavour && lane_wanted(p.lpol, lists.size(), lim.lane_min_tiny);
    if (!out.lean) return false;
    out.wl = lists;
    out.count[DC_TINY] = lists.size();
    return true;
}
// The plan of every other call (after plan_decode_lean said no): classes, promotion, layout.  whole_sorted: `lists` is 0 .. nlist-1
// and v.order_desc holds the same lists longest first.  allow_b2: the chain and row-per-list kernels may be planned.
inline void plan_decode_classes(const DecView &v, const std::vector<uint32_t> &lists, bool rows_flavour, bool allow_b2, bool whole_sorted,
                                const DecPolicy &p, const DecLimits &lim, DecPlan &out) {
    DecWorkLists w;
    DecUse use;
    if (!(whole_sorted && !rows_flavour && classify_dec_by_length(v, lists.size(), allow_b2, p, lim, use, w)))
        classify_dec_per_list(v, lists, rows_flavour, allow_b2, p, lim, use, w);
    out.tiny_lane = use.tiny_lane;
    if (allow_b2 && !rows_flavour) promote_b2(w, v, lists, p, lim);
    dec_layout(w, v, lists, p.lane_align, out);
}

// Stream assignment: a class's kernel lasts about max(its longest chain, its share of the machine); classes are taken longest
// first (order[]) and each goes to the queue that frees up first (LPT over nq queues; queue_of[c], -1 for a class without items).
// A fixed assignment left three general classes back to back on one stream on S2 (70 + 45 + 18 ms) while the others had drained.
// (the lane-pair class first and alone on the caller's stream: measured no better, HISTORY.md)
constexpr int DEC_MAX_QUEUES = 32;
inline void dec_assign_queues(const size_t *count, const uint64_t *sum_n, const uint64_t *max_n, int nq, int *order, int *queue_of) {
    double est[DC_COUNT];
    for (int c = 0; c < DC_COUNT; c++) {
        order[c] = c;
        queue_of[c] = -1;
        const bool u = c == DC_U18 || c == DC_U20 || c == DC_B2 || c == DC_B2T || c == DC_B2S || c == DC_B2L || c == DC_B2M, lane = c == DC_LANE || c == DC_LANE64 || c == DC_LANE128 || c == DC_LANEP || c == DC_LANEQ;
        const bool grpc = c >= DC_GRP0 && c <= DC_GRP4;
        // (constants fitted to the S2 timeline: general kernels ~2.5 G steps/s while they share the machine)
        const double step_us = u ? 0.4 : (lane ? 2.5 : (c == DC_TINY ? 0.5 : (grpc ? 1.5 : 1.2)));       // one chain step
        const double rate = u ? 0.6e3 : (lane ? 16e3 : (c == DC_TINY ? 30e3 : (grpc ? 12e3 : 2.5e3)));     // steps / us, all CUs
        est[c] = std::max((double)max_n[c] * step_us, (double)sum_n[c] / rate);
    }
    std::sort(order, order + DC_COUNT, [&](int x, int y) { return est[x] > est[y]; });
    double load[DEC_MAX_QUEUES] = {};
    nq = std::min(nq, DEC_MAX_QUEUES);
    for (int k = 0; k < DC_COUNT; k++) {
        const int c = order[k];
        if (!count[c]) continue;
        int best = 0;
        for (int q = 1; q < nq; q++)
            if (load[q] < load[best]) best = q;
        queue_of[c] = best;
        load[best] += est[c] + 1.0;
    }
}

}  // namespace vidc
