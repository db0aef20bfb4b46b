// roc_enc_plan.h -- the planning half of the ROC encoder's host call (roc.hip: encode_impl): which kernel class takes which list, in
// which order, and the grammar of the VIDC_ENC_SCHED / VIDC_DEC_SCHED schedule strings.  Host code only, no HIP include and nothing
// that touches a stream: tests/roc_enc_plan_test.cpp builds it with g++.  roc.hip fills EncLimits from the kernel headers' macros and
// EncPolicy from the environment and the context, at the points where it always read them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vidc.h"

namespace vidc {

enum LanePolicy { LANE_NEVER = 0, LANE_AUTO = 1, LANE_ALWAYS = 2 };
inline bool lane_wanted(LanePolicy p, uint64_t nlists, uint64_t min_lists) { return p == LANE_ALWAYS || (p == LANE_AUTO && nlists >= min_lists); }
struct GrpPolicy { uint64_t min_lists, min_n, max_n, dec_max_n, dec_min_n; };
// prepass flags of a list (roc_u.h: VIDC_PF_*; roc.hip asserts that they agree)
constexpr uint32_t ENC_PF_UNSORTED = 1u, ENC_PF_DOMAIN = 2u;
// class boundaries that belong to no kernel header: 4-word lane strips, the general kernel's first and second prefix-row depth
constexpr uint64_t ENC_L4_MAX = 256, ENC_C1_MAX = 4096, ENC_C2_MAX = 32768;
struct EncLimits { uint64_t tiny_max, lane_max, lane_max64, grp_lev2_max, u_min_list, r2_min_list, roc_max_list, lane_min_lists, lane_min_lists64, lane_min_tiny; };
struct EncPolicy {
    bool f_general = false, old_u = false, no_r2 = false, no_length_classes = false, wide = false, want_perm = false;
    LanePolicy lpol = LANE_AUTO;
    GrpPolicy gpol{};
    int num_cu = 0;
};
// work lists: tiny (n <= 64), universe-bitmap kernels (ids < 2^18 / 2^20), general kernels by bitmap depth, lane-per-list kernels,
// position-bitmap chains, row-per-list kernels.  The order is the upload order: kernels receive d_wl + base(c), and the tiny class
// relies on being first.
enum EncClass { W_TINY, W_U18, W_U20, W_C1, W_C2, W_C3, W_L4, W_L16, W_L64, W_R2, W_G2, W_G3, W_COUNT };
struct EncWorkLists {
    std::vector<uint32_t> wl[W_COUNT];
    bool sorted[W_COUNT] = {};  // classes found longest-first while they were filled (one-part classification only)
    size_t base(int c) const { size_t b = 0; for (int k = 0; k < c; k++) b += wl[k].size(); return b; }
    size_t total() const { return base(W_COUNT); }
};

// validity, extremes and the class sizes the kernel-family policies look at, of lists [la, lb): the one counting loop
struct EncCounts {
    uint64_t nonempty = 0, max_n = 0, min_n = ~0ull, c0 = 0, c1 = 0, c2 = 0, cg = 0;  // c0 tiny, c1 / c2 the lane classes, cg in reach of the row kernels
    bool bad = false;
    void add(const EncCounts &x) {
        nonempty += x.nonempty; max_n = std::max(max_n, x.max_n); min_n = std::min(min_n, x.min_n); c0 += x.c0; c1 += x.c1; c2 += x.c2; cg += x.cg; bad |= x.bad;
    }
};
inline EncCounts count_classes(const uint64_t *offsets, uint64_t la, uint64_t lb, const GrpPolicy &gpol, const EncLimits &lim) {
    EncCounts x;
    for (uint64_t l = la; l < lb; l++) {
        const uint64_t n = offsets[l + 1] - offsets[l];
        x.bad |= n > lim.roc_max_list;
        x.nonempty += n != 0;
        x.max_n = std::max(x.max_n, n);
        x.min_n = std::min(x.min_n, n);
        x.c0 += n <= lim.tiny_max;
        x.c1 += n > lim.tiny_max && n <= lim.lane_max;
        x.c2 += n > lim.lane_max && n <= lim.lane_max64;
        x.cg += n >= gpol.min_n && n <= gpol.max_n;
    }
    return x;
}
// Kernel families of a call, from its class sizes.  The bitmap kernels own a whole CU's LDS (2^20-bit universe): latency-optimal for
// long lists, but only num_cu lists in flight.  With many lists, short ones go to the high-occupancy kernels.
struct EncUse { bool lane = false, lane64 = false, lane_tiny = false, grp = false; };
inline EncUse enc_families(uint64_t n_tiny, uint64_t n_mid, uint64_t n_mid64, uint64_t n_grp, const EncPolicy &p, const EncLimits &lim) {
    EncUse u;
    u.lane = lane_wanted(p.lpol, n_mid, lim.lane_min_lists);
    u.lane64 = lane_wanted(p.lpol, n_mid64, lim.lane_min_lists64);
    u.lane_tiny = lane_wanted(p.lpol, n_tiny, lim.lane_min_tiny);
    // (the octaves of a call must overlap: without spare hardware queues they would run one after the other)
    u.grp = n_grp && n_grp >= p.gpol.min_lists && (p.wide || p.gpol.min_lists == 0);
    return u;
}
inline uint32_t prec_from_max(uint64_t n, uint32_t m, int precision_mode) {
    return n == 0 ? 0u
           : precision_mode >= 0    ? (uint32_t)precision_mode
           : precision_mode == VIDC_PREC_EXACT ? (m ? 32u - (uint32_t)__builtin_clz(m) : 0u)
                                               : (m > 1u ? 32u - (uint32_t)__builtin_clz(m - 1u) : 0u);
}

// The class of a list of n ids inside the domain.  have_maxid: the prepass results are on the host (width: ids < 2^width; pflags);
// without them (prepass read back later: no list is long enough for the bitmap kernels, the only classes chosen by the width of the
// ids) the class is a function of the length alone.
inline EncClass enc_class(uint64_t n, bool have_maxid, uint32_t width, uint32_t pflags, bool use_lane, bool use_lane64, bool use_grp,
                          const EncPolicy &p, const EncLimits &lim) {
    if (n <= lim.tiny_max) return W_TINY;
    const bool unsorted = pflags & ENC_PF_UNSORTED;
    // the bitmap kernels need no sort; they cannot report input positions of an unsorted list
    const bool u_ok = have_maxid && !p.f_general && !(unsorted && p.want_perm) && (n >= lim.u_min_list || unsorted);
    const bool lane_ok = !unsorted && ((use_lane && n <= lim.lane_max) || (use_lane64 && n > lim.lane_max && n <= lim.lane_max64));
    // (the row-per-list kernel samples positions: ascending input; it checks that itself under the light prepass)
    const bool grp_ok = use_grp && n >= p.gpol.min_n && n <= p.gpol.max_n && !unsorted;
    const bool grp_first = grp_ok && p.gpol.min_lists == 0;  // VIDC_FORCE_GRP: ahead of every other family
    return grp_first ? (n <= lim.grp_lev2_max ? W_G2 : W_G3)
           : (u_ok && width <= 18) ? W_U18
           : (u_ok && width <= 20) ? W_U20
           : grp_ok ? (n <= lim.grp_lev2_max ? W_G2 : W_G3)
           : (lane_ok && n <= ENC_L4_MAX) ? W_L4
           : (lane_ok && n <= lim.lane_max) ? W_L16
           : lane_ok ? W_L64
           : n <= ENC_C1_MAX ? W_C1
           : n <= ENC_C2_MAX ? W_C2 : W_C3;
}

// Without per-list maxima the class of a list is a function of its LENGTH: the lists are ordered by length once -- longest first, a
// stable counting sort, or nothing at all for an index of equal-sized lists -- and every class is a run of that order, copied out
// between two binary searches.  The per-list loop with its dozen push_back targets and the per-class sorts behind it were
// 0.13 + 0.02 ms of a 65 536-list call.  `order` (empty on entry; the caller's to pool) comes back as every list of the call,
// longest first: the decode planner cuts its classes out of the same order.
inline void classify_by_length(const uint64_t *offsets, uint64_t nlist, uint64_t max_n, bool all_desc, const EncUse &use,
                               const EncPolicy &p, const EncLimits &lim, EncWorkLists &w, std::vector<uint32_t> &order) {
    order.resize(nlist);
    if (all_desc) {
        std::iota(order.begin(), order.end(), 0u);
    } else {
        std::vector<uint32_t> start(max_n + 2, 0);
        for (uint64_t l = 0; l < nlist; l++) start[max_n - (offsets[l + 1] - offsets[l]) + 1]++;  // bucket 0 = longest
        for (size_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
        for (uint64_t l = 0; l < nlist; l++) order[start[max_n - (offsets[l + 1] - offsets[l])]++] = (uint32_t)l;
    }
    auto len_at = [&](size_t i) { return offsets[order[i] + 1] - offsets[order[i]]; };
    auto first_le = [&](uint64_t bound) {  // first position of the order whose list has at most `bound` ids
        size_t lo = 0, hi = nlist;
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (len_at(mid) > bound) lo = mid + 1; else hi = mid; }
        return lo;
    };
    // upper ends of the length intervals on which enc_class is constant, longest first
    uint64_t cuts[] = {lim.roc_max_list, p.gpol.max_n, ENC_C2_MAX, lim.grp_lev2_max, ENC_C1_MAX, lim.lane_max64, p.gpol.min_n - 1, lim.lane_max, ENC_L4_MAX, lim.tiny_max};
    std::sort(std::begin(cuts), std::end(cuts), std::greater<uint64_t>());
    const size_t ncuts = sizeof(cuts) / sizeof(cuts[0]);
    size_t pos = 0;
    for (size_t c = 0; c < ncuts && pos < nlist; c++) {
        const uint64_t hi = cuts[c], lo = c + 1 < ncuts ? cuts[c + 1] : 0;  // interval (lo, hi]
        if (hi == lo) continue;
        const size_t end = lo ? first_le(lo) : nlist;  // (the last interval also takes the empty lists)
        if (end > pos) {
            std::vector<uint32_t> &dst = w.wl[enc_class(hi, false, 0, 0, use.lane, use.lane64, use.grp, p, lim)];
            dst.insert(dst.end(), order.begin() + (ptrdiff_t)pos, order.begin() + (ptrdiff_t)end);
            pos = end;
        }
    }
    for (int c = 0; c < W_COUNT; c++) w.sorted[c] = true;
}

// The per-list route: one pass with the prepass results (maxid / pflags; both may be null) over `parts` contiguous ranges run by
// par(nlist, parts, f(begin, end, part)), concatenated in range order: the same lists in the same order as a single pass.  prec[] is
// filled where maxid is given.  Returns the first list with an id outside the domain, or -1.  n_tiny / n_lane4: upper bounds of two
// class sizes (no regrowth while 65 536 lists are appended).
template <class Par>
inline int64_t classify_per_list(const uint64_t *offsets, uint64_t nlist, const uint32_t *maxid, const uint32_t *pflags, int precision_mode,
                                 const EncUse &use, const EncPolicy &p, const EncLimits &lim, uint64_t n_tiny, uint64_t n_lane4,
                                 unsigned parts, Par &&par, uint32_t *prec, EncWorkLists &w) {
    std::vector<std::vector<uint32_t>> part_wl((size_t)parts * W_COUNT);
    std::vector<int64_t> bad_list(parts, -1);
    bool cls_desc[W_COUNT];
    uint64_t cls_last[W_COUNT];
    for (int c = 0; c < W_COUNT; c++) { cls_desc[c] = parts == 1; cls_last[c] = ~0ull; }
    par(nlist, parts, [&](uint64_t la, uint64_t lb, unsigned tpart) {
        std::vector<uint32_t> *pw = &part_wl[(size_t)tpart * W_COUNT];
        if (parts == 1) { pw[W_TINY].reserve(n_tiny); pw[W_L4].reserve(n_lane4); }
        for (uint64_t l = la; l < lb; l++) {
            const uint64_t n = offsets[l + 1] - offsets[l];
            if (maxid) prec[l] = prec_from_max(n, maxid[l], precision_mode);
            if (n <= lim.tiny_max) { pw[W_TINY].push_back((uint32_t)l); continue; }
            const uint32_t pf = pflags ? pflags[l] : 0u;  // (deferred prepass: no list of the call depends on them)
            if (pf & ENC_PF_DOMAIN) { if (bad_list[tpart] < 0) bad_list[tpart] = (int64_t)l; continue; }
            const uint32_t width = (maxid && maxid[l]) ? 32u - (uint32_t)__builtin_clz(maxid[l]) : 0u;  // ids < 2^width
            const int cls = enc_class(n, maxid != nullptr, width, pf, use.lane, use.lane64, use.grp, p, lim);
            pw[cls].push_back((uint32_t)l);
            if (parts == 1) {  // (is the class already longest-first?  equal-sized lists: saves the sort's own pass)
                cls_desc[cls] &= n <= cls_last[cls];
                cls_last[cls] = n;
            }
        }
    });
    for (unsigned t = 0; t < parts; t++)
        if (bad_list[t] >= 0) return bad_list[t];  // the first offending list, as a single pass would report it
    for (int c = 0; c < W_COUNT; c++) {
        w.sorted[c] = cls_desc[c];
        if (parts == 1) { w.wl[c].swap(part_wl[c]); continue; }
        size_t tot = 0;
        for (unsigned t = 0; t < parts; t++) tot += part_wl[(size_t)t * W_COUNT + c].size();
        w.wl[c].reserve(tot);
        for (unsigned t = 0; t < parts; t++) {
            const auto &v = part_wl[(size_t)t * W_COUNT + c];
            w.wl[c].insert(w.wl[c].end(), v.begin(), v.end());
        }
    }
    return -1;
}

// The longest general lists (any precision, more than 256 ids) take the position-bitmap chain kernel
// (k_roc_encode_r2: 0.26 instead of 0.48 us per step alone) -- when ALL the chains that decide the call's duration
// fit on the machine at once: at most four per CU (32 KiB of LDS and 233 VGPRs each), and only if no more than that
// many lists are at least half as long as the longest one.  1024 lists of 977 ids: encode 0.51 -> 0.35 ms; 256 x
// 3900: 1.75 -> 1.07; 1024 x 6000: 3.9 -> 2.5.  On S2 (1754 lists of 32 769..65 536 ids) 1024 of these chains took
// the LDS the lane-per-list classes need and the call went from 78 to 117 ms: there the general kernel, which packs
// six times as many chains per CU, keeps all of them.
// (the general classes of `w` are sorted longest first)
inline void promote_r2(EncWorkLists &w, const uint64_t *offsets, const EncPolicy &p, const EncLimits &lim) {
    if (p.f_general || p.old_u || p.no_r2) return;
    std::vector<uint32_t> &c1 = w.wl[W_C1], &c2 = w.wl[W_C2], &c3 = w.wl[W_C3], &r2 = w.wl[W_R2];
    const size_t cap = (size_t)p.num_cu * 4;
    const std::vector<uint32_t> &top = !c3.empty() ? c3 : (!c2.empty() ? c2 : c1);
    if (top.empty()) return;
    const uint64_t n_top = offsets[top[0] + 1] - offsets[top[0]];
    size_t n_long = 0;
    for (const std::vector<uint32_t> *v : {&c3, &c2, &c1})
        for (uint32_t l : *v) { if (2 * (offsets[l + 1] - offsets[l]) < n_top || n_long > cap) break; n_long++; }
    size_t take_cap = cap;
    auto take = [&](std::vector<uint32_t> &v) {
        size_t k = 0;
        while (k < v.size() && r2.size() < take_cap && offsets[v[k] + 1] - offsets[v[k]] > lim.r2_min_list) r2.push_back(v[k++]);
        v.erase(v.begin(), v.begin() + (ptrdiff_t)k);
    };
    if (n_long <= cap) {
        take(c3);
        if (c3.empty()) take(c2);
        if (c3.empty() && c2.empty()) take(c1);
    } else if (n_top <= 65536 && !c3.empty()) {
        // More long chains than that (S2: 1754 lists of 32 769..65 536 ids): the `cap` longest ones -- one per SIMD --
        // still decide the call (65 536 steps at 0.9 us on the general kernel under load against ~0.7 here) and, with
        // the bitmap sized for 65 536 positions (8 KiB instead of 32), no longer take the LDS the other classes need;
        // the rest of the class (<= ~45 000 ids on S2) finishes earlier on the general kernel anyway.
        // Half as many again queue behind the resident ones in the same launch: each starts when one of the longest
        // chains has finished, still ends before the launch's longest chain would have on the general kernel, and
        // leaves that kernel ~500 fewer chains (S2 encode 59-62 -> 55-57 ms; all 1754: 59).
        take_cap = cap + cap / 2;
        take(c3);
    }
}

// row-per-list kernels: one launch per octave of list length (the LDS of a launch is sized by its longest list).  A work list sorted
// longest first -> segments of lengths in (lo, 2 lo], lo a power of two
struct GrpSegment { size_t first, count; uint64_t longest; };
inline std::vector<GrpSegment> grp_segments(const std::vector<uint32_t> &wl, const uint64_t *offsets) {
    std::vector<GrpSegment> segs;
    size_t k0 = 0;
    while (k0 < wl.size()) {
        const uint64_t n0 = offsets[wl[k0] + 1] - offsets[wl[k0]];  // longest of the segment
        uint64_t lo = 1;
        while (lo * 2 < n0) lo *= 2;
        size_t k1 = k0;
        while (k1 < wl.size() && offsets[wl[k1] + 1] - offsets[wl[k1]] > lo) k1++;
        segs.push_back({k0, k1 - k0, n0});
        k0 = k1;
    }
    return segs;
}
// perm fix-up of the bitmap-kernel lists: (list, first position of a chunk) pairs.  lists -> 8 lanes (longest first to the lane with
// the fewest chunks), lane x's k-th chunk at item 8 k + x; holes are 0xffffffff pairs
inline std::vector<uint32_t> perm_items(const std::vector<uint32_t> &ul, const uint64_t *offsets, uint32_t chunk) {
    std::vector<uint32_t> byl(ul);
    std::stable_sort(byl.begin(), byl.end(), [&](uint32_t x, uint32_t y) { return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y]; });
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> lanes(8);
    for (uint32_t l : byl) {
        size_t best = 0;
        for (size_t x = 1; x < 8; x++)
            if (lanes[x].size() < lanes[best].size()) best = x;
        for (uint64_t st0 = 0, n = offsets[l + 1] - offsets[l]; st0 < n; st0 += chunk) lanes[best].push_back({l, (uint32_t)st0});
    }
    size_t depth = 0;
    for (auto &ln : lanes) depth = std::max(depth, ln.size());
    std::vector<uint32_t> items(depth * 8 * 2, 0xffffffffu);
    for (size_t x = 0; x < 8; x++)
        for (size_t k = 0; k < lanes[x].size(); k++) {
            items[(k * 8 + x) * 2] = lanes[x][k].first;
            items[(k * 8 + x) * 2 + 1] = lanes[x][k].second;
        }
    return items;
}

// ---- VIDC_ENC_SCHED / VIDC_DEC_SCHED (measurements): an explicit schedule of a call's launches.  Streams separated by ';' (first =
// the caller's stream, then the auxiliary ones), the launches of a stream by ',' in FIFO order; "NAME^DEP" also waits for launch DEP.
// Host launch order: first entries of every stream, then the second ones, ... (run_schedule's caller sorts by pos).
// find(name) -> launch index, or -1 for a name the call does not have: such an entry is dropped, such a dependency ignored; so are
// the entries of stream groups beyond max_groups and, with first_only, every repetition of a name -- WITH their dependencies (a
// deliberate change for VIDC_ENC_SCHED: its parser used to add the dependencies of such an entry to the name's first entry).
struct SchedEntry { int item, group, pos; std::vector<int> deps; };
template <class Find>
inline std::vector<SchedEntry> parse_schedule(const char *s, Find &&find, int max_groups, bool first_only) {
    std::vector<SchedEntry> sched;
    const std::string str(s ? s : "");
    int grp = 0, pos = 0; size_t i0 = 0;
    for (size_t i = 0; i <= str.size(); i++) {
        if (i < str.size() && str[i] != ',' && str[i] != ';') continue;
        const std::string tok = str.substr(i0, i - i0);
        i0 = i + 1;
        if (!tok.empty()) {
            SchedEntry it{-1, grp, pos, {}};
            size_t j0 = 0;
            bool first = true;
            for (size_t j = 0; j <= tok.size(); j++) {
                if (j < tok.size() && tok[j] != '^') continue;
                const int c = find(tok.substr(j0, j - j0));
                j0 = j + 1;
                if (first) it.item = c; else if (c >= 0) it.deps.push_back(c);
                first = false;
            }
            bool seen = false;
            if (first_only) for (const SchedEntry &x : sched) seen |= x.item == it.item;
            if (it.item >= 0 && !seen && grp <= max_groups) { sched.push_back(it); pos++; }
        }
        if (i < str.size() && str[i] == ';') { grp++; pos = 0; }
    }
    return sched;
}
// The ready / dependency loop: entries in host launch order, done[] per launch index.  launch(entry) queues one (after its waits) and
// returns 0 or an error, which ends the loop.  An entry whose dependency is launched later in the list waits for the next round; in
// a round without progress (circular dependencies, or a dependency nobody launches) either every dependency is dropped and the loop
// goes on (drop_deps_on_stall) or the loop ends and the caller launches what is not done[].  A repeated entry is skipped.
template <class Launch>
inline int run_schedule(std::vector<SchedEntry> &entries, std::vector<char> &done, bool drop_deps_on_stall, Launch &&launch) {
    size_t left = entries.size(); bool dropped = false;
    while (left) {
        const size_t before = left;
        for (SchedEntry &it : entries) {
            if (done[it.item]) continue;
            bool ready = true;
            for (int d : it.deps) ready &= done[d] != 0;
            if (!ready) continue;
            if (const int rc = launch(it)) return rc;
            done[it.item] = 1;
            left--;
        }
        if (left == before) {
            if (!drop_deps_on_stall || dropped) break;
            for (SchedEntry &it : entries) it.deps.clear();
            dropped = true;
        }
    }
    return 0;
}

}  // namespace vidc
