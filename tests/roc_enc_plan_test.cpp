// The planning half of the ROC encoder's host call (csrc/roc_enc_plan.h): class boundaries against a hand-written table, the
// by-length route against the per-list route, the chain promotion, octaves, perm items and the schedule grammar; built and run by
// tests/test_roc_enc_plan_cpu.py (g++, no HIP, no GPU).
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "../vector_db_id_compression_amd/csrc/roc_enc_plan.h"

using namespace vidc;

static int fails = 0;
static char what[256] = "";
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d, case %s)\n", #c, __LINE__, what); fails++; } } while (0)

// the values roc.hip fills in from the kernel headers
static const EncLimits LIM{64, 1024, 4096, 8192, 4097, 256, 262144, 8192, 8192, 2048};
enum GrpMode { GRP_OFF, GRP_ON, GRP_FORCED };
static GrpPolicy gpol_of(GrpMode m) {
    GrpPolicy g{8192, 4097, 32768, 16384, 4097};
    if (m == GRP_OFF) g.min_lists = ~0ull;
    if (m == GRP_FORCED) { g.min_lists = 0; g.min_n = g.dec_min_n = 65; g.max_n = g.dec_max_n = 131072; }
    return g;
}
static std::vector<uint64_t> offsets_of(const std::vector<uint64_t> &lens) {
    std::vector<uint64_t> off(lens.size() + 1, 0);
    for (size_t l = 0; l < lens.size(); l++) off[l + 1] = off[l] + lens[l];
    return off;
}
// `parts` contiguous ranges one after the other, cut like the library's threaded form
static auto serial = [](uint64_t n, unsigned parts, auto &&f) {
    if (parts <= 1 || n == 0) { f((uint64_t)0, n, 0u); return; }
    const uint64_t per = (n + parts - 1) / parts;
    for (unsigned t = 0; t < parts; t++) {
        const uint64_t a = std::min<uint64_t>(n, t * per), b = std::min<uint64_t>(n, a + per);
        f(a, b, t);
    }
};

// ---- class boundaries.  One row per length: the general class; the lane class and which family switch it needs (1: lists up to
// 1024 ids, 2: 1025..4096); the row-per-list class under the automatic policy (4097..32768 ids) and under VIDC_FORCE_GRP
// (65..131072); whether a SORTED list of this length may take a universe-bitmap kernel (U_MIN_LIST applies to sorted lists only).
struct Row { uint64_t n; int gen, lane, lane_family, grp_auto, grp_forced; bool u_sorted; };
static const int NONE = -1;
static const Row TABLE[] = {
    {0, W_TINY, NONE, 0, NONE, NONE, false},     {1, W_TINY, NONE, 0, NONE, NONE, false},     {64, W_TINY, NONE, 0, NONE, NONE, false},
    {65, W_C1, W_L4, 1, NONE, W_G2, false},      {256, W_C1, W_L4, 1, NONE, W_G2, false},     {257, W_C1, W_L16, 1, NONE, W_G2, false},
    {1024, W_C1, W_L16, 1, NONE, W_G2, false},   {1025, W_C1, W_L64, 2, NONE, W_G2, false},   {2048, W_C1, W_L64, 2, NONE, W_G2, false},
    {2049, W_C1, W_L64, 2, NONE, W_G2, false},   {4096, W_C1, W_L64, 2, NONE, W_G2, false},   {4097, W_C2, NONE, 0, W_G2, W_G2, true},
    {8192, W_C2, NONE, 0, W_G2, W_G2, true},     {8193, W_C2, NONE, 0, W_G3, W_G3, true},     {32768, W_C2, NONE, 0, W_G3, W_G3, true},
    {32769, W_C3, NONE, 0, NONE, W_G3, true},    {65536, W_C3, NONE, 0, NONE, W_G3, true},    {65537, W_C3, NONE, 0, NONE, W_G3, true},
    {131072, W_C3, NONE, 0, NONE, W_G3, true},   {262144, W_C3, NONE, 0, NONE, NONE, true},
};
static int expected_class(const Row &r, bool have_maxid, bool lane, bool lane64, GrpMode grp, bool unsorted, uint32_t width, bool want_perm,
                          bool f_general) {
    if (r.gen == W_TINY) return W_TINY;
    // the row and lane kernels sample positions: ascending input only
    const int g = unsorted || grp == GRP_OFF ? NONE : (grp == GRP_FORCED ? r.grp_forced : r.grp_auto);
    // rule 1: U_MIN_LIST applies to sorted lists only; rule 2: an unsorted list with want_perm avoids the bitmap classes
    const bool u_ok = have_maxid && !f_general && width <= 20 && (unsorted ? !want_perm : r.u_sorted);
    if (g != NONE && grp == GRP_FORCED) return g;  // rule 3: grp_first precedes the bitmap classes
    if (u_ok) return width <= 18 ? W_U18 : W_U20;
    if (g != NONE) return g;
    if (!unsorted && ((r.lane_family == 1 && lane) || (r.lane_family == 2 && lane64))) return r.lane;
    return r.gen;
}
static void test_class_boundaries() {
    for (const Row &row : TABLE)
        for (int lane = 0; lane < 2; lane++) for (int lane64 = 0; lane64 < 2; lane64++) for (int grp = 0; grp < 3; grp++)
        for (int unsorted = 0; unsorted < 2; unsorted++) for (uint32_t width : {18u, 20u, 21u}) for (int perm = 0; perm < 2; perm++)
        for (int fg = 0; fg < 2; fg++) for (int have = 0; have < 2; have++) {
            if (!have && unsorted) continue;  // (no prepass results: no flags)
            EncPolicy p;
            p.gpol = gpol_of((GrpMode)grp); p.want_perm = perm; p.f_general = fg;
            // (the grp family is `used` when the call has enough such lists; forced: always)
            const int got = enc_class(row.n, have, have ? width : 0, unsorted ? ENC_PF_UNSORTED : 0, lane, lane64, grp != GRP_OFF, p, LIM);
            std::snprintf(what, sizeof what, "n=%llu lane=%d/%d grp=%d unsorted=%d width=%u perm=%d fg=%d maxid=%d got=%d", (unsigned long long)row.n,
                          lane, lane64, grp, unsorted, width, perm, fg, have, got);
            CHECK(got == expected_class(row, have, lane, lane64, (GrpMode)grp, unsorted, width, perm, fg));
        }
    // the three rules once more, spelled out
    std::strcpy(what, "rules");
    EncPolicy p;
    p.gpol = gpol_of(GRP_ON);
    CHECK(enc_class(300, true, 18, 0, false, false, false, p, LIM) == W_C1);                // sorted and short: no bitmap kernel
    CHECK(enc_class(300, true, 18, ENC_PF_UNSORTED, false, false, false, p, LIM) == W_U18);  // unsorted and short: the bitmap needs no sort
    p.want_perm = true;
    CHECK(enc_class(300, true, 18, ENC_PF_UNSORTED, false, false, false, p, LIM) == W_C1);   // ... but cannot report input positions
    CHECK(enc_class(5000, true, 20, ENC_PF_UNSORTED, true, true, true, p, LIM) == W_C2);
    CHECK(enc_class(5000, true, 20, 0, false, false, true, p, LIM) == W_U20);                // automatic row policy: behind the bitmaps
    p.gpol = gpol_of(GRP_FORCED);
    CHECK(enc_class(5000, true, 20, 0, false, false, true, p, LIM) == W_G2);                 // forced: ahead of them
    CHECK(enc_class(9000, true, 18, 0, true, true, true, p, LIM) == W_G3);
    // crossed cases, written out: (n, prepass, width, flags, lane, lane64, grp used) under the forced row policy with want_perm ...
    CHECK(enc_class(65, true, 18, 0, true, true, true, p, LIM) == W_G2 && enc_class(64, true, 18, 0, true, true, true, p, LIM) == W_TINY);
    CHECK(enc_class(131072, true, 21, 0, true, true, true, p, LIM) == W_G3 && enc_class(131073, true, 21, 0, true, true, true, p, LIM) == W_C3);
    CHECK(enc_class(131073, true, 20, 0, true, true, true, p, LIM) == W_U20 && enc_class(2049, true, 20, ENC_PF_UNSORTED, true, true, true, p, LIM) == W_C1);
    p.gpol = gpol_of(GRP_OFF); p.want_perm = false;  // ... and without row kernels, without want_perm
    CHECK(enc_class(256, false, 0, 0, true, false, false, p, LIM) == W_L4 && enc_class(257, false, 0, 0, true, false, false, p, LIM) == W_L16);
    CHECK(enc_class(1025, false, 0, 0, true, false, false, p, LIM) == W_C1 && enc_class(1025, false, 0, 0, false, true, false, p, LIM) == W_L64);
    CHECK(enc_class(4096, true, 18, 0, true, true, false, p, LIM) == W_L64 && enc_class(4097, true, 18, 0, true, true, false, p, LIM) == W_U18);
    CHECK(enc_class(4097, true, 21, 0, true, true, false, p, LIM) == W_C2 && enc_class(32769, true, 21, 0, true, true, false, p, LIM) == W_C3);
    CHECK(enc_class(2049, true, 20, ENC_PF_UNSORTED, true, true, false, p, LIM) == W_U20 && enc_class(2049, true, 21, ENC_PF_UNSORTED, true, true, false, p, LIM) == W_C1);
    p.f_general = true;
    CHECK(enc_class(40000, true, 18, 0, true, true, false, p, LIM) == W_C3 && enc_class(300, true, 18, ENC_PF_UNSORTED, false, false, false, p, LIM) == W_C1);
    // precisions: fixed; bit_width(max) (exact); bit_width(max - 1) (the reference's); empty lists
    CHECK(prec_from_max(0, 77, -1) == 0 && prec_from_max(0, 77, 9) == 0 && prec_from_max(5, 77, 9) == 9 && prec_from_max(5, 77, 0) == 0);
    CHECK(prec_from_max(5, 8, VIDC_PREC_EXACT) == 4 && prec_from_max(5, 7, VIDC_PREC_EXACT) == 3 && prec_from_max(5, 0, VIDC_PREC_EXACT) == 0);
    CHECK(prec_from_max(5, 8, -1) == 3 && prec_from_max(5, 9, -1) == 4 && prec_from_max(5, 1, -1) == 0 && prec_from_max(5, 0, -1) == 0);
    CHECK(prec_from_max(5, 0x7fffffffu, -1) == 31 && prec_from_max(5, 0x80000000u, VIDC_PREC_EXACT) == 32);
}

// ---- both routes
static bool same_lists(const EncWorkLists &a, const EncWorkLists &b) {
    for (int c = 0; c < W_COUNT; c++)
        if (a.wl[c] != b.wl[c]) { std::printf("class %d differs (%zu / %zu lists)\n", c, a.wl[c].size(), b.wl[c].size()); return false; }
    return true;
}
// what the encoder does behind the per-list route: classes not found longest-first get a stable sort by length.  The tiny class is
// never sorted there (its kernels need no order: list order); the by-length route cuts it out of the same longest-first order as
// every other class, so it is compared in that order
static void sort_classes(EncWorkLists &w, const std::vector<uint64_t> &off) {
    for (int c = W_TINY; c < W_COUNT; c++)
        if (!w.sorted[c] || c == W_TINY)
            std::stable_sort(w.wl[c].begin(), w.wl[c].end(), [&](uint32_t x, uint32_t y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
}
static void both_routes(const std::vector<uint64_t> &lens, bool all_desc, const char *name) {
    const std::vector<uint64_t> off = offsets_of(lens);
    const uint64_t nlist = lens.size();
    uint64_t max_n = 0;
    for (uint64_t n : lens) max_n = std::max(max_n, n);
    for (int lane = 0; lane < 2; lane++) for (int lane64 = 0; lane64 < 2; lane64++) for (int grp = 0; grp < 3; grp++) for (int perm = 0; perm < 2; perm++) {
        std::snprintf(what, sizeof what, "%s lane=%d/%d grp=%d perm=%d", name, lane, lane64, grp, perm);
        EncPolicy p;
        p.gpol = gpol_of((GrpMode)grp); p.want_perm = perm;
        EncUse use;
        use.lane = lane; use.lane64 = lane64; use.grp = grp != GRP_OFF;
        EncWorkLists a, b;
        std::vector<uint32_t> order;
        classify_by_length(off.data(), nlist, max_n, all_desc, use, p, LIM, a, order);
        const int64_t bad = classify_per_list(off.data(), nlist, nullptr, nullptr, -1, use, p, LIM, nlist, nlist, 1, serial, nullptr, b);
        CHECK(bad == -1);
        sort_classes(b, off);
        CHECK(same_lists(a, b));
        CHECK(a.total() == nlist && order.size() == nlist);
        std::vector<char> seen(nlist, 0);  // the order: every list once, longest first, equal lengths in list order
        for (size_t i = 0; i < order.size(); i++) {
            CHECK(!seen[order[i]]);
            seen[order[i]] = 1;
            if (i) CHECK(lens[order[i - 1]] > lens[order[i]] || (lens[order[i - 1]] == lens[order[i]] && order[i - 1] < order[i]));
        }
        size_t at = 0;  // base(): the classes back to back in upload order
        for (int c = 0; c < W_COUNT; c++) { CHECK(a.base(c) == at); at += a.wl[c].size(); }
    }
}
static void test_both_routes(std::mt19937_64 &rng) {
    const uint64_t edges[] = {0, 1, 2, 63, 64, 65, 66, 255, 256, 257, 258, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 4095, 4096};
    std::vector<uint64_t> lens;
    for (int rep = 0; rep < 25; rep++) for (uint64_t e : edges) lens.push_back(e);
    for (int i = 0; i < 300; i++) lens.push_back(rng() % 4097);
    std::shuffle(lens.begin(), lens.end(), rng);
    both_routes(lens, false, "shuffled");
    for (uint64_t n : {0ull, 64ull, 65ull, 256ull, 1024ull, 4096ull}) both_routes(std::vector<uint64_t>(777, n), true, "equal");
    both_routes(std::vector<uint64_t>(777, 300), false, "equal, counting sort");
    std::vector<uint64_t> desc(lens);
    std::sort(desc.begin(), desc.end(), std::greater<uint64_t>());
    both_routes(desc, true, "descending");
    both_routes(desc, false, "descending, counting sort");
    std::vector<uint64_t> holes(lens);
    for (size_t i : {(size_t)0, (size_t)1, holes.size() / 2, holes.size() / 2 + 1, holes.size() - 2, holes.size() - 1}) holes[i] = 0;
    both_routes(holes, false, "empty lists at the front, middle and end");
    // beyond the lengths the encoder sends down the by-length route: the same function of the length
    std::vector<uint64_t> big;
    for (const Row &row : TABLE) for (int k = 0; k < 3; k++) big.push_back(row.n);
    std::shuffle(big.begin(), big.end(), rng);
    both_routes(big, false, "every table length");
    both_routes({}, true, "no lists");
}

// ---- the per-list route on 1, 2 and 7 ranges
static void test_parts(std::mt19937_64 &rng) {
    const uint64_t nlist = 3001;
    std::vector<uint64_t> lens(nlist);
    std::vector<uint32_t> maxid(nlist), pflags(nlist, 0);
    for (uint64_t l = 0; l < nlist; l++) {
        const uint64_t k = rng() % 100;
        lens[l] = k < 30 ? rng() % 65 : k < 90 ? 65 + rng() % 5000 : k < 98 ? 4097 + rng() % 60000 : 65537 + rng() % 190000;
        maxid[l] = (uint32_t)(rng() % (1ull << (10 + rng() % 14)));
        if (rng() % 7 == 0) pflags[l] = ENC_PF_UNSORTED;
    }
    const std::vector<uint64_t> off = offsets_of(lens);
    for (int grp = 0; grp < 3; grp++) for (int perm = 0; perm < 2; perm++) for (int mode : {-2, -1, 12}) for (int with_bad = 0; with_bad < 2; with_bad++) {
        std::snprintf(what, sizeof what, "parts grp=%d perm=%d mode=%d bad=%d", grp, perm, mode, with_bad);
        std::vector<uint32_t> pf(pflags);
        int64_t first_bad = -1;
        if (with_bad)  // domain errors in several ranges; (a tiny list is never looked at: its kernel reports it)
            for (uint64_t l : {2900ull, 1400ull, 1399ull, 2000ull}) {
                pf[l] |= ENC_PF_DOMAIN;
                if (lens[l] > 64 && (first_bad < 0 || (int64_t)l < first_bad)) first_bad = (int64_t)l;
            }
        EncPolicy p;
        p.gpol = gpol_of((GrpMode)grp); p.want_perm = perm;
        EncUse use;
        use.lane = use.lane64 = true; use.grp = grp != GRP_OFF;
        EncWorkLists ref;
        std::vector<uint32_t> prec1(nlist, 99);
        const int64_t bad1 = classify_per_list(off.data(), nlist, maxid.data(), pf.data(), mode, use, p, LIM, 0, 0, 1, serial, prec1.data(), ref);
        CHECK(bad1 == first_bad);
        for (unsigned parts : {2u, 7u}) {
            EncWorkLists w;
            std::vector<uint32_t> prec(nlist, 99);
            const int64_t bad = classify_per_list(off.data(), nlist, maxid.data(), pf.data(), mode, use, p, LIM, 0, 0, parts, serial, prec.data(), w);
            CHECK(bad == first_bad);
            if (first_bad < 0) { CHECK(same_lists(ref, w)); CHECK(prec == prec1); }
        }
        if (first_bad >= 0) continue;
        CHECK(ref.total() == nlist);
        for (uint64_t l = 0; l < nlist; l++) CHECK(prec1[l] == prec_from_max(lens[l], maxid[l], mode));
        for (int c = 0; c < W_COUNT; c++)  // list order inside a class; every list in the class enc_class names
            for (size_t i = 0; i < ref.wl[c].size(); i++) {
                const uint32_t l = ref.wl[c][i];
                if (i) CHECK(ref.wl[c][i - 1] < l);
                const uint32_t width = maxid[l] ? 32u - (uint32_t)__builtin_clz(maxid[l]) : 0u;
                CHECK(enc_class(lens[l], true, width, pf[l], true, true, use.grp, p, LIM) == c);
            }
        CHECK(ref.wl[W_R2].empty());
    }
}

// ---- the counting loop and the family switches
static void test_counts() {
    std::strcpy(what, "counts");
    const std::vector<uint64_t> lens = {0, 64, 65, 1024, 1025, 4096, 4097, 32768, 32769, 262144, 0, 7};
    const std::vector<uint64_t> off = offsets_of(lens);
    EncCounts x = count_classes(off.data(), 0, lens.size(), gpol_of(GRP_ON), LIM);
    CHECK(!x.bad && x.nonempty == 10 && x.max_n == 262144 && x.min_n == 0 && x.c0 == 4 && x.c1 == 2 && x.c2 == 2 && x.cg == 2);
    x = count_classes(off.data(), 2, 9, gpol_of(GRP_FORCED), LIM);
    CHECK(!x.bad && x.nonempty == 7 && x.max_n == 32769 && x.min_n == 65 && x.c0 == 0 && x.c1 == 2 && x.c2 == 2 && x.cg == 7);
    EncCounts sum = count_classes(off.data(), 0, 5, gpol_of(GRP_ON), LIM);
    sum.add(count_classes(off.data(), 5, lens.size(), gpol_of(GRP_ON), LIM));
    x = count_classes(off.data(), 0, lens.size(), gpol_of(GRP_ON), LIM);
    CHECK(sum.nonempty == x.nonempty && sum.max_n == x.max_n && sum.min_n == x.min_n && sum.c0 == x.c0 && sum.c1 == x.c1 && sum.c2 == x.c2 && sum.cg == x.cg);
    std::vector<uint64_t> bad = offsets_of({5, 262145, 5});
    CHECK(count_classes(bad.data(), 0, 3, gpol_of(GRP_ON), LIM).bad);
    bad = {0, 10, 9, 20};  // offsets that decrease
    CHECK(count_classes(bad.data(), 0, 3, gpol_of(GRP_ON), LIM).bad);
    EncPolicy p;
    p.gpol = gpol_of(GRP_ON);
    EncUse u = enc_families(2047, 8191, 8192, 8192, p, LIM);
    CHECK(!u.lane_tiny && !u.lane && u.lane64 && !u.grp);  // (the row kernels by themselves: only with the streams for their octaves)
    p.wide = true;
    u = enc_families(2048, 8192, 0, 8192, p, LIM);
    CHECK(u.lane_tiny && u.lane && !u.lane64 && u.grp && !enc_families(0, 0, 0, 8191, p, LIM).grp);
    p.wide = false; p.gpol = gpol_of(GRP_FORCED); p.lpol = LANE_ALWAYS;
    u = enc_families(0, 0, 0, 1, p, LIM);
    CHECK(u.lane_tiny && u.lane && u.lane64 && u.grp && !enc_families(0, 0, 0, 0, p, LIM).grp);
    p.lpol = LANE_NEVER; p.gpol = gpol_of(GRP_OFF);
    u = enc_families(1 << 20, 1 << 20, 1 << 20, 1 << 20, p, LIM);
    CHECK(!u.lane_tiny && !u.lane && !u.lane64 && !u.grp);
}

// ---- promote_r2: lists given as lengths per general class, longest first
struct R2Case { std::vector<uint64_t> c3, c2, c1; };
static void run_r2(const R2Case &k, const EncPolicy &p, size_t want3, size_t want2, size_t want1, const char *name) {
    std::snprintf(what, sizeof what, "promote_r2: %s", name);
    std::vector<uint64_t> lens;
    EncWorkLists w;
    // (list numbers deliberately not in length order)
    for (uint64_t n : k.c1) { w.wl[W_C1].push_back((uint32_t)lens.size()); lens.push_back(n); }
    for (uint64_t n : k.c3) { w.wl[W_C3].push_back((uint32_t)lens.size()); lens.push_back(n); }
    for (uint64_t n : k.c2) { w.wl[W_C2].push_back((uint32_t)lens.size()); lens.push_back(n); }
    const std::vector<uint64_t> off = offsets_of(lens);
    const EncWorkLists before = w;
    promote_r2(w, off.data(), p, LIM);
    // taken: the first want3 of C3, then want2 of C2, then want1 of C1, in that order; the donors keep the rest in their order
    std::vector<uint32_t> r2;
    const size_t want[3] = {want3, want2, want1};
    const int cls[3] = {W_C3, W_C2, W_C1};
    for (int i = 0; i < 3; i++) {
        const std::vector<uint32_t> &b = before.wl[cls[i]];
        CHECK(want[i] <= b.size());
        r2.insert(r2.end(), b.begin(), b.begin() + (ptrdiff_t)want[i]);
        CHECK(w.wl[cls[i]] == std::vector<uint32_t>(b.begin() + (ptrdiff_t)want[i], b.end()));
    }
    CHECK(w.wl[W_R2] == r2);
    for (uint32_t l : w.wl[W_R2]) CHECK(lens[l] > LIM.r2_min_list);
}
static void test_promote_r2() {
    EncPolicy p;
    p.gpol = gpol_of(GRP_OFF);
    p.num_cu = 4;  // cap = 16
    auto rep = [](size_t k, uint64_t n) { return std::vector<uint64_t>(k, n); };
    auto cat = [](std::vector<uint64_t> a, const std::vector<uint64_t> &b) { a.insert(a.end(), b.begin(), b.end()); return a; };
    run_r2({{}, {}, cat(rep(10, 3000), cat(rep(20, 300), rep(5, 200)))}, p, 0, 0, 16, "fewer long lists than cap: filled up with shorter ones");
    run_r2({{}, {}, cat(rep(5, 3000), cat(rep(4, 257), rep(10, 256)))}, p, 0, 0, 9, "lists of 256 ids are never taken");
    run_r2({{}, {}, rep(9, 256)}, p, 0, 0, 0, "only lists of 256 ids");
    run_r2({{}, {}, cat(rep(16, 3000), rep(30, 1000))}, p, 0, 0, 16, "exactly cap long lists");
    run_r2({{}, {}, cat(rep(17, 3000), rep(30, 1000))}, p, 0, 0, 0, "cap + 1 long lists in C1: none");
    run_r2({rep(3, 40000), rep(4, 30000), rep(30, 4000)}, p, 3, 4, 9, "C3, then C2, then C1 once the deeper class is empty");
    run_r2({rep(20, 200000), rep(4, 30000), rep(30, 4000)}, p, 0, 0, 0, "20 equally long lists beyond 65536 ids: none");
    run_r2({cat(rep(8, 200000), rep(12, 40000)), rep(4, 30000), {}}, p, 16, 0, 0, "8 long lists, C3 fills the cap alone");
    run_r2({cat(rep(30, 65536), rep(3, 33000)), rep(7, 20000), rep(7, 4000)}, p, 24, 0, 0, "more than cap, longest <= 65536: cap + cap / 2 from C3 only");
    run_r2({cat(rep(20, 65536), rep(2, 33000)), rep(7, 20000), {}}, p, 22, 0, 0, "... and no further than C3 when it runs out");
    run_r2({cat(rep(30, 65537), rep(3, 33000)), rep(7, 20000), rep(7, 4000)}, p, 0, 0, 0, "more than cap, longest > 65536: none");
    run_r2({{}, rep(30, 30000), rep(7, 4000)}, p, 0, 0, 0, "more than cap without a C3 class: none");
    run_r2({{}, {}, {}}, p, 0, 0, 0, "no general lists");
    EncPolicy q = p;
    q.f_general = true;
    run_r2({{}, {}, rep(10, 3000)}, q, 0, 0, 0, "VIDC_FORCE_GENERAL");
    q = p; q.old_u = true;
    run_r2({{}, {}, rep(10, 3000)}, q, 0, 0, 0, "VIDC_OLD_U");
    q = p; q.no_r2 = true;
    run_r2({{}, {}, rep(10, 3000)}, q, 0, 0, 0, "VIDC_NO_R2");
}

// ---- octaves of the row-per-list classes
static void test_grp_segments(std::mt19937_64 &rng) {
    std::strcpy(what, "grp_segments");
    std::vector<uint64_t> lens = {131072, 100000, 65537, 65536, 40000, 32769, 32768, 16385, 16384, 9000, 8193, 8192, 5000, 4097};
    std::vector<uint64_t> off = offsets_of(lens);
    std::vector<uint32_t> wl(lens.size());
    std::iota(wl.begin(), wl.end(), 0u);
    std::vector<GrpSegment> s = grp_segments(wl, off.data());
    const size_t first[] = {0, 3, 6, 8, 11}, count[] = {3, 3, 2, 3, 3};
    const uint64_t longest[] = {131072, 65536, 32768, 16384, 8192};
    CHECK(s.size() == 5);
    for (size_t i = 0; i < s.size() && i < 5; i++) CHECK(s[i].first == first[i] && s[i].count == count[i] && s[i].longest == longest[i]);
    CHECK(grp_segments({}, off.data()).empty());
    lens.clear();
    for (int i = 0; i < 500; i++) lens.push_back(4097 + rng() % (131072 - 4097 + 1));
    std::sort(lens.begin(), lens.end(), std::greater<uint64_t>());
    off = offsets_of(lens);
    wl.resize(lens.size());
    std::iota(wl.begin(), wl.end(), 0u);
    s = grp_segments(wl, off.data());
    size_t at = 0;
    uint64_t prev_lo = ~0ull;
    for (const GrpSegment &g : s) {
        CHECK(g.first == at && g.count > 0 && g.longest == lens[g.first]);
        uint64_t lo = 1;
        while (lo * 2 < g.longest) lo *= 2;
        for (size_t i = g.first; i < g.first + g.count; i++) CHECK(lens[i] > lo && lens[i] <= 2 * lo);
        CHECK(lo < prev_lo);  // longest octave first
        prev_lo = lo;
        at += g.count;
    }
    CHECK(at == lens.size());
}

// ---- perm fix-up items
static void test_perm_items(std::mt19937_64 &rng) {
    std::strcpy(what, "perm_items");
    for (uint32_t chunk : {2048u, 7u}) for (size_t nul : {(size_t)0, (size_t)1, (size_t)5, (size_t)8, (size_t)40}) {
        std::vector<uint64_t> lens(60);
        for (uint64_t &n : lens) n = 1 + rng() % (chunk * 9);
        lens[3] = 0; lens[4] = chunk; lens[5] = chunk + 1;
        const std::vector<uint64_t> off = offsets_of(lens);
        std::vector<uint32_t> ul;
        for (uint32_t l = 0; ul.size() < nul; l += 1 + (uint32_t)(rng() % 2)) ul.push_back(l % 60 == 59 ? 58 : l % 60);
        std::sort(ul.begin(), ul.end());
        ul.erase(std::unique(ul.begin(), ul.end()), ul.end());
        const std::vector<uint32_t> items = perm_items(ul, off.data(), chunk);
        CHECK(items.size() % 16 == 0);
        const size_t depth = items.size() / 16;
        std::set<std::pair<uint32_t, uint32_t>> got;
        size_t lane_depth_max = 0;
        for (size_t x = 0; x < 8; x++) {
            bool hole_seen = false;
            size_t d = 0;
            for (size_t k = 0; k < depth; k++) {  // lane x's k-th chunk sits at item 8 k + x: no hole ahead of a chunk
                const uint32_t l = items[(8 * k + x) * 2], st = items[(8 * k + x) * 2 + 1];
                if (l == 0xffffffffu) { CHECK(st == 0xffffffffu); hole_seen = true; continue; }
                CHECK(!hole_seen);
                CHECK(st % chunk == 0 && l < 60 && st < lens[l]);
                CHECK(got.insert({l, st}).second);
                d++;
            }
            lane_depth_max = std::max(lane_depth_max, d);
        }
        CHECK(lane_depth_max == depth);
        size_t want = 0;
        for (uint32_t l : ul) {
            for (uint64_t st = 0; st < lens[l]; st += chunk) { CHECK(got.count({l, (uint32_t)st}) == 1); want++; }
        }
        CHECK(got.size() == want);
    }
}

// ---- schedule strings
static const char *DEC_NAMES[] = {"TINY", "U18", "U20", "GSMALL", "G8K", "G16K", "GMID", "GHUGE", "LANE", "LANE64", "LANE128", "B2", "B2T", "B2S",
                                  "B2L", "B2M", "GRP0", "GRP2", "GRP3", "GRP4", "LANEP", "LANEQ"};
static int dec_find(const std::string &t) {
    for (int c = 0; c < 22; c++) if (t == DEC_NAMES[c]) return c;
    return -1;
}
struct E { int item, group, pos; std::vector<int> deps; };
static bool same_sched(const std::vector<SchedEntry> &s, const std::vector<E> &e) {
    if (s.size() != e.size()) return false;
    for (size_t i = 0; i < s.size(); i++)
        if (s[i].item != e[i].item || s[i].group != e[i].group || s[i].pos != e[i].pos || s[i].deps != e[i].deps) return false;
    return true;
}
// the launches run_schedule makes, in order; `done` comes back for the caller's "launch the rest"
static std::vector<int> run(std::vector<SchedEntry> s, size_t nitems, bool drop, std::vector<char> *done_out = nullptr, int fail_at = -1) {
    std::stable_sort(s.begin(), s.end(), [](const SchedEntry &x, const SchedEntry &y) { return x.pos < y.pos; });
    std::vector<char> done(nitems, 0);
    std::vector<int> seq;
    const int rc = run_schedule(s, done, drop, [&](const SchedEntry &it) -> int {
        for (int d : it.deps) CHECK(done[d]);
        if (it.item == fail_at) return 7;
        seq.push_back(it.item);
        return 0;
    });
    CHECK(rc == (fail_at >= 0 ? 7 : 0));
    if (done_out) *done_out = done;
    return seq;
}
static void test_schedule() {
    std::strcpy(what, "schedule");
    const int B2 = 11, GHUGE = 7, LANEP = 20, LANE = 8, LANE64 = 9, GMID = 6, TINY = 0, U18 = 1;
    std::vector<SchedEntry> s = parse_schedule("B2;GHUGE;LANEP,LANE,LANE64;GMID^LANEP", dec_find, 3, false);
    CHECK(same_sched(s, {{B2, 0, 0, {}}, {GHUGE, 1, 0, {}}, {LANEP, 2, 0, {}}, {LANE, 2, 1, {}}, {LANE64, 2, 2, {}}, {GMID, 3, 0, {LANEP}}}));
    // host launch order: first entries of every stream, then the second ones, ...
    CHECK(run(s, 22, false) == std::vector<int>({B2, GHUGE, LANEP, GMID, LANE, LANE64}));
    CHECK(parse_schedule(nullptr, dec_find, 3, false).empty() && parse_schedule("", dec_find, 3, false).empty());
    CHECK(parse_schedule(";,;,,", dec_find, 3, false).empty());
    // empty tokens take no position; unknown names are no entry and no dependency
    CHECK(same_sched(parse_schedule(";,TINY,,U18;", dec_find, 3, false), {{TINY, 1, 0, {}}, {U18, 1, 1, {}}}));
    CHECK(same_sched(parse_schedule("NOPE,TINY^WHAT^U18^,nope^TINY,U18", dec_find, 3, false), {{TINY, 0, 0, {U18}}, {U18, 0, 1, {}}}));
    // a group beyond max_groups (the caller's stream + max_groups auxiliary ones)
    CHECK(same_sched(parse_schedule("TINY;U18;B2;LANE", dec_find, 2, false), {{TINY, 0, 0, {}}, {U18, 1, 0, {}}, {B2, 2, 0, {}}}));
    // the same name twice
    CHECK(same_sched(parse_schedule("TINY,TINY^B2,U18", dec_find, 3, true), {{TINY, 0, 0, {}}, {U18, 0, 1, {}}}));
    s = parse_schedule("TINY,TINY^B2,U18", dec_find, 3, false);
    CHECK(same_sched(s, {{TINY, 0, 0, {}}, {TINY, 0, 1, {B2}}, {U18, 0, 2, {}}}));
    std::vector<char> done;
    CHECK(run(s, 22, false, &done) == std::vector<int>({TINY, U18}) && done[TINY] && done[U18] && !done[B2]);
    CHECK(run(s, 22, true) == std::vector<int>({TINY, U18}));
    // a dependency launched later in the list waits for the next round
    CHECK(run(parse_schedule("TINY^U18,U18,B2", dec_find, 3, true), 22, true) == std::vector<int>({U18, B2, TINY}));
    // a self-dependency, a two-cycle: the encoder drops every dependency and goes on, the decoder stops and leaves the rest
    s = parse_schedule("TINY^TINY,U18", dec_find, 3, true);
    CHECK(same_sched(s, {{TINY, 0, 0, {TINY}}, {U18, 0, 1, {}}}));
    CHECK(run(s, 22, true) == std::vector<int>({U18, TINY}));
    CHECK(run(s, 22, false, &done) == std::vector<int>({U18}) && !done[TINY]);
    s = parse_schedule("TINY^U18;U18^TINY;B2^U18", dec_find, 3, true);
    CHECK(same_sched(s, {{TINY, 0, 0, {U18}}, {U18, 1, 0, {TINY}}, {B2, 2, 0, {U18}}}));
    CHECK(run(s, 22, true) == std::vector<int>({TINY, U18, B2}));
    CHECK(run(s, 22, false, &done).empty() && !done[TINY] && !done[U18] && !done[B2]);
    // a dependency nobody launches (the decoder: a class the string does not schedule)
    s = parse_schedule("TINY^B2,U18", dec_find, 3, false);
    CHECK(run(s, 22, false, &done) == std::vector<int>({U18}) && !done[TINY]);
    CHECK(run(s, 22, true) == std::vector<int>({U18, TINY}));
    // an error from a launch ends the loop
    CHECK(run(parse_schedule("TINY,U18,B2", dec_find, 3, true), 22, true, nullptr, U18) == std::vector<int>({TINY}));
}

int main() {
    std::mt19937_64 rng(20240607);
    test_class_boundaries();
    test_both_routes(rng);
    test_parts(rng);
    test_counts();
    test_promote_r2();
    test_grp_segments(rng);
    test_perm_items(rng);
    test_schedule();
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("roc enc plan ok\n");
    return 0;
}
