// Stand-alone check of csrc/graph_search_ref.h and csrc/graph_search_plan.h (g++, no HIP): the serial search built from the step
// rules against cases the numpy model writes out (tests/graph_search_ref.py), every array in an allocation of its exact size so
// that a sanitizer build sees any read or write outside it; the argument checks and the plan's figures.
//   graph_search_test                      self checks
//   graph_search_test cases < text         the model's cases
//   graph_search_test plan nq num_cu N L d prints: slots scratch_bytes lds_bytes min_queries max_queries G V
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/graph_search_plan.h"
#include "../vector_db_id_compression_amd/csrc/graph_search_ref.h"

using namespace vidc;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

static void self_checks() {
    // keys order like (distance, node); the flag does not take part
    CHECK(gs::key_less(gs::key_make(1.f, 7), gs::key_make(2.f, 3)));
    CHECK(gs::key_less(gs::key_make(2.f, 3), gs::key_make(2.f, 4)));
    CHECK(!gs::key_less(gs::key_expand(gs::key_make(2.f, 3)), gs::key_make(2.f, 3)));
    CHECK(!gs::key_less(gs::key_make(2.f, 3), gs::key_expand(gs::key_make(2.f, 3))));
    CHECK(gs::key_less(gs::key_expand(gs::key_make(2.f, 3)), gs::key_make(2.f, 4)));
    CHECK(gs::key_less(gs::key_make(0.f, 0x7fffffffu), gs::key_make(1e-30f, 0)));
    CHECK(gs::key_less(gs::key_make(3e38f, 5), gs::key_make(INFINITY, 0)));
    const uint64_t kk = gs::key_expand(gs::key_make(12.5f, 0x7fffffffu));
    CHECK(gs::key_node(kk) == 0x7fffffffu && gs::key_dist(kk) == 12.5f && gs::key_expanded(kk));
    CHECK(!gs::key_expanded(gs::key_make(12.5f, 1)));
    // loop bound
    CHECK(gs::step_bound(100, 0) == 100 && gs::step_bound(100, 3) == 3 && gs::step_bound(100, 1000) == 100 && gs::step_bound(0, 0) == 0);
    CHECK(gs::step_bound((1ull << 31) - 1, 0) == 0x7fffffffu && gs::step_bound(5, 0xffffffffu) == 5);
    // claim
    CHECK(gs::vis_word(0) == 0 && gs::vis_word(31) == 0 && gs::vis_word(32) == 1 && gs::vis_bit(33) == 2u && gs::vis_bit(31) == 0x80000000u);
    CHECK(gs::claim_won(0xfffffffdu, 2u) && !gs::claim_won(2u, 2u));
    CHECK(gs::id_usable(4, 5) && !gs::id_usable(5, 5) && !gs::id_usable(~0ull, 5));
    // ranks
    const uint64_t keys[4] = {gs::key_make(1.f, 1), gs::key_expand(gs::key_make(1.f, 5)), gs::key_make(2.f, 0), gs::key_make(4.f, 9)};
    CHECK(gs::lower_bound(keys, 4, gs::key_make(0.f, 9)) == 0 && gs::lower_bound(keys, 4, gs::key_make(1.f, 3)) == 1);
    CHECK(gs::lower_bound(keys, 4, gs::key_make(1.f, 6)) == 2 && gs::lower_bound(keys, 4, gs::key_make(9.f, 0)) == 4);
    CHECK(gs::lower_bound(keys, 0, gs::key_make(9.f, 0)) == 0);
    CHECK(gs::first_unexpanded(keys, 4) == 0 && gs::first_unexpanded(keys + 1, 3) == 1 && gs::first_unexpanded(keys + 1, 1) == 1);
    CHECK(gs::merged_size(3, 4, 8) == 7 && gs::merged_size(5, 4, 8) == 8 && gs::place_kept(7, 8) && !gs::place_kept(8, 8));
    // argument checks
    int dummy = 0;
    const void *p = &dummy;
    gs::Args ok = {100, p, 16, 5, p, 10, 64, 0, 0, p, p};
    CHECK(gs::check_args(ok) == nullptr);
    auto bad = [&](void (*edit)(gs::Args &)) {
        gs::Args a = ok;
        edit(a);
        return gs::check_args(a) != nullptr;
    };
    CHECK(bad([](gs::Args &a) { a.x = nullptr; }) && bad([](gs::Args &a) { a.xq = nullptr; }) && bad([](gs::Args &a) { a.D = nullptr; }));
    CHECK(bad([](gs::Args &a) { a.I = nullptr; }) && bad([](gs::Args &a) { a.k = 0; }) && bad([](gs::Args &a) { a.k = 65; }));
    CHECK(bad([](gs::Args &a) { a.L = 257; a.k = 257; }) && bad([](gs::Args &a) { a.L = 257; }) && bad([](gs::Args &a) { a.d = 0; }));
    CHECK(bad([](gs::Args &a) { a.d = 2049; }) && bad([](gs::Args &a) { a.entry = 100; }) && bad([](gs::Args &a) { a.N = 1ull << 31; }));
    CHECK(bad([](gs::Args &a) { a.nq = 0xffffffffull; }) && bad([](gs::Args &a) { a.N = 0; }));
    gs::Args edge = {(1ull << 31) - 1, p, 2048, 0xfffffffeull, p, 256, 256, 0x7ffffffeu, 0xffffffffu, p, p};
    CHECK(gs::check_args(edge) == nullptr);
    gs::Args none = {100, nullptr, 16, 0, nullptr, 10, 64, 0, 0, nullptr, nullptr};  // nq == 0: no array is needed
    CHECK(gs::check_args(none) == nullptr);
    // plan
    CHECK(gs::slots(1, 256) == 1 && gs::slots(300, 256) == 300 && gs::slots(100000, 256) == 1024 && gs::slots(101, 1) == 32);
    CHECK(gs::slots(0, 256) == 1 && gs::slots(10, 0) == 1);
    CHECK(gs::vis_words64(1) == 1 && gs::vis_words64(64) == 1 && gs::vis_words64(65) == 2 && gs::vis_words64(1000000) == 15625);
    CHECK(gs::scratch_bytes(1024, 1000000) == 128000000ull);
    uint64_t total = 0;
    for (uint32_t s = 0; s < 32; s++) total += gs::slot_queries(101, 32, s);
    CHECK(total == 101 && gs::slot_queries(101, 32, 4) == 4 && gs::slot_queries(101, 32, 5) == 3 && gs::slot_queries(3, 32, 5) == 0);
    CHECK(gs::group(16, true).G == 4 && gs::group(16, true).V == 4 && gs::group(16, false).G == 16 && gs::group(16, false).V == 1);
    CHECK(gs::group(1, true).G == 1 && gs::group(4, true).G == 1 && gs::group(8, true).G == 2 && gs::group(2048, true).G == 16);
    CHECK(gs::group(7, true).V == 1 && gs::group(7, true).G == 8 && gs::group(3, false).G == 4);
    CHECK(gs::lds_bytes(64, 16) == 2112 && gs::lds_bytes(256, 2048) == 13312 && gs::lds_bytes(1, 1) % 16 == 0);
}

static bool read_u64(uint64_t &v) {
    unsigned long long t;
    if (std::scanf("%llu", &t) != 1) return false;
    v = t;
    return true;
}

static int run_cases() {
    uint64_t ncases = 0, nqueries = 0;
    if (!read_u64(ncases)) return 2;
    for (uint64_t c = 0; c < ncases; c++) {
        uint64_t N, K, d, nq, k, L, entry, max_rounds;
        if (!(read_u64(N) && read_u64(K) && read_u64(d) && read_u64(nq) && read_u64(k) && read_u64(L) && read_u64(entry) && read_u64(max_rounds))) return 2;
        auto rows = exact<int32_t>(N * K);
        auto x = exact<float>(N * d);
        auto xq = exact<float>(nq * d);
        auto wantD = exact<float>(nq * k);
        auto wantI = exact<long long>(nq * k);
        auto wantS = exact<uint32_t>(nq * 2);
        for (uint64_t i = 0; i < N * K; i++) if (std::scanf("%d", &rows[i]) != 1) return 2;
        char buf[64];
        auto rf = [&](float &f) {
            if (std::scanf("%63s", buf) != 1) return false;
            f = std::strtof(buf, nullptr);
            return true;
        };
        for (uint64_t i = 0; i < N * d; i++) if (!rf(x[i])) return 2;
        for (uint64_t i = 0; i < nq * d; i++) if (!rf(xq[i])) return 2;
        for (uint64_t i = 0; i < nq * k; i++) if (!rf(wantD[i])) return 2;
        for (uint64_t i = 0; i < nq * k; i++) if (std::scanf("%lld", &wantI[i]) != 1) return 2;
        for (uint64_t i = 0; i < nq * 2; i++) if (std::scanf("%u", &wantS[i]) != 1) return 2;
        const int32_t *rp = rows.get();
        auto row = [rp, K](uint32_t node, uint32_t j) { return (int64_t)rp[(uint64_t)node * K + j]; };
        for (uint64_t q = 0; q < nq; q++) {
            auto pool = exact<uint64_t>(L);
            auto tmp = exact<uint64_t>(L);
            auto cand = exact<uint64_t>(gs::TRIP);
            auto vis = exact<uint32_t>((N + 31) / 32);
            gs::Stats st;
            const uint32_t P = gs::search_serial(N, (uint32_t)K, row, x.get(), (uint32_t)d, xq.get() + q * d, (uint32_t)L, (uint32_t)entry,
                                                 (uint32_t)max_rounds, pool.get(), tmp.get(), cand.get(), vis.get(), &st);
            bool same = st.steps == wantS[q * 2] && st.dists == wantS[q * 2 + 1];
            for (uint64_t i = 0; i < k; i++) {
                const float D = i < P ? gs::key_dist(pool[i]) : INFINITY;
                const long long I = i < P ? (long long)gs::key_node(pool[i]) : -1;
                same = same && D == wantD[q * k + i] && I == wantI[q * k + i];
            }
            if (!same) {
                std::printf("FAIL case %llu query %llu: steps %u/%u dists %u/%u\n", (unsigned long long)c, (unsigned long long)q, st.steps,
                            wantS[q * 2], st.dists, wantS[q * 2 + 1]);
                fails++;
            }
            nqueries++;
        }
    }
    std::printf("%llu cases, %llu queries\n", (unsigned long long)ncases, (unsigned long long)nqueries);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 7 && !std::strcmp(argv[1], "plan")) {
        const uint64_t nq = std::strtoull(argv[2], nullptr, 10), N = std::strtoull(argv[4], nullptr, 10);
        const uint32_t cu = (uint32_t)std::strtoul(argv[3], nullptr, 10), L = (uint32_t)std::strtoul(argv[5], nullptr, 10),
                       d = (uint32_t)std::strtoul(argv[6], nullptr, 10);
        const uint32_t s = gs::slots(nq, cu);
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t i = 0; i < s; i++) {
            const uint64_t n = gs::slot_queries(nq, s, i);
            lo = n < lo ? n : lo;
            hi = n > hi ? n : hi;
        }
        const gs::Group g = gs::group(d, true);
        std::printf("%u %llu %zu %llu %llu %u %u\n", s, (unsigned long long)gs::scratch_bytes(s, N), gs::lds_bytes(L, d), (unsigned long long)lo,
                    (unsigned long long)hi, g.G, g.V);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "cases")) {
        const int r = run_cases();
        if (r) { std::printf("FAIL: malformed case text\n"); return r; }
    } else {
        self_checks();
    }
    if (fails) return 1;
    std::printf("graph search ok\n");
    return 0;
}
