// Stand-alone check of csrc/ivf_scan_ref.h and csrc/ivf_scan_plan.h (g++, no HIP): the serial scan built from the rules against cases
// the numpy model writes out (tests/ivf_scan_ref.py), as one piece and as S pieces merged for every S, every array in an allocation
// of its exact size so that a sanitizer build sees any read or write outside it; the argument checks and the plan's figures.
//   ivf_scan_test                                    self checks
//   ivf_scan_test cases < text                       the model's cases
//   ivf_scan_test plan nq num_cu kind d M nprobe k   prints: lds resident S items nslots scratch min_items max_items G V W merge_lds
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/ivf_scan_plan.h"
#include "../vector_db_id_compression_amd/csrc/ivf_scan_ref.h"

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
    // keys order like (distance, position); ~0 is above every key
    CHECK(ivs::key_less(ivs::key_make(1.f, 7), ivs::key_make(2.f, 3)) && ivs::key_less(ivs::key_make(2.f, 3), ivs::key_make(2.f, 4)));
    CHECK(!ivs::key_less(ivs::key_make(2.f, 3), ivs::key_make(2.f, 3)) && ivs::key_less(ivs::key_make(0.f, 0xfffffffeu), ivs::key_make(1e-30f, 0)));
    CHECK(ivs::key_less(ivs::key_make(INFINITY, 0xfffffffeu), ivs::EMPTY));
    const uint64_t kk = ivs::key_make(12.5f, 0xfffffffeu);
    CHECK(ivs::key_pos(kk) == 0xfffffffeu && ivs::key_dist(kk) == 12.5f);
    CHECK(ivs::key_dropped(ivs::key_make(2.f, 3), ivs::key_make(2.f, 3)) && ivs::key_dropped(ivs::key_make(2.f, 4), ivs::key_make(2.f, 3)));
    CHECK(!ivs::key_dropped(ivs::key_make(2.f, 2), ivs::key_make(2.f, 3)) && !ivs::key_dropped(ivs::key_make(3e38f, 0), ivs::EMPTY));
    // probes
    CHECK(ivs::probe_list(-1, 8) == -1 && ivs::probe_list(8, 8) == -1 && ivs::probe_list(1ll << 40, 8) == -1 && ivs::probe_list(7, 8) == 7);
    CHECK(ivs::probe_list(0, 0) == -1 && ivs::probe_list(0x7ffffffe, 0x7fffffff) == 0x7ffffffe && ivs::probe_list(INT64_MIN, 8) == -1);
    const int32_t row[6] = {5, -1, 5, 6, -1, 5};
    CHECK(!ivs::probe_repeats(row, 0) && !ivs::probe_repeats(row, 1) && ivs::probe_repeats(row, 2) && !ivs::probe_repeats(row, 3));
    CHECK(!ivs::probe_repeats(row, 4) && ivs::probe_repeats(row, 5));
    for (uint32_t S = 1; S <= 16; S *= 2)
        for (uint32_t np : {1u, 3u, 16u, 17u, 1024u}) {
            CHECK(ivs::piece_begin(np, S, 0) == 0 && ivs::piece_begin(np, S, S) == np);
            for (uint32_t s = 0; s < S; s++) CHECK(ivs::piece_begin(np, S, s) <= ivs::piece_begin(np, S, s + 1));
        }
    // the clamp
    ivs::Range r = ivs::list_range(3, 9, 100);
    CHECK(r.a == 3 && r.b == 9);
    r = ivs::list_range(9, 3, 100);
    CHECK(r.a == 3 && r.b == 3);
    r = ivs::list_range(90, 200, 100);
    CHECK(r.a == 90 && r.b == 100);
    r = ivs::list_range(~0ull, ~0ull, 100);
    CHECK(r.a == 100 && r.b == 100);
    r = ivs::list_range(5, 7, 0);
    CHECK(r.a == 0 && r.b == 0);
    // ranks and places
    const uint64_t keys[4] = {ivs::key_make(1.f, 1), ivs::key_make(1.f, 5), ivs::key_make(2.f, 0), ivs::EMPTY};
    CHECK(ivs::lower_bound(keys, 4, ivs::key_make(0.f, 9)) == 0 && ivs::lower_bound(keys, 4, ivs::key_make(1.f, 3)) == 1);
    CHECK(ivs::lower_bound(keys, 4, ivs::key_make(9.f, 0)) == 3 && ivs::lower_bound(keys, 4, ivs::EMPTY) == 3 && ivs::lower_bound(keys, 0, 5) == 0);
    CHECK(ivs::place_kept(3, 4) && !ivs::place_kept(4, 4));
    const uint64_t runs[6] = {ivs::key_make(1.f, 1), ivs::key_make(3.f, 0), ivs::EMPTY, ivs::key_make(2.f, 9), ivs::EMPTY, ivs::EMPTY};
    CHECK(ivs::merge_place(runs, 2, 3, 0, 0) == 0 && ivs::merge_place(runs, 2, 3, 1, 0) == 1 && ivs::merge_place(runs, 2, 3, 0, 1) == 2);
    uint64_t out[3];
    ivs::merge_serial(runs, 2, 3, out);
    CHECK(out[0] == runs[0] && out[1] == runs[3] && out[2] == runs[1]);
    // labels: empty lists in front of a position lose
    const uint64_t off[6] = {0, 0, 1, 1, 5, 5};
    CHECK(ivs::list_of(off, 5, 0) == 1 && ivs::list_of(off, 5, 1) == 3 && ivs::list_of(off, 5, 4) == 3 && ivs::list_of(off, 1, 0) == 0);
    CHECK(ivs::key_label(off, 5, ivs::key_make(1.f, 3)) == ((3ll << 32) | 2));
    const uint64_t bad[4] = {9, 2, ~0ull, 0};  // damaged offsets: the index stays inside
    for (uint64_t pos = 0; pos < 12; pos++) CHECK(ivs::list_of(bad, 3, pos) < 3);
    // argument checks
    int dummy = 0;
    const void *p = &dummy;
    const ivs::Args ok = {16, p, 2000, p, ivs::PQ8, 128, 16, p, 5, p, 4, p, 20, p, p};
    CHECK(ivs::check_args(ok) == nullptr);
    auto refused = [&](void (*edit)(ivs::Args &)) {
        ivs::Args a = ok;
        edit(a);
        return ivs::check_args(a) != nullptr;
    };
    CHECK(refused([](ivs::Args &a) { a.offsets = nullptr; }) && refused([](ivs::Args &a) { a.codes = nullptr; }));
    CHECK(refused([](ivs::Args &a) { a.xq = nullptr; }) && refused([](ivs::Args &a) { a.probes = nullptr; }));
    CHECK(refused([](ivs::Args &a) { a.D = nullptr; }) && refused([](ivs::Args &a) { a.labels = nullptr; }));
    CHECK(refused([](ivs::Args &a) { a.k = 0; }) && refused([](ivs::Args &a) { a.k = 257; }) && refused([](ivs::Args &a) { a.nprobe = 0; }));
    CHECK(refused([](ivs::Args &a) { a.nprobe = 1025; }) && refused([](ivs::Args &a) { a.d = 0; }) && refused([](ivs::Args &a) { a.d = 2049; }));
    CHECK(refused([](ivs::Args &a) { a.ntotal = 1ull << 32; }) && refused([](ivs::Args &a) { a.nlist = 1ull << 31; }));
    CHECK(refused([](ivs::Args &a) { a.kind = 2; }) && refused([](ivs::Args &a) { a.kind = -1; }) && refused([](ivs::Args &a) { a.M = 0; }));
    CHECK(refused([](ivs::Args &a) { a.M = 65; a.d = 65; }) && refused([](ivs::Args &a) { a.M = 3; }) && refused([](ivs::Args &a) { a.codebooks = nullptr; }));
    const ivs::Args edge = {(1ull << 31) - 1, p, (1ull << 32) - 1, p, ivs::PQ8, 2048, 64, p, 1ull << 40, p, 1024, p, 256, p, p};
    CHECK(ivs::check_args(edge) == nullptr);
    const ivs::Args flat = {16, p, 2000, p, ivs::FLAT, 7, 0, nullptr, 5, p, 4, p, 20, p, p};  // FLAT looks at neither M nor the codebooks
    CHECK(ivs::check_args(flat) == nullptr);
    const ivs::Args none = {16, nullptr, 2000, nullptr, ivs::FLAT, 7, 0, nullptr, 0, nullptr, 4, nullptr, 20, nullptr, nullptr};  // nq == 0
    CHECK(ivs::check_args(none) == nullptr);
    // plan
    CHECK(ivs::lds_bytes(ivs::PQ8, 20, 16, 128, 16) == 17536 && ivs::lds_bytes(ivs::PQ8, 256, 1024, 2048, 64) == 77824);
    CHECK(ivs::lds_bytes(ivs::FLAT, 20, 16, 32, 0) == 1280 && ivs::lds_bytes(ivs::FLAT, 256, 1024, 2048, 0) == 17152);
    CHECK(ivs::slots_per_cu(77824) == 2 && ivs::slots_per_cu(17536) == 9 && ivs::slots_per_cu(1280) == 32 && ivs::slots_per_cu(200000) == 1);
    CHECK(ivs::resident_slots(256, 1280) == 8192 && ivs::resident_slots(256, 17536) == 2304 && ivs::resident_slots(1, 1280) == 32);
    CHECK(ivs::pieces(10, 16, 2304) == 16 && ivs::pieces(1000, 16, 2304) == 4 && ivs::pieces(10000, 16, 2304) == 1);
    CHECK(ivs::pieces(10, 1, 2304) == 1 && ivs::pieces(10, 3, 2304) == 2 && ivs::pieces(10, 4, 2304) == 4 && ivs::pieces(10, 1024, 8192) == 16);
    CHECK(ivs::pieces(2304, 16, 2304) == 1 && ivs::pieces(2303, 16, 2304) == 2);
    CHECK(ivs::scratch_bytes(10, 16, 20) == 10 * 16 * 21 * 8 && ivs::scratch_bytes(10, 1, 20) == 0 && ivs::scratch_keys(10, 16, 20) == 3200);
    CHECK(ivs::slots(0, 32) == 1 && ivs::slots(10, 32) == 10 && ivs::slots(100, 32) == 32);
    CHECK(ivs::code_load_bytes(16, 0x1000) == 16 && ivs::code_load_bytes(16, 0x1004) == 4 && ivs::code_load_bytes(12, 0x1000) == 4);
    CHECK(ivs::code_load_bytes(64, 0x1008) == 8 && ivs::code_load_bytes(1, 0x1000) == 1 && ivs::code_load_bytes(6, 0x1000) == 2);
    CHECK(ivs::code_load_bytes(16, 0x1001) == 1);
}

static bool read_u64(uint64_t &v) {
    unsigned long long t;
    if (std::scanf("%llu", &t) != 1) return false;
    v = t;
    return true;
}
static bool read_f32(float &f) {
    char buf[64];
    if (std::scanf("%63s", buf) != 1) return false;
    f = std::strtof(buf, nullptr);
    return true;
}

static int run_cases() {
    uint64_t ncases = 0, nqueries = 0, nruns = 0;
    if (!read_u64(ncases)) return 2;
    for (uint64_t c = 0; c < ncases; c++) {
        uint64_t nlist, ntotal, kind, d, M, nq, nprobe, k;
        if (!(read_u64(nlist) && read_u64(ntotal) && read_u64(kind) && read_u64(d) && read_u64(M) && read_u64(nq) && read_u64(nprobe) && read_u64(k))) return 2;
        const uint64_t code_size = kind == ivs::PQ8 ? M : d * 4;
        auto off = exact<uint64_t>(nlist + 1);
        auto codes = exact<uint8_t>(ntotal * code_size);
        auto cb = exact<float>(kind == ivs::PQ8 ? 256 * d : 0);
        auto xq = exact<float>(nq * d);
        auto probes = exact<int64_t>(nq * nprobe);
        auto wantD = exact<float>(nq * k);
        auto wantL = exact<long long>(nq * k);
        auto wantS = exact<uint32_t>(nq * 2);
        for (uint64_t i = 0; i <= nlist; i++) if (!read_u64(off[i])) return 2;
        for (uint64_t i = 0; i < ntotal * code_size; i++) {
            unsigned b;
            if (std::scanf("%u", &b) != 1) return 2;
            codes[i] = (uint8_t)b;
        }
        if (kind == ivs::PQ8) for (uint64_t i = 0; i < 256 * d; i++) if (!read_f32(cb[i])) return 2;
        for (uint64_t i = 0; i < nq * d; i++) if (!read_f32(xq[i])) return 2;
        for (uint64_t i = 0; i < nq * nprobe; i++) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            probes[i] = v;
        }
        for (uint64_t i = 0; i < nq * k; i++) if (!read_f32(wantD[i])) return 2;
        for (uint64_t i = 0; i < nq * k; i++) if (std::scanf("%lld", &wantL[i]) != 1) return 2;
        for (uint64_t i = 0; i < nq * 2; i++) if (std::scanf("%u", &wantS[i]) != 1) return 2;
        const ivs::Args args = {nlist, off.get(), ntotal, codes.get(), (int)kind, (uint32_t)d, (uint32_t)M, cb.get(), nq, xq.get(),
                                (uint32_t)nprobe, probes.get(), (uint32_t)k, wantD.get(), wantL.get()};
        if (ivs::check_args(args)) {
            std::printf("FAIL case %llu: refused: %s\n", (unsigned long long)c, ivs::check_args(args));
            fails++;
            continue;
        }
        for (uint64_t q = 0; q < nq; q++) {
            for (uint32_t S = 1; S <= ivs::MAX_S; S *= 2) {
                auto row = exact<int32_t>(nprobe);
                auto table = exact<float>(kind == ivs::PQ8 ? M * 256 : 0);
                auto runs = exact<uint64_t>((uint64_t)S * k);
                auto tmp = exact<uint64_t>(k);
                auto cand = exact<uint64_t>(ivs::TRIP);
                auto res = exact<uint64_t>(k);
                uint32_t lists = 0, ncodes = 0;
                for (uint32_t s = 0; s < S; s++) {
                    ivs::Stats st;
                    ivs::scan_serial(nlist, off.get(), ntotal, codes.get(), (int)kind, (uint32_t)d, (uint32_t)M, cb.get(), xq.get() + q * d,
                                     (uint32_t)nprobe, probes.get() + q * nprobe, (uint32_t)k, S, s, row.get(), table.get(),
                                     runs.get() + (uint64_t)s * k, tmp.get(), cand.get(), &st);
                    lists += st.lists;
                    ncodes += st.codes;
                }
                ivs::merge_serial(runs.get(), S, (uint32_t)k, res.get());
                bool same = lists == wantS[q * 2] && ncodes == wantS[q * 2 + 1];
                for (uint64_t i = 0; i < k; i++) {
                    const float D = res[i] == ivs::EMPTY ? INFINITY : ivs::key_dist(res[i]);
                    const long long L = res[i] == ivs::EMPTY ? -1 : (long long)ivs::key_label(off.get(), nlist, res[i]);
                    same = same && D == wantD[q * k + i] && L == wantL[q * k + i];
                }
                if (!same) {
                    std::printf("FAIL case %llu query %llu S %u: lists %u/%u codes %u/%u\n", (unsigned long long)c, (unsigned long long)q, S,
                                lists, wantS[q * 2], ncodes, wantS[q * 2 + 1]);
                    fails++;
                }
                nruns++;
            }
            nqueries++;
        }
    }
    std::printf("%llu cases, %llu queries, %llu runs\n", (unsigned long long)ncases, (unsigned long long)nqueries, (unsigned long long)nruns);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 9 && !std::strcmp(argv[1], "plan")) {
        const uint64_t nq = std::strtoull(argv[2], nullptr, 10);
        uint32_t v[6];
        for (int i = 0; i < 6; i++) v[i] = (uint32_t)std::strtoul(argv[3 + i], nullptr, 10);
        const ivs::Plan p = ivs::make_plan(v[0], (int)v[1], v[2], v[3], nq, v[4], v[5], 0, 0);
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t i = 0; i < p.nslots; i++) {
            const uint64_t n = ivs::slot_items(p.items, p.nslots, i);
            lo = n < lo ? n : lo;
            hi = n > hi ? n : hi;
        }
        std::printf("%zu %u %u %llu %u %llu %llu %llu %u %u %u %zu\n", p.lds, p.resident, p.S, (unsigned long long)p.items, p.nslots,
                    (unsigned long long)p.scratch, (unsigned long long)lo, (unsigned long long)hi, p.grp.G, p.grp.V, p.W, p.merge_lds);
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "cases")) {
        const int r = run_cases();
        if (r) { std::printf("FAIL: malformed case text\n"); return r; }
    } else {
        self_checks();
    }
    if (fails) return 1;
    std::printf("ivf scan ok\n");
    return 0;
}
