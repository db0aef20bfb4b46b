// Stand-alone check of csrc/ivf_residual_ref.h and csrc/ivf_residual_plan.h (g++, no HIP): the serial residual-PQ scan, count and fill
// built from the rules against cases the numpy model writes out (tests/ivf_residual_ref.py), as one piece and as four, every array in
// an allocation of its exact size so that a sanitizer build sees any read or write outside it; the argument checks and the plan.
//   ivf_residual_test                                self checks
//   ivf_residual_test cases < text                   the model's cases
//   ivf_residual_test plan nq num_cu d M nprobe k    prints two lines, scan and range: lds resident S items nslots scratch min_items
//                                                    max_items W merge_lds
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../vector_db_id_compression_amd/csrc/ivf_residual_plan.h"
#include "../vector_db_id_compression_amd/csrc/ivf_residual_ref.h"

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

static const float POISON_D = -12345.f;
static const int64_t POISON_L = 0x5a5a5a5a5a5a5a5all;

static void self_checks() {
    // the residual and the table of a list: d = 4, M = 2, entry (m, c) of the codebooks is (c, -c)
    const float xq[4] = {1.f, 2.f, 3.f, 4.f}, cent[8] = {9.f, 9.f, 9.f, 9.f, 1.f, 1.f, 1.f, 1.f};
    auto cb = exact<float>(2 * 256 * 2);
    for (int m = 0; m < 2; m++)
        for (int c = 0; c < 256; c++) {
            cb[(m * 256 + c) * 2] = (float)c;
            cb[(m * 256 + c) * 2 + 1] = -(float)c;
        }
    float r[4];
    ivx::residual(xq, cent + 4, 4, r);
    CHECK(r[0] == 0.f && r[1] == 1.f && r[2] == 2.f && r[3] == 3.f);
    auto table = exact<float>(512);
    ivx::list_table(xq, cent, 1, 4, 2, cb.get(), r, table.get());
    CHECK(table[0] == 1.f && table[1] == 1.f + 4.f && table[256] == 4.f + 9.f && table[256 + 2] == 0.f + 25.f);
    ivx::list_table(xq, cent, 0, 4, 2, cb.get(), r, table.get());  // (another list: another table)
    CHECK(r[0] == -8.f && table[0] == 64.f + 49.f);
    // argument checks: the scan's for PQ8, and the centroids
    int dummy = 0;
    const void *p = &dummy;
    const ivx::Args ok = {16, p, 2000, p, 128, 16, p, p, 5, p, 4, p};
    CHECK(!ivx::check_scan(ok, 20, p, p) && !ivx::check_count(ok, p) && !ivx::check_fill(ok, p, 10, p, p) && !ivx::check_fill(ok, p, 0, nullptr, nullptr));
    auto refused = [&](void (*edit)(ivx::Args &)) {
        ivx::Args a = ok;
        edit(a);
        return ivx::check_scan(a, 20, p, p) && ivx::check_count(a, p) && ivx::check_fill(a, p, 10, p, p);
    };
    CHECK(refused([](ivx::Args &a) { a.offsets = nullptr; }) && refused([](ivx::Args &a) { a.codes = nullptr; }));
    CHECK(refused([](ivx::Args &a) { a.xq = nullptr; }) && refused([](ivx::Args &a) { a.probes = nullptr; }));
    CHECK(refused([](ivx::Args &a) { a.centroids = nullptr; }) && refused([](ivx::Args &a) { a.codebooks = nullptr; }));
    CHECK(refused([](ivx::Args &a) { a.nprobe = 0; }) && refused([](ivx::Args &a) { a.nprobe = 1025; }));
    CHECK(refused([](ivx::Args &a) { a.d = 0; }) && refused([](ivx::Args &a) { a.d = 2049; }));
    CHECK(refused([](ivx::Args &a) { a.ntotal = 1ull << 32; }) && refused([](ivx::Args &a) { a.nlist = 1ull << 31; }));
    CHECK(refused([](ivx::Args &a) { a.M = 0; }) && refused([](ivx::Args &a) { a.M = 65; a.d = 65; }) && refused([](ivx::Args &a) { a.M = 3; }));
    CHECK(ivx::check_scan(ok, 0, p, p) && ivx::check_scan(ok, 257, p, p) && ivx::check_scan(ok, 20, nullptr, p) && ivx::check_scan(ok, 20, p, nullptr));
    CHECK(ivx::check_count(ok, nullptr) && ivx::check_fill(ok, nullptr, 10, p, p) && ivx::check_fill(ok, p, 1, nullptr, p) && ivx::check_fill(ok, p, 1, p, nullptr));
    ivx::Args wide = ok;
    wide.nq = 1ull << 22;
    wide.nprobe = 1024;
    CHECK(!ivx::check_scan(wide, 20, p, p) && ivx::check_count(wide, p) && ivx::check_fill(wide, p, 10, p, p));  // nq * nprobe >= 2^32 - 1
    const ivx::Args none = {16, nullptr, 2000, nullptr, 128, 16, p, nullptr, 0, nullptr, 4, nullptr};  // nq == 0: no array is needed
    CHECK(!ivx::check_scan(none, 20, nullptr, nullptr) && !ivx::check_count(none, nullptr) && !ivx::check_fill(none, nullptr, 0, nullptr, nullptr));
    CHECK(ivx::check_scan(none, 0, nullptr, nullptr));  // (the limits still hold)
    // plan
    CHECK(ivx::scan_lds_bytes(20, 16, 128, 16) == 18560 && ivx::scan_lds_bytes(256, 1024, 2048, 64) == 90880);
    CHECK(ivx::range_lds_bytes(16, 128, 16) == 17472 && ivx::range_lds_bytes(1024, 2048, 64) == 4096 + 16384 + 65536);
    CHECK(ivx::pool_bytes(20) == 1088 && ivx::pool_bytes(20) % 16 == 0 && ivx::pool_bytes(1) % 16 == 0 && ivx::vec_bytes(7) == 32);
    CHECK(ivx::codebook_vec4(128, 16, 0x1000) && !ivx::codebook_vec4(128, 16, 0x1004) && !ivx::codebook_vec4(24, 4, 0x1000) && ivx::codebook_vec4(4, 1, 0));
    CHECK(!ivx::codebook_vec4(4, 4, 0) && ivx::scan_plan(256, 128, 16, 10, 16, 20, 0, 16).vec4 && !ivx::range_plan(256, 128, 16, 10, 16, 0, 8).vec4);
    CHECK(ivs::slots_per_cu(18560) == 8 && ivs::slots_per_cu(90880) == 1 && ivs::slots_per_cu(17472) == 9);
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
static bool same_f32(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static int run_cases() {
    uint64_t ncases = 0, nruns = 0;
    if (!read_u64(ncases)) return 2;
    for (uint64_t c = 0; c < ncases; c++) {
        uint64_t nlist, ntotal, d, M, nq, nprobe, k, total;
        float radius;
        if (!(read_u64(nlist) && read_u64(ntotal) && read_u64(d) && read_u64(M) && read_u64(nq) && read_u64(nprobe) && read_u64(k) &&
              read_f32(radius) && read_u64(total)))
            return 2;
        const uint64_t nslots = nq * nprobe;
        auto off = exact<uint64_t>(nlist + 1);
        auto codes = exact<uint8_t>(ntotal * M);
        auto cb = exact<float>(256 * d);
        auto cent = exact<float>(nlist * d);
        auto xq = exact<float>(nq * d);
        auto probes = exact<int64_t>(nslots);
        auto wantD = exact<float>(nq * k);
        auto wantL = exact<long long>(nq * k);
        auto wantS = exact<uint32_t>(nq * 2);
        auto lims = exact<uint64_t>(nslots + 1);
        auto wantRD = exact<float>(total);
        auto wantRL = exact<long long>(total);
        for (uint64_t i = 0; i <= nlist; i++) if (!read_u64(off[i])) return 2;
        for (uint64_t i = 0; i < ntotal * M; i++) {
            unsigned b;
            if (std::scanf("%u", &b) != 1) return 2;
            codes[i] = (uint8_t)b;
        }
        for (uint64_t i = 0; i < 256 * d; i++) if (!read_f32(cb[i])) return 2;
        for (uint64_t i = 0; i < nlist * d; i++) if (!read_f32(cent[i])) return 2;
        for (uint64_t i = 0; i < nq * d; i++) if (!read_f32(xq[i])) return 2;
        for (uint64_t i = 0; i < nslots; i++) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            probes[i] = v;
        }
        for (uint64_t i = 0; i < nq * k; i++) if (!read_f32(wantD[i])) return 2;
        for (uint64_t i = 0; i < nq * k; i++) if (std::scanf("%lld", &wantL[i]) != 1) return 2;
        for (uint64_t i = 0; i < nq * 2; i++) if (std::scanf("%u", &wantS[i]) != 1) return 2;
        for (uint64_t i = 0; i <= nslots; i++) if (!read_u64(lims[i])) return 2;
        for (uint64_t i = 0; i < total; i++) if (!read_f32(wantRD[i])) return 2;
        for (uint64_t i = 0; i < total; i++) if (std::scanf("%lld", &wantRL[i]) != 1) return 2;
        const ivx::Args args = {nlist, off.get(), ntotal, codes.get(), (uint32_t)d, (uint32_t)M, cb.get(), cent.get(), nq, xq.get(), (uint32_t)nprobe,
                                probes.get()};
        if (ivx::check_scan(args, (uint32_t)k, wantD.get(), wantL.get()) || ivx::check_count(args, lims.get()) || lims[nslots] != total) {
            std::printf("FAIL case %llu: refused or malformed\n", (unsigned long long)c);
            fails++;
            continue;
        }
        for (uint32_t S : {1u, 4u}) {
            if (S > nprobe) continue;
            auto row = exact<int32_t>(nprobe);
            auto r = exact<float>(d);
            auto table = exact<float>(M * 256);
            // scan: the pieces of every query, merged
            for (uint64_t q = 0; q < nq; q++) {
                auto runs = exact<uint64_t>((uint64_t)S * k);
                auto tmp = exact<uint64_t>(k);
                auto cand = exact<uint64_t>(ivs::TRIP);
                auto res = exact<uint64_t>(k);
                uint32_t lists = 0, ncodes = 0;
                for (uint32_t s = 0; s < S; s++) {
                    ivs::Stats st;
                    ivx::scan_serial(nlist, off.get(), ntotal, codes.get(), (uint32_t)d, (uint32_t)M, cb.get(), cent.get(), xq.get() + q * d,
                                     (uint32_t)nprobe, probes.get() + q * nprobe, (uint32_t)k, S, s, row.get(), r.get(), table.get(),
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
                    std::printf("FAIL case %llu query %llu S %u: the scan differs from the model\n", (unsigned long long)c, (unsigned long long)q, S);
                    fails++;
                }
            }
            // count: every slot written, the prefix sum is the model's; fill at the exact capacity and at half of it
            auto counts = exact<uint32_t>(nslots);
            for (uint64_t i = 0; i < nslots; i++) counts[i] = 0xdeadbeefu;
            for (uint64_t q = 0; q < nq; q++)
                for (uint32_t s = 0; s < S; s++)
                    ivx::count_serial(nlist, off.get(), ntotal, codes.get(), (uint32_t)d, (uint32_t)M, cb.get(), cent.get(), xq.get() + q * d,
                                      (uint32_t)nprobe, probes.get() + q * nprobe, radius, S, s, row.get(), r.get(), table.get(),
                                      counts.get() + q * nprobe);
            bool same = true;
            uint64_t acc = 0;
            for (uint64_t s = 0; s < nslots; s++) {
                same = same && acc == lims[s];
                acc += counts[s];
            }
            same = same && acc == total;
            for (uint64_t cap : {total, total / 2}) {
                auto D = exact<float>(cap);
                auto L = exact<int64_t>(cap);
                for (uint64_t i = 0; i < cap; i++) {
                    D[i] = POISON_D;
                    L[i] = POISON_L;
                }
                for (uint64_t q = 0; q < nq; q++)
                    for (uint32_t s = 0; s < S; s++)
                        ivx::fill_serial(nlist, off.get(), ntotal, codes.get(), (uint32_t)d, (uint32_t)M, cb.get(), cent.get(), xq.get() + q * d,
                                         (uint32_t)nprobe, probes.get() + q * nprobe, radius, S, s, row.get(), r.get(), table.get(),
                                         lims.get() + q * nprobe, cap, D.get(), L.get());
                for (uint64_t i = 0; i < cap; i++) same = same && same_f32(D[i], wantRD[i]) && L[i] == wantRL[i];
            }
            if (!same) {
                std::printf("FAIL case %llu S %u: count or fill differs from the model\n", (unsigned long long)c, S);
                fails++;
            }
            nruns++;
        }
    }
    std::printf("%llu cases, %llu runs\n", (unsigned long long)ncases, (unsigned long long)nruns);
    return 0;
}

static void print_plan(const ivx::Plan &p) {
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = 0; i < p.nslots; i++) {
        const uint64_t n = ivs::slot_items(p.items, p.nslots, i);
        lo = n < lo ? n : lo;
        hi = n > hi ? n : hi;
    }
    std::printf("%zu %u %u %llu %u %llu %llu %llu %u %zu\n", p.lds, p.resident, p.S, (unsigned long long)p.items, p.nslots,
                (unsigned long long)p.scratch, (unsigned long long)lo, (unsigned long long)hi, p.W, p.merge_lds);
}

int main(int argc, char **argv) {
    if (argc >= 8 && !std::strcmp(argv[1], "plan")) {
        const uint64_t nq = std::strtoull(argv[2], nullptr, 10);
        uint32_t v[5];
        for (int i = 0; i < 5; i++) v[i] = (uint32_t)std::strtoul(argv[3 + i], nullptr, 10);
        print_plan(ivx::scan_plan(v[0], v[1], v[2], nq, v[3], v[4], 0, 0));
        print_plan(ivx::range_plan(v[0], v[1], v[2], nq, v[3], 0, 0));
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "cases")) {
        const int r = run_cases();
        if (r) { std::printf("FAIL: malformed case text\n"); return r; }
    } else {
        self_checks();
    }
    if (fails) return 1;
    std::printf("ivf residual ok\n");
    return 0;
}
