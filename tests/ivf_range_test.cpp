// Stand-alone check of csrc/ivf_range_ref.h and csrc/ivf_range_plan.h (g++, no HIP): the serial count and fill built from the rules
// against cases the numpy model writes out (tests/ivf_range_ref.py), as one piece and as S pieces for every S, every array in an
// allocation of its exact size so that a sanitizer build sees any read or write outside it; the place and the write-bound rule
// under slot limits of another radius and short capacities; the argument checks and the plan's figures.
//   ivf_range_test                                  self checks
//   ivf_range_test cases < text                     the model's cases
//   ivf_range_test plan nq num_cu kind d M nprobe   prints: lds resident S items nslots min_items max_items G V W count_bytes
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/ivf_range_plan.h"
#include "../vector_db_id_compression_amd/csrc/ivf_range_ref.h"

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
    // slots, hits, places, the write bound
    CHECK(ivr::slot_of(0, 16, 0) == 0 && ivr::slot_of(3, 16, 5) == 53 && ivr::slot_of(4194303, 1024, 1023) == 0xffffffffull);
    CHECK(ivr::is_hit(1.f, 1.5f) && !ivr::is_hit(1.f, 1.f) && !ivr::is_hit(2.f, 1.f) && !ivr::is_hit(0.f, 0.f) && !ivr::is_hit(0.f, -1.f));
    CHECK(ivr::is_hit(3e38f, INFINITY) && !ivr::is_hit(INFINITY, INFINITY) && !ivr::is_hit(0.f, NAN) && !ivr::is_hit(NAN, 1.f));
    CHECK(ivr::is_hit(0.f, 1e-45f));
    CHECK(ivr::hit_place(10, 0, 0) == 10 && ivr::hit_place(10, 64, 3) == 77 && ivr::hit_place(1ull << 40, 128, 63) == (1ull << 40) + 191);
    CHECK(ivr::place_written(5, 6, 6) && !ivr::place_written(6, 6, 100) && !ivr::place_written(5, 100, 5) && !ivr::place_written(0, 0, 0));
    CHECK(!ivr::place_written(7, 3, 100));  // slot limits that decrease: nothing is written
    // argument checks
    int dummy = 0;
    const void *p = &dummy;
    const ivr::Args ok = {16, p, 2000, p, ivs::PQ8, 128, 16, p, 5, p, 4, p, p};
    CHECK(ivr::check_count(ok) == nullptr && ivr::check_fill(ok, 10, p, p) == nullptr && ivr::check_fill(ok, 0, nullptr, nullptr) == nullptr);
    auto refused = [&](void (*edit)(ivr::Args &)) {
        ivr::Args a = ok;
        edit(a);
        return ivr::check_count(a) != nullptr && ivr::check_fill(a, 10, p, p) != nullptr;
    };
    CHECK(refused([](ivr::Args &a) { a.offsets = nullptr; }) && refused([](ivr::Args &a) { a.codes = nullptr; }));
    CHECK(refused([](ivr::Args &a) { a.xq = nullptr; }) && refused([](ivr::Args &a) { a.probes = nullptr; }));
    CHECK(refused([](ivr::Args &a) { a.slot_lims = nullptr; }));
    CHECK(refused([](ivr::Args &a) { a.nprobe = 0; }) && refused([](ivr::Args &a) { a.nprobe = 1025; }));
    CHECK(refused([](ivr::Args &a) { a.d = 0; }) && refused([](ivr::Args &a) { a.d = 2049; }));
    CHECK(refused([](ivr::Args &a) { a.ntotal = 1ull << 32; }) && refused([](ivr::Args &a) { a.nlist = 1ull << 31; }));
    CHECK(refused([](ivr::Args &a) { a.kind = 2; }) && refused([](ivr::Args &a) { a.kind = -1; }) && refused([](ivr::Args &a) { a.M = 0; }));
    CHECK(refused([](ivr::Args &a) { a.M = 65; a.d = 65; }) && refused([](ivr::Args &a) { a.M = 3; }) && refused([](ivr::Args &a) { a.codebooks = nullptr; }));
    // nq * nprobe >= 2^32 - 1
    CHECK(refused([](ivr::Args &a) { a.nq = 0xffffffffull; a.nprobe = 1; }) && !refused([](ivr::Args &a) { a.nq = 0xfffffffeull; a.nprobe = 1; }));
    CHECK(refused([](ivr::Args &a) { a.nq = 1ull << 22; a.nprobe = 1024; }) && !refused([](ivr::Args &a) { a.nq = (1ull << 22) - 1; a.nprobe = 1024; }));
    CHECK(refused([](ivr::Args &a) { a.nq = 1431655765; a.nprobe = 3; }) && !refused([](ivr::Args &a) { a.nq = 1431655764; a.nprobe = 3; }));
    CHECK(refused([](ivr::Args &a) { a.nq = ~0ull; }) && refused([](ivr::Args &a) { a.nq = 1ull << 62; a.nprobe = 4; }));
    CHECK(ivr::check_fill(ok, 1, nullptr, p) != nullptr && ivr::check_fill(ok, 1, p, nullptr) != nullptr);
    const ivr::Args none = {16, nullptr, 2000, nullptr, ivs::FLAT, 7, 0, nullptr, 0, nullptr, 4, nullptr, nullptr};  // nq == 0
    CHECK(ivr::check_count(none) == nullptr && ivr::check_fill(none, 0, nullptr, nullptr) == nullptr);
    ivr::Args none_bad = none;
    none_bad.kind = 5;
    CHECK(ivr::check_count(none_bad) != nullptr);  // (the limits still hold)
    // plan
    CHECK(ivr::lds_bytes(ivs::PQ8, 16, 128, 16) == 16960 && ivr::lds_bytes(ivs::PQ8, 1024, 2048, 64) == 77824);
    CHECK(ivr::lds_bytes(ivs::FLAT, 16, 32, 0) == 448 && ivr::lds_bytes(ivs::FLAT, 1024, 2048, 0) == 256 + 4096 + 8192);
    CHECK(ivr::lds_bytes(ivs::FLAT, 1, 1, 0) == 256 + 16 + 16 && ivr::head_bytes(ivs::FLAT, 7) % 16 == 0 && ivr::head_bytes(ivs::PQ8, 7) == 32);
    CHECK(ivr::count_bytes(10, 16) == 640);
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

struct Case {
    uint64_t nlist, ntotal, kind, d, M, nq, nprobe, total;
    float radius;
    std::unique_ptr<uint64_t[]> off, lims;
    std::unique_ptr<uint8_t[]> codes;
    std::unique_ptr<float[]> cb, xq, wantD;
    std::unique_ptr<int64_t[]> probes;
    std::unique_ptr<long long[]> wantL;
};

// the serial count of a whole batch, every query cut into S pieces -> counts[nq * nprobe] (poisoned first: every slot must be written)
static void count_all(const Case &c, float radius, uint32_t S, uint32_t *counts) {
    for (uint64_t i = 0; i < c.nq * c.nprobe; i++) counts[i] = 0xdeadbeefu;
    for (uint64_t q = 0; q < c.nq; q++)
        for (uint32_t s = 0; s < S; s++) {
            auto row = exact<int32_t>(c.nprobe);
            auto table = exact<float>(c.kind == ivs::PQ8 ? c.M * 256 : 0);
            ivr::count_serial(c.nlist, c.off.get(), c.ntotal, c.codes.get(), (int)c.kind, (uint32_t)c.d, (uint32_t)c.M, c.cb.get(),
                              c.xq.get() + q * c.d, (uint32_t)c.nprobe, c.probes.get() + q * c.nprobe, radius, S, s, row.get(), table.get(),
                              counts + q * c.nprobe);
        }
}
static void fill_all(const Case &c, float radius, uint32_t S, const uint64_t *lims, uint64_t capacity, float *D, int64_t *L) {
    for (uint64_t i = 0; i < capacity; i++) {
        D[i] = POISON_D;
        L[i] = POISON_L;
    }
    for (uint64_t q = 0; q < c.nq; q++)
        for (uint32_t s = 0; s < S; s++) {
            auto row = exact<int32_t>(c.nprobe);
            auto table = exact<float>(c.kind == ivs::PQ8 ? c.M * 256 : 0);
            ivr::fill_serial(c.nlist, c.off.get(), c.ntotal, c.codes.get(), (int)c.kind, (uint32_t)c.d, (uint32_t)c.M, c.cb.get(),
                             c.xq.get() + q * c.d, (uint32_t)c.nprobe, c.probes.get() + q * c.nprobe, radius, S, s, row.get(), table.get(),
                             lims + q * c.nprobe, capacity, D, L);
        }
}

static int run_cases() {
    uint64_t ncases = 0, nruns = 0, nbound = 0;
    if (!read_u64(ncases)) return 2;
    for (uint64_t ci = 0; ci < ncases; ci++) {
        Case c;
        if (!(read_u64(c.nlist) && read_u64(c.ntotal) && read_u64(c.kind) && read_u64(c.d) && read_u64(c.M) && read_u64(c.nq) && read_u64(c.nprobe) &&
              read_f32(c.radius) && read_u64(c.total)))
            return 2;
        const uint64_t code_size = c.kind == ivs::PQ8 ? c.M : c.d * 4, nslots = c.nq * c.nprobe;
        c.off = exact<uint64_t>(c.nlist + 1);
        c.codes = exact<uint8_t>(c.ntotal * code_size);
        c.cb = exact<float>(c.kind == ivs::PQ8 ? 256 * c.d : 0);
        c.xq = exact<float>(c.nq * c.d);
        c.probes = exact<int64_t>(nslots);
        c.lims = exact<uint64_t>(nslots + 1);
        c.wantD = exact<float>(c.total);
        c.wantL = exact<long long>(c.total);
        for (uint64_t i = 0; i <= c.nlist; i++) if (!read_u64(c.off[i])) return 2;
        for (uint64_t i = 0; i < c.ntotal * code_size; i++) {
            unsigned b;
            if (std::scanf("%u", &b) != 1) return 2;
            c.codes[i] = (uint8_t)b;
        }
        if (c.kind == ivs::PQ8) for (uint64_t i = 0; i < 256 * c.d; i++) if (!read_f32(c.cb[i])) return 2;
        for (uint64_t i = 0; i < c.nq * c.d; i++) if (!read_f32(c.xq[i])) return 2;
        for (uint64_t i = 0; i < nslots; i++) {
            long long v;
            if (std::scanf("%lld", &v) != 1) return 2;
            c.probes[i] = v;
        }
        for (uint64_t i = 0; i <= nslots; i++) if (!read_u64(c.lims[i])) return 2;
        for (uint64_t i = 0; i < c.total; i++) if (!read_f32(c.wantD[i])) return 2;
        for (uint64_t i = 0; i < c.total; i++) if (std::scanf("%lld", &c.wantL[i]) != 1) return 2;
        const ivr::Args args = {c.nlist, c.off.get(), c.ntotal, c.codes.get(), (int)c.kind, (uint32_t)c.d, (uint32_t)c.M, c.cb.get(), c.nq,
                                c.xq.get(), (uint32_t)c.nprobe, c.probes.get(), c.lims.get()};
        if (ivr::check_count(args) || c.lims[nslots] != c.total) {
            std::printf("FAIL case %llu: refused or malformed\n", (unsigned long long)ci);
            fails++;
            continue;
        }
        for (uint32_t S = 1; S <= ivs::MAX_S; S *= 2) {
            // count: every slot written, the prefix sum is the model's
            auto counts = exact<uint32_t>(nslots);
            count_all(c, c.radius, S, counts.get());
            bool same = true;
            uint64_t acc = 0;
            for (uint64_t s = 0; s < nslots; s++) {
                same = same && acc == c.lims[s];
                acc += counts[s];
            }
            same = same && acc == c.total;
            // fill at the exact capacity: every place written, nothing else exists
            auto D = exact<float>(c.total);
            auto L = exact<int64_t>(c.total);
            fill_all(c, c.radius, S, c.lims.get(), c.total, D.get(), L.get());
            for (uint64_t i = 0; i < c.total; i++) same = same && same_f32(D[i], c.wantD[i]) && L[i] == c.wantL[i];
            if (!same) {
                std::printf("FAIL case %llu S %u: count or fill differs from the model\n", (unsigned long long)ci, S);
                fails++;
            }
            nruns++;
        }
        // the write bound, serially: short capacities, and the slot limits of this radius under a larger radius (+inf: every
        // candidate is a hit, every slot holds its first hits) -- the arrays have exactly `cap` entries
        const uint64_t caps[4] = {c.total, c.total ? c.total - 1 : 0, c.total / 2, 0};
        for (uint64_t cap : caps) {
            auto D = exact<float>(cap);
            auto L = exact<int64_t>(cap);
            fill_all(c, c.radius, 4, c.lims.get(), cap, D.get(), L.get());
            bool same = true;
            for (uint64_t i = 0; i < cap; i++) same = same && same_f32(D[i], c.wantD[i]) && L[i] == c.wantL[i];
            fill_all(c, INFINITY, 1, c.lims.get(), cap, D.get(), L.get());
            for (uint64_t i = 0; i < cap; i++) same = same && !same_f32(D[i], POISON_D) && L[i] != POISON_L;  // (full slots, in bounds)
            if (!same) {
                std::printf("FAIL case %llu capacity %llu: the bounded fill differs\n", (unsigned long long)ci, (unsigned long long)cap);
                fails++;
            }
            nbound++;
        }
        // the slot limits of this radius under a radius of 0: nothing is a hit, nothing is written
        {
            auto D = exact<float>(c.total);
            auto L = exact<int64_t>(c.total);
            fill_all(c, 0.f, 2, c.lims.get(), c.total, D.get(), L.get());
            for (uint64_t i = 0; i < c.total; i++) CHECK(same_f32(D[i], POISON_D) && L[i] == POISON_L);
        }
    }
    std::printf("%llu cases, %llu runs, %llu bounded fills\n", (unsigned long long)ncases, (unsigned long long)nruns, (unsigned long long)nbound);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 8 && !std::strcmp(argv[1], "plan")) {
        const uint64_t nq = std::strtoull(argv[2], nullptr, 10);
        uint32_t v[5];
        for (int i = 0; i < 5; i++) v[i] = (uint32_t)std::strtoul(argv[3 + i], nullptr, 10);
        const ivr::Plan p = ivr::make_plan(v[0], (int)v[1], v[2], v[3], nq, v[4], 0, 0);
        uint64_t lo = ~0ull, hi = 0;
        for (uint32_t i = 0; i < p.nslots; i++) {
            const uint64_t n = ivs::slot_items(p.items, p.nslots, i);
            lo = n < lo ? n : lo;
            hi = n > hi ? n : hi;
        }
        std::printf("%zu %u %u %llu %u %llu %llu %u %u %u %llu\n", p.lds, p.resident, p.S, (unsigned long long)p.items, p.nslots,
                    (unsigned long long)lo, (unsigned long long)hi, p.grp.G, p.grp.V, p.W, (unsigned long long)ivr::count_bytes(nq, v[4]));
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "cases")) {
        const int r = run_cases();
        if (r) { std::printf("FAIL: malformed case text\n"); return r; }
    } else {
        self_checks();
    }
    if (fails) return 1;
    std::printf("ivf range ok\n");
    return 0;
}
