// ef_rank_test.cpp -- csrc/ef_rank_ref.h on the host (g++, no HIP): the arithmetic the rank kernels of ef.hip call, against cases the
// numpy model (tests/ef_rank_ref.py) writes out, plus self-checks that need no input.
//
//   ef_rank_test                 self-checks: select_in_word against a bit walk, the directory tie rule, low_field at the stream's end,
//                                the clamp
//   ef_rank_test cases < text    per list `L m l u nlw nhw nb nq`, low words, high words, directory, then nq lines `x rank found`:
//                                rank_serial (the arena kernel's body) and the 16-lane form of the select (k_ef_rank_g16's scan, restated
//                                here lane by lane) must both give the model's answer
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/ef_rank_ref.h"

using namespace vidc::efr;

static int fails = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            if (fails++ < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                              \
    } while (0)

// ef_g16_select0 of ef.hip, lane by lane: lane j holds words 4j .. 4j + 3 of the batch, an inclusive scan of the 16 sums, the first
// lane whose sum exceeds `need` walks its four words
static uint64_t select0_g16(const uint64_t *hw, uint64_t nhw, const uint32_t *hr, uint64_t nb, uint64_t jz) {
    const uint64_t k = batch_of_zero(hr, nb, jz);
    const uint64_t need = jz - zeros_before_batch(k, hr[k]);
    uint64_t z[16][4];
    uint32_t c[16], incl[16];
    for (uint32_t j = 0; j < 16; j++) {
        c[j] = 0;
        for (int i = 0; i < 4; i++) { z[j][i] = zero_word(hw, nhw, k * 64 + 4u * j + i); c[j] += popc(z[j][i]); }
        incl[j] = c[j] + (j ? incl[j - 1] : 0u);
    }
    for (uint32_t j = 0; j < 16; j++) {
        if ((uint64_t)incl[j] > need) {
            uint32_t kk = (uint32_t)need - (incl[j] - c[j]);
            int ws = 0;
            while (ws < 3 && kk >= popc(z[j][ws])) { kk -= popc(z[j][ws]); ws++; }
            return (k * 64 + 4u * j + ws) * 64 + select_in_word(z[j][ws], kk);
        }
    }
    return nhw * 64;
}

static void self_checks() {
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (int t = 0; t < 2000; t++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        uint64_t w = t == 0 ? 1ull : t == 1 ? 1ull << 63 : t == 2 ? ~0ull : t % 5 == 0 ? s & (s >> 3) & (s << 5) : s;
        if (!w) continue;
        uint32_t k = 0;
        for (uint32_t b = 0; b < 64; b++)
            if (w >> b & 1) { CHECK(select_in_word(w, k) == b); k++; }
        CHECK(select_in_word(w, 64) <= 63);  // (a k beyond the popcount stays inside the word)
    }
    // batches 1 and 2 hold ones only: they tie with batch 3, which holds the zero
    const uint32_t hr[5] = {0, 4086, 8182, 12278, 12300};
    CHECK(batch_of_zero(hr, 5, 9) == 0 && batch_of_zero(hr, 5, 10) == 3 && batch_of_zero(hr, 5, 4083) == 3 && batch_of_zero(hr, 5, 4084) == 4);
    CHECK(batch_of_zero(hr, 1, 1000000) == 0);
    // low_field: a field that crosses the last word reads zeros behind it, a position behind the stream reads zero
    const uint64_t low[2] = {0xf000000000000000ull, 0x5ull};
    CHECK(low_field(low, 2, 60, 8) == 0x5f && low_field(low, 1, 60, 8) == 0x0f && low_field(low, 2, 124, 8) == 0 && low_field(low, 2, 128, 8) == 0);
    CHECK(low_field(low, 2, 0, 0) == 0 && low_field(low, 2, 0, 63) == 0x7000000000000000ull);
    // the clamp keeps a bucket inside the list whatever the positions were
    Bucket b = ef_rank_clamp(10, 5, 3, 100);
    CHECK(b.r0 == 7 && b.c == 0);
    b = ef_rank_clamp(1000, 5000, 3, 100);
    CHECK(b.r0 == 100 && b.c == 0);
    b = ef_rank_clamp(50, 5000, 3, 100);
    CHECK(b.r0 == 47 && b.c == 53);
    b = ef_rank_clamp(2, 9, 5, 100);
    CHECK(b.r0 == 0 && b.c == 7);
}

static int run_cases() {
    uint64_t m, u, nlw, nhw, nb, nq, lists = 0, total = 0;
    uint32_t l;
    char tag[8];
    while (std::scanf("%7s %" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, tag, &m, &l, &u, &nlw, &nhw, &nb, &nq) == 8) {
        if (std::strcmp(tag, "L") != 0) { std::printf("bad case header\n"); return 2; }
        // (each array in its own allocation of its exact size: the address sanitizer sees a read one word behind any of them)
        std::vector<uint64_t> low(nlw), high(nhw);
        std::vector<uint32_t> hr(nb);
        for (auto &w : low) if (std::scanf("%" SCNu64, &w) != 1) return 2;
        for (auto &w : high) if (std::scanf("%" SCNu64, &w) != 1) return 2;
        for (auto &w : hr) if (std::scanf("%" SCNu32, &w) != 1) return 2;
        for (uint64_t q = 0; q < nq; q++) {
            uint64_t x, want_r;
            uint32_t want_f;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu32, &x, &want_r, &want_f) != 3) return 2;
            const RankResult a = rank_serial(low.data(), nlw, high.data(), nhw, hr.data(), nb, m, l, u, x);
            if (a.rank != want_r || a.found != want_f) {
                if (fails++ < 20) std::printf("FAIL list %" PRIu64 " x %" PRIu64 ": serial %" PRIu64 "/%u, model %" PRIu64 "/%u\n", lists, x, a.rank, a.found, want_r, want_f);
            }
            if (x <= u) {  // the group form of the two selects, then the same bucket search
                const uint64_t h = x >> l;
                const uint64_t p0 = h ? select0_g16(high.data(), nhw, hr.data(), nb, h - 1) + 1 : 0;
                const uint64_t p1 = select0_g16(high.data(), nhw, hr.data(), nb, h);
                const RankResult g = rank_in_bucket(low.data(), nlw, l, m, x, p0, p1);
                if (g.rank != want_r || g.found != want_f) {
                    if (fails++ < 20) std::printf("FAIL list %" PRIu64 " x %" PRIu64 ": group %" PRIu64 "/%u, model %" PRIu64 "/%u\n", lists, x, g.rank, g.found, want_r, want_f);
                }
                // no directory (the arena rows): the walk from word 0 finds the same zeros in a one-batch list
                if (nb == 1) CHECK(select0_serial(high.data(), nhw, nullptr, 0, h) == p1);
            }
            total++;
        }
        lists++;
    }
    std::printf("%" PRIu64 " lists, %" PRIu64 " queries\n", lists, total);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "cases")) {
        const int rc = run_cases();
        if (rc) return rc;
    } else {
        self_checks();
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ef rank ok\n");
    return 0;
}
