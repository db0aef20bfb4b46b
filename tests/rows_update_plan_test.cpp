// Stand-alone host program: the host-side statement of csrc/rows_update.h -- the slot table (last mention wins, skipped and invalid
// nodes), where every row of the updated matrix comes from, the accepted sizes, and the re-stride of a fixed-stride record -- against
// their definitions written out the slow way.  Built by tests/test_rows_update_ref_cpu.py, plain and with the sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/rows_update.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                \
        }                                                            \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int main() {
    using namespace vidc;
    // slot table against "walk the batch, remember the last mention"
    for (int trial = 0; trial < 200; trial++) {
        const uint64_t N_old = rnd() % 70, N_new = N_old + rnd() % 5, m = rnd() % 200;
        std::vector<int64_t> nodes(m);
        for (auto &v : nodes) {
            const uint64_t r = rnd() % 10;
            v = r == 0 ? -1 - (int64_t)(rnd() % 3) : r == 1 ? (int64_t)(N_new + rnd() % 3) : (int64_t)(rnd() % (N_new ? N_new : 1));
            if (N_new == 0 && v >= 0) v = (int64_t)(rnd() % 3);  // (every non-negative node is invalid then)
        }
        std::vector<uint32_t> slot(N_new + 1, 0xdeadbeefu);  // (+1: a guard the call must not touch)
        const uint64_t invalid = rows_upd_slots_host(nodes.data(), m, N_new, slot.data());
        CHECK(slot[N_new] == 0xdeadbeefu);
        uint64_t want_invalid = 0;
        std::vector<int64_t> last(N_new, -1);
        for (uint64_t i = 0; i < m; i++) {
            if (nodes[i] < 0) continue;
            if ((uint64_t)nodes[i] >= N_new) { want_invalid++; continue; }
            last[nodes[i]] = (int64_t)i;
        }
        CHECK(invalid == want_invalid);
        for (uint64_t v = 0; v < N_new; v++) {
            CHECK(slot[v] == (uint32_t)(last[v] + 1));
            const RowsUpdSource s = rows_upd_source(slot[v], v, N_old);
            CHECK(s == (last[v] >= 0 ? RU_BATCH : v < N_old ? RU_OLD : RU_EMPTY));
        }
    }
    // sizes
    CHECK(rows_upd_sizes_ok(0, 0, 0) == 0);
    CHECK(rows_upd_sizes_ok(5, 10, 10) == 0 && rows_upd_sizes_ok(5, 10, 11) == 0);
    CHECK(rows_upd_sizes_ok(5, 10, 9) != 0);
    CHECK(rows_upd_sizes_ok(0xfffffffeull, 1, 1) == 0 && rows_upd_sizes_ok(0xffffffffull, 1, 1) != 0);
    CHECK(rows_upd_sizes_ok(1, 1, 0xfffffffeull) == 0 && rows_upd_sizes_ok(1, 1, 0xffffffffull) != 0);
    // re-stride: every (LWo, HWo) -> (LWn, HWn = HWo): a record's words land low first, then high, dropped / new words are zero
    for (uint32_t LWo = 0; LWo < 6; LWo++)
        for (uint32_t HW = 1; HW < 5; HW++)
            for (uint32_t LWn = 0; LWn < 8; LWn++) {
                std::vector<uint64_t> old(LWo + HW), out(LWn + HW);
                // (a record that is kept at a smaller LWn has zeros in the low words that go away)
                for (uint32_t w = 0; w < LWo + HW; w++) old[w] = (w < LWo && w >= LWn) ? 0 : 0x100 + w;
                for (uint32_t w = 0; w < LWn + HW; w++) {
                    const uint32_t wo = rows_upd_restride(w, LWn, LWo, HW);
                    CHECK(wo == ~0u || wo < LWo + HW);
                    out[w] = wo == ~0u ? 0 : old[wo];
                }
                for (uint32_t w = 0; w < LWn; w++) CHECK(out[w] == (w < LWo ? old[w] : 0));
                for (uint32_t h = 0; h < HW; h++) CHECK(out[LWn + h] == old[LWo + h]);
            }
    std::printf("rows update plan ok\n");
    return 0;
}
