// The plan of vidc_ivf_kmeans_step_dev (csrc/ivf_kmeans_plan.h) against a written-out table: held-whole or streamed at its boundary,
// LDS, the cut and the grid, the lanes of k_kmeans_partial, update batches, scratch, and the limits of the status list.
// Stand-alone: g++ -std=c++17 [-fsanitize=address,undefined] -I vector_db_id_compression_amd/csrc; exit status 0 and "ok <cases>".
#include <stdio.h>

#include "ivf_kmeans_plan.h"

using namespace vidc;

static unsigned cases = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                              \
        }                                                          \
        cases++;                                                   \
    } while (0)

struct Row {
    uint32_t cu;
    uint64_t n;
    uint32_t ld, G, dsub, k;
    bool whole;
    size_t lds;
    uint32_t resident, S, grid;
    bool vec;
};
struct LaneRow {
    uint32_t dsub;
    bool vec;
    uint32_t V, slots, W, side, passes;
};

int main() {
    const Row rows[] = {
        // cu, n, ld, G, dsub, k -> whole, lds, resident, S, grid, vec
        {256, 200000, 128, 1, 128, 1024, false, 36864, 512, 512, 512, true},
        {256, 200000, 128, 16, 8, 256, true, 12288, 512, 32, 512, true},
        {256, 200000, 128, 4, 32, 256, true, 36864, 512, 128, 512, true},
        {256, 700, 60, 1, 60, 256, true, 65536, 512, 6, 6, true},      // the last dsub held whole at k = 256 ...
        {256, 700, 61, 1, 61, 256, false, 36864, 512, 6, 6, false},    // ... and the first streamed (round_up(61, 4) + 4 = 68)
        {256, 700, 4, 1, 1, 2048, true, 65536, 512, 6, 6, false},      // k at the boundary, dsub = 1: rows of 8 floats
        {256, 700, 4, 1, 1, 2049, false, 36864, 512, 6, 6, false},
        {1, 700, 28, 3, 8, 256, true, 12288, 2, 1, 2, true},           // one CU: three uncut items on two workgroups
        {1, 129, 33, 1, 33, 600, false, 36864, 2, 2, 2, false},
        {256, 1, 1, 1, 1, 1, true, 32, 512, 1, 1, false},
    };
    for (const Row &r : rows) {
        const ikm::Plan p = ikm::make_plan(r.cu, r.n, r.ld, r.G, r.dsub, r.k, 16, 32);
        CHECK(p.whole == r.whole && p.lds == r.lds && p.resident == r.resident && p.S == r.S && p.grid == r.grid && p.vec == r.vec);
        CHECK(p.items == (uint64_t)r.G * r.S && p.ntiles == (r.n + 127) / 128 && p.S <= p.ntiles && p.gb == r.G);
        CHECK(!ikm::make_plan(r.cu, r.n, r.ld, r.G, r.dsub, r.k, 20, 32).vec && !ikm::make_plan(r.cu, r.n, r.ld, r.G, r.dsub, r.k, 16, 36).vec);
        CHECK(ikm::piece_tile(p.ntiles, p.S, 0) == 0 && ikm::piece_tile(p.ntiles, p.S, p.S) == p.ntiles);
        for (uint32_t s = 0; s < p.S; s++) CHECK(ikm::piece_tile(p.ntiles, p.S, s) < ikm::piece_tile(p.ntiles, p.S, s + 1));
    }
    const LaneRow lanes[] = {{1, false, 1, 1, 1, 64, 1},  {3, false, 1, 3, 4, 16, 1},    {8, false, 1, 8, 8, 8, 1},     {8, true, 4, 2, 2, 32, 1},
                             {32, false, 1, 32, 32, 2, 1}, {33, false, 1, 33, 64, 1, 1},  {128, false, 1, 128, 64, 1, 2}, {128, true, 4, 32, 32, 2, 1},
                             {132, true, 4, 33, 64, 1, 1}, {2048, true, 4, 512, 64, 1, 8}, {2047, false, 1, 2047, 64, 1, 32}};
    for (const LaneRow &l : lanes) {
        const ikm::Lanes g = ikm::partial_lanes(l.dsub, l.vec);
        CHECK(g.V == l.V && g.slots == l.slots && g.W == l.W && g.side == l.side && g.passes == l.passes && g.W * g.side == 64);
    }
    // update batches, key bits, the chunk bound and the scratch formula
    CHECK(ikm::batch_groups(200000, 16) == 16 && ikm::batch_groups(1ull << 26, 16) == 1 && ikm::batch_groups(1ull << 25, 16) == 2);
    CHECK(ikm::batch_groups((1ull << 32) - 1, 16) == 1 && ikm::batch_groups(1, 1) == 1 && ikm::batch_groups((1ull << 26) + 1, 3) == 1);
    CHECK(ikm::key_bits(1) == 0 && ikm::key_bits(2) == 1 && ikm::key_bits(256) == 8 && ikm::key_bits(257) == 9 && ikm::key_bits(1u << 24) == 24);
    CHECK(ikm::chunk_bound(1027, 7) == 11 && ikm::chunk_bound(0, 1) == 1);
    CHECK(ikm::scratch_bytes(1024, 1, 4, 2, false) == 8 + 16 * 1024 + 3072 + 8 + 16 * 3 + 8 * 7 + 16 * 6);
    CHECK(ikm::scratch_bytes(1024, 1, 4, 2, true) == ikm::scratch_bytes(1024, 1, 4, 2, false) + 4096);

    // the status list
    int live = 0;
    const void *p = &live, *q = &cases;
    const ikm::Args ok = {5, p, 8, 2, 4, 3, p, q};
    CHECK(ikm::check_args(ok) == nullptr);
    ikm::Args a = ok;
    a.x = nullptr; CHECK(ikm::check_args(a)); a = ok;
    a.c_in = nullptr; CHECK(ikm::check_args(a)); a = ok;
    a.c_out = nullptr; CHECK(ikm::check_args(a)); a = ok;
    a.n = 0; a.x = a.c_in = a.c_out = nullptr; CHECK(ikm::check_args(a) == nullptr); a = ok;
    a.G = 0; CHECK(ikm::check_args(a)); a = ok;
    a.k = 0; CHECK(ikm::check_args(a)); a = ok;
    a.dsub = 0; CHECK(ikm::check_args(a)); a = ok;
    a.dsub = 2049; a.ld = 5000; CHECK(ikm::check_args(a)); a.dsub = 2048; CHECK(ikm::check_args(a) == nullptr); a = ok;
    a.ld = 7; CHECK(ikm::check_args(a)); a = ok;
    a.G = 1; a.k = (1u << 24) + 1; CHECK(ikm::check_args(a)); a.k = 1u << 24; CHECK(ikm::check_args(a) == nullptr); a = ok;
    a.G = 0xffffffffu; a.dsub = 2; a.ld = 0xffffffffu; CHECK(ikm::check_args(a)); a = ok;  // (G * dsub does not wrap)
    a.n = 1ull << 32; CHECK(ikm::check_args(a)); a.n = (1ull << 32) - 1; CHECK(ikm::check_args(a) == nullptr); a = ok;
    a.c_out = a.c_in; CHECK(ikm::check_args(a));
    printf("ok %u\n", cases);
    return 0;
}
