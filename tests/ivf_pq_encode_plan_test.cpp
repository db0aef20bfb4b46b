// The plan of vidc_ivf_pq_encode_dev (csrc/ivf_pq_encode_plan.h) over a grid of shapes: LDS, the cut, the piece bounds, the grid.
// Stand-alone: g++ -std=c++17 [-fsanitize=address,undefined] -I vector_db_id_compression_amd/csrc; exit status 0 and "ok <cases>".
#include <stdio.h>

#include "ivf_pq_encode_plan.h"

using namespace vidc;

#define CHECK(c)                                                                                                                      \
    do {                                                                                                                              \
        if (!(c)) {                                                                                                                   \
            fprintf(stderr, "%s:%d: %s (cu %u n %llu dsub %u M %u)\n", __FILE__, __LINE__, #c, cu, (unsigned long long)n, dsub, M); \
            return 1;                                                                                                                 \
        }                                                                                                                             \
    } while (0)

int main() {
    const uint32_t cus[] = {1, 256}, dsubs[] = {1, 3, 4, 8, 17, 64, 65, 128}, Ms[] = {1, 2, 5, 16};
    const uint64_t ns[] = {1, 127, 128, 129, 300, 10000, 1000000, (1ull << 32) - 1};
    unsigned cases = 0;
    for (uint32_t cu : cus)
        for (uint64_t n : ns)
            for (uint32_t dsub : dsubs)
                for (uint32_t M : Ms) {
                    const uint32_t d = dsub * M;
                    const ipe::Args ok = {n, &cases, d, M, &cases, 0, nullptr, nullptr, &cases};
                    CHECK(ipe::check_args(ok) == nullptr);
                    const ipe::Plan p = ipe::make_plan(cu, n, d, M, 16, 32, 0);
                    CHECK(p.dsub == dsub && p.vec == (d % 4 == 0 && dsub % 4 == 0));
                    CHECK(!ipe::make_plan(cu, n, d, M, 20, 32, 0).vec && !ipe::make_plan(cu, n, d, M, 16, 32, 4).vec);
                    CHECK(p.lds == (size_t)1024 * (((dsub + 3) & ~3u) + 5) && p.lds <= ivs::LDS_PER_CU && p.lds % 16 == 0);
                    CHECK(p.resident >= cu && p.resident <= cu * ipe::MAX_WG_PER_CU && p.resident * p.lds <= cu * ivs::LDS_PER_CU);
                    CHECK(p.ntiles == (n + ipe::TV - 1) / ipe::TV && p.S >= 1 && p.S <= p.ntiles && p.items == (uint64_t)M * p.S);
                    // the smallest S that covers the resident workgroups, as far as the tiles go
                    CHECK(p.items >= p.resident || p.S == p.ntiles);
                    CHECK(p.S == 1 || (uint64_t)M * (p.S - 1) < p.resident);
                    CHECK(p.grid >= 1 && p.grid <= p.resident && p.grid <= p.items);
                    // the pieces tile [0, ntiles), so the vectors [0, n): no gap, no overlap, none empty
                    CHECK(ipe::piece_tile(p.ntiles, p.S, 0) == 0 && ipe::piece_tile(p.ntiles, p.S, p.S) == p.ntiles);
                    CHECK(p.ntiles * ipe::TV >= n && (p.ntiles - 1) * ipe::TV < n);
                    for (uint32_t s = 0; s < p.S; s++)  // (S <= the resident workgroups)
                        CHECK(ipe::piece_tile(p.ntiles, p.S, s) < ipe::piece_tile(p.ntiles, p.S, s + 1));
                    cases++;
                }
    printf("ok %u\n", cases);
    return 0;
}
