// The plan of vidc_ivf_probe_dev (csrc/ivf_probe_plan.h) over a grid of shapes: LDS, pools, the cut, the piece bounds, the scratch.
// Stand-alone: g++ -std=c++17 [-fsanitize=address,undefined] -I vector_db_id_compression_amd/csrc; exit status 0 and "ok <cases>".
#include <stdio.h>
#include <stdlib.h>

#include "ivf_probe_plan.h"

using namespace vidc;

#define CHECK(c)                                                                                                              \
    do {                                                                                                                      \
        if (!(c)) {                                                                                                           \
            fprintf(stderr, "%s:%d: %s (cu %u nq %llu nlist %llu nprobe %u d %u)\n", __FILE__, __LINE__, #c, cu, (unsigned long long)nq, \
                    (unsigned long long)nlist, nprobe, d);                                                                    \
            return 1;                                                                                                         \
        }                                                                                                                     \
    } while (0)

int main() {
    const uint32_t cus[] = {1, 256}, nprobes[] = {1, 16, 64, 65, 256}, ds[] = {1, 3, 4, 130, 2048};
    const uint64_t nqs[] = {1, 3, 17, 100, 163, 10000, (1ull << 32) - 1}, nlists[] = {1, 127, 128, 129, 1000, 5000, 65536, (1ull << 31) - 1};
    unsigned cases = 0;
    for (uint32_t cu : cus)
        for (uint64_t nq : nqs)
            for (uint64_t nlist : nlists)
                for (uint32_t nprobe : nprobes)
                    for (uint32_t d : ds) {
                        const ivp::Args ok = {nlist, &cases, d, nq, &cases, nprobe, &cases};
                        CHECK(ivp::check_args(ok) == nullptr);
                        const ivp::Plan p = ivp::make_plan(cu, nlist, d, nq, nprobe, 16, 32);
                        CHECK(p.TQ == (nprobe <= 64 ? 32u : 16u) && p.vec == (d % 4 == 0));
                        CHECK(!ivp::make_plan(cu, nlist, d, nq, nprobe, 20, 32).vec && !ivp::make_plan(cu, nlist, d, nq, nprobe, 16, 4).vec);
                        CHECK(p.lds <= ivs::LDS_PER_CU && p.lds % 16 == 0);
                        CHECK((size_t)p.TQ * 2 * nprobe * 8 == ivp::pool_bytes(p.TQ, nprobe) && ivp::pool_bytes(p.TQ, nprobe) < p.lds);
                        CHECK(p.resident >= cu && p.resident <= cu * 8 && p.resident * p.lds <= cu * ivs::LDS_PER_CU);
                        CHECK(p.S >= 1 && p.S <= 256 && (p.S & (p.S - 1)) == 0);
                        CHECK(p.qtiles == (nq + p.TQ - 1) / p.TQ && p.ntiles == (nlist + 127) / 128 && p.items == p.qtiles * p.S);
                        // the smallest S that fills the resident workgroups, as far as the tiles go
                        CHECK(p.S == 1 || (p.qtiles * (p.S / 2) < p.resident && p.S <= p.ntiles));
                        CHECK(p.S == 256 || p.qtiles * p.S >= p.resident || (uint64_t)p.S * 2 > p.ntiles);
                        CHECK(p.grid >= 1 && p.grid <= p.resident && p.grid <= p.items);
                        // the pieces tile [0, nlist): no gap, no overlap, whole tiles, none empty
                        CHECK(ivp::piece_begin(nlist, p.S, 0) == 0 && ivp::piece_begin(nlist, p.S, p.S) == nlist);
                        for (uint32_t s = 0; s < p.S; s++) {
                            const uint64_t a = ivp::piece_begin(nlist, p.S, s), b = ivp::piece_begin(nlist, p.S, s + 1);
                            CHECK(a < b && a % ivp::TC == 0 && (b % ivp::TC == 0 || b == nlist));
                            CHECK(a == ivp::piece_tile(p.ntiles, p.S, s) * ivp::TC);
                        }
                        CHECK(p.scratch == (p.S > 1 ? nq * p.S * nprobe * 8 : 0));
                        CHECK(p.S == 1 || p.scratch <= (1ull << 32));  // (a cut call is a small batch)
                        cases++;
                    }
    printf("ok %u\n", cases);
    return 0;
}
