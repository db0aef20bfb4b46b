// The member-row geometry of the ROC decoders as the headers compute it, for tests/test_roc_rows_ref_cpu.py to compare with
// tests/roc_rows_ref.py: reads lines "n P umax align" from standard input and prints, per line,
//   n P umax align | lane caps on 64 / 128 / 256 buckets | row-per-list bucket bits, cap | general fine bits, cap | b2_buckets_for
// Built with g++ like tests/roc_dec_plan_test.cpp (no HIP, no GPU).
#include <cstdio>

#include "../vector_db_id_compression_amd/csrc/roc_dec_plan.h"
#include "../vector_db_id_compression_amd/csrc/roc_sizing.h"

using namespace vidc;

// the kernels' limits as literals (roc.hip fills DecLimits from the headers' macros: DEC_LIMITS).  The ones b2_buckets_for reads:
// r2_min_list = 256 (roc.hip: constexpr uint64_t R2_MIN_LIST), b2l_max_list = 4096, b2l_mid_list = 2048, b2l_load = 30
// (roc_u2.h: VIDC_B2L_MAX_LIST, VIDC_B2L_MID_LIST, VIDC_B2L_LOAD)
static const DecLimits LIM{64, 4096, 4097, 256, 256, 512, 1024, 1024, 2048, 4096, 4096, 2048, 30, 8192, 8192, 2048};

int main() {
    unsigned long long n, P, umax, align;
    int rows = 0;
    while (std::scanf("%llu %llu %llu %llu", &n, &P, &umax, &align) == 4) {
        const uint32_t n32 = (uint32_t)n, P32 = (uint32_t)P, al = (uint32_t)align;
        std::printf("%llu %llu %llu %llu %u %u %u %u %u %u %u %u\n", n, P, umax, align, dev::roc_lane_cap_nb<64>(n32, al),
                    dev::roc_lane_cap_nb<128>(n32, al), dev::roc_lane_cap_nb<256>(n32, al), 8u + dev::roc_grp_dec_fbits(n32),
                    dev::roc_grp_dec_cap(n32), dev::roc_dec_fine_bits(n32, P32 > 32u ? 32u : P32), dev::roc_dec_cap(n32),
                    b2_buckets_for(n, P32, (uint32_t)umax, LIM));
        rows++;
    }
    std::printf("roc rows geometry ok %d\n", rows);
    return 0;
}
