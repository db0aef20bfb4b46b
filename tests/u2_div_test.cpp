// The 64-bit reciprocal multiply of the ROC chain encoders (U2_DIV in csrc/roc_u2.h), restated in plain C++ in csrc/u2_div_ref.h:
// hi64(B * m) in five instructions that drop the carry of the middle sum.  Checked against unsigned __int128 over the loop's
// domain (B < U2_SAFE_HI * 2^32, d >= 2); the carry must be absent there and present for one stated input outside it.  Built and
// run by tests/test_u2_div_cpu.py (g++, no HIP, no GPU).
#include <cstdio>
#include <random>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/u2_div_ref.h"

using namespace vidc;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s (line %d, d %u, B %llx)\n", #c, __LINE__, cur_d, (unsigned long long)cur_B); fails++; } } while (0)
static uint32_t cur_d;
static uint64_t cur_B;

static const uint32_t SAFE_HI = 0x7ff80000u;  // U2_SAFE_HI (roc_u2.h): the loops leave when B_hi reaches it

static uint64_t recip(uint32_t d) { return ~0ull / (uint64_t)d; }  // x, y of u2_div_entry (common.h)

// one (d, B) inside the domain: no carry, the exact high half, and the quotient / remainder contract of the loop
static void check_in_domain(uint32_t d, uint64_t B) {
    cur_d = d; cur_B = B;
    const uint64_t m = recip(d);
    const U2DivFlow f = u2_div_flow(B, m);
    const uint64_t want = (uint64_t)(((unsigned __int128)B * m) >> 64);
    CHECK(!f.carry);
    CHECK(f.q == want);
    // U2_DIV_REM: r = B - q^ d (32-bit arithmetic in the kernel) lies in [0, 2d)
    const unsigned __int128 r = (unsigned __int128)B - (unsigned __int128)f.q * d;
    CHECK(f.q <= B / d && r < 2ull * d);
    CHECK((uint32_t)B - (uint32_t)f.q * d == (uint32_t)r);
}

int main() {
    std::mt19937_64 g(20240607);
    std::vector<uint32_t> ds = {2, 3, 4, 5, 7, 63, 64, 65, 4097, 52114, 65535, 65536, 65537, 262143, 262144};
    for (int i = 0; i < 300; i++) ds.push_back(2u + (uint32_t)(g() % 262143ull));  // 2 .. 262 144 (VIDC_ROC_MAX_LIST)
    const uint64_t top = ((uint64_t)SAFE_HI << 32) - 1ull;
    std::vector<uint64_t> Bs = {0ull, 1ull, 0x7fffffffull, 0x80000000ull, 0xffffffffull, 0x100000000ull, 0x7fffffffffffull,
                                (1ull << 62) - 1ull, 1ull << 62, ((uint64_t)SAFE_HI << 32) - 0x100000000ull, top - 1ull, top};
    uint64_t pairs = 0;
    for (uint32_t d : ds) {
        for (uint64_t B : Bs) { check_in_domain(d, B); pairs++; }
        for (int i = 0; i < 2000; i++) {
            uint64_t B = g() % (top + 1ull);
            if (i & 1) B >>= (g() % 40ull);  // small heads and heads just above 2^31 are as common as large ones
            check_in_domain(d, B);
            pairs++;
        }
        // multiples of d and their neighbours: where a truncated quotient would first go wrong
        for (int i = 0; i < 200; i++) {
            const uint64_t q = g() % (top / d);
            const uint64_t near[3] = {q * d, q * d + 1u, q * d + d - 1u};
            for (uint64_t B : near)
                if (B <= top) { check_in_domain(d, B); pairs++; }
        }
    }
    // outside the domain the carry exists: B = 2^64 - 1 (>= 2^63) with d = 2 -- m = 2^63 - 1, b1 m0 = P1 = (2^32 - 1)^2 + ..., S wraps.
    // The five-instruction form is then 2^32 short of the true high half: the exit test of the loops is what makes it exact.
    {
        cur_d = 2; cur_B = ~0ull;
        const U2DivFlow f = u2_div_flow(~0ull, recip(2));
        const uint64_t want = (uint64_t)(((unsigned __int128)(~0ull) * recip(2)) >> 64);
        CHECK(f.carry);
        CHECK(f.q + (1ull << 32) == want);
    }
    // a clamped lane (divisor 1, m = 2^64 - 1) may wrap as well: no step reads such a lane (roc_u2.h, U2_DIV), pinned here as a fact
    {
        cur_d = 1; cur_B = top;
        CHECK(u2_div_flow(top, ~0ull).carry);
    }
    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("u2 div ok (%llu pairs)\n", (unsigned long long)pairs);
    return 0;
}
