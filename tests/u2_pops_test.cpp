// The slice pops of the k_roc_decode_u2 step (csrc/roc_u2.h, U2_DEC_TOP_P), restated in csrc/u2_pops_ref.h: the one-test, one-shift
// form against the two pops of codec.cpp:78-90 -- head, id, words popped and refill class -- for every precision 1 .. 20, heads on both
// sides of every threshold and random heads; then a whole synthetic decode (random stream words, uniform ranks), in which no step may
// refill twice and whose per-class frequencies are printed.  Built and run by tests/test_u2_pops_cpu.py (g++, no HIP, no GPU).
// usage: u2_pops_test            the checks
//        u2_pops_test eval N     N lines "head w P" on stdin -> "head x popped class" of both forms (the Python port is checked with it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/u2_pops_ref.h"

using namespace vidc;

static int fails = 0;
static uint64_t cur_head;
static uint32_t cur_P;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s (line %d, P %u, head %llx)\n", #c, __LINE__, cur_P, (unsigned long long)cur_head); fails++; } } while (0)

static const uint64_t L = 1ull << 31;  // rans_l

struct Words {  // a stack the pops take their words from: w0 first, w1 second
    uint32_t w[2];
    uint32_t taken = 0;
    uint32_t operator()() { return w[taken++ & 1u]; }
};

static U2Pops check_pair(uint64_t head, uint32_t w0, uint32_t w1, uint32_t P) {
    cur_head = head; cur_P = P;
    const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P);
    Words ws; ws.w[0] = w0; ws.w[1] = w1;
    const U2Pops a = u2_pops_two(head, p1, p0, ws);
    const U2Pops b = u2_pops_one(head, w0, p1, p0);
    CHECK(a.cls != U2_POP_BOTH && a.popped <= 1u);
    CHECK(a.head == b.head);
    CHECK(a.x == b.x);
    CHECK(a.popped == b.popped);
    CHECK(a.cls == b.cls);
    CHECK(a.head >= L);
    CHECK(a.x < (1ull << P));
    // the class is a function of head' alone
    const uint32_t want = head < (1ull << (31u + p1)) ? U2_POP_SLICE1 : head < (1ull << (31u + p1 + p0)) ? U2_POP_SLICE0 : U2_POP_NONE;
    CHECK(a.cls == want);
    return a;
}

// one synthetic decode: n steps of (two pops, index push of a uniform rank with nmax = i + 1: codec.cpp:44-63) on a stack of random words
struct Freq { uint64_t cls[4] = {0, 0, 0, 0}, undone = 0, slice1_after_renorm = 0, slice1 = 0, steps = 0; };
static Freq synthetic(uint32_t n, uint32_t P, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::vector<uint32_t> st(4u * n + 64u);
    for (auto &w : st) w = (uint32_t)g();
    uint64_t head = L;
    const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P);
    Freq f;
    bool renorm_before = false;
    for (uint32_t i = 0; i < n; i++) {
        cur_head = head; cur_P = P;
        const size_t sp0 = st.size();
        auto pop = [&]() { const uint32_t w = st.back(); st.pop_back(); return w; };
        const uint32_t w = st.back();
        const U2Pops b = u2_pops_one(head, w, p1, p0);
        const U2Pops a = u2_pops_two(head, p1, p0, pop);
        CHECK(a.cls != U2_POP_BOTH && a.popped <= 1u);  // no step refills twice
        CHECK(a.head == b.head && a.x == b.x && a.popped == b.popped && a.cls == b.cls);
        CHECK(sp0 - st.size() == a.popped);
        f.cls[a.cls]++; f.steps++;
        if (a.cls == U2_POP_SLICE1) { f.slice1++; if (renorm_before) f.slice1_after_renorm++; }
        head = a.head;
        const uint64_t nmax = (uint64_t)i + 1u, rank = g() % nmax;
        renorm_before = false;
        if (head >= ((L / nmax) << 32)) {
            st.push_back((uint32_t)head);
            if (a.cls == U2_POP_SLICE0) { CHECK((uint32_t)head == w && st.size() == sp0); f.undone++; }  // the same word, back in its slot
            head >>= 32;
            renorm_before = true;
        }
        head = head * nmax + rank;
        if (head < L) { head = (uint64_t)pop() | (head << 32); }
        CHECK(head >= L);
    }
    return f;
}

static int eval_mode(int n) {
    for (int i = 0; i < n; i++) {
        unsigned long long head; unsigned w, P;
        if (std::scanf("%llu %u %u", &head, &w, &P) != 3) return 1;
        const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P);
        Words ws; ws.w[0] = w; ws.w[1] = ~w;
        const U2Pops a = u2_pops_two(head, p1, p0, ws), b = u2_pops_one(head, w, p1, p0);
        std::printf("%llu %u %u %u %llu %u %u %u\n", (unsigned long long)a.head, a.x, a.popped, a.cls, (unsigned long long)b.head, b.x, b.popped, b.cls);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 2 && !std::strcmp(argv[1], "eval")) return eval_mode(std::atoi(argv[2]));
    std::mt19937_64 g(20240611);
    uint64_t heads = 0;
    for (uint32_t P = 1; P <= 20; P++) {
        const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P);
        cur_P = P; cur_head = 0;
        CHECK(p1 + p0 == P && p1 + p0 <= 32u && p0 <= 16u && p1 <= 16u);  // x_lo lies in the low dword of head'
        const uint64_t t1 = 1ull << (31u + p1), t0 = 1ull << (31u + p1 + p0);
        const uint64_t edge[] = {L, L + 1u, t1 - 1u, t1, t1 + 1u, t0 - 1u, t0, t0 + 1u, (1ull << 32) - 1u, 1ull << 32, (1ull << 63) - 1u, 1ull << 63, ~0ull};
        for (uint64_t h : edge)
            for (uint32_t w : {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, (uint32_t)g()})
                if (h >= L) { check_pair(h, w, ~w, P); heads++; }
        for (int i = 0; i < 200000; i++) {  // 4 M heads over the twenty precisions, every magnitude from 2^31 up equally often
            uint64_t h = g() >> (g() % 33ull);
            if (h < L) h |= L;
            check_pair(h, (uint32_t)g(), (uint32_t)g(), P);
            heads++;
        }
    }
    std::printf("pairs agree on %llu heads\n", (unsigned long long)heads);
    // whole synthetic decodes: the list of the headline workload, and 4100 steps at the precisions of the GPU cases
    std::printf("synthetic decode, per-class steps (none / slice-0 refill / slice-1 refill / both), slice-0 refills undone by the index push, "
                "slice-1 refills behind a push that renormalised:\n");
    const struct { uint32_t n, P; } runs[] = {{52114, 20}, {4100, 20}, {4100, 19}, {4100, 18}, {4100, 17}, {4100, 16}, {4100, 13}};
    for (auto r : runs) {
        const Freq f = synthetic(r.n, r.P, 7u + r.P);
        cur_P = r.P; cur_head = 0;
        CHECK(f.cls[U2_POP_BOTH] == 0u);
        if (r.P <= 16u) CHECK(f.cls[U2_POP_SLICE1] == 0u);
        std::printf("  n %6u P %2u: %6llu (%4.1f %%) / %6llu (%4.1f %%) / %6llu (%4.1f %%) / %llu; undone %llu (%4.1f %%); %llu of %llu\n", r.n, r.P,
                    (unsigned long long)f.cls[0], 100.0 * f.cls[0] / f.steps, (unsigned long long)f.cls[1], 100.0 * f.cls[1] / f.steps,
                    (unsigned long long)f.cls[2], 100.0 * f.cls[2] / f.steps, (unsigned long long)f.cls[3], (unsigned long long)f.undone,
                    100.0 * f.undone / f.steps, (unsigned long long)f.slice1_after_renorm, (unsigned long long)f.slice1);
    }
    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("u2 pops ok\n");
    return 0;
}
