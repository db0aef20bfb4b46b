// The ring traffic of the k_roc_decode_u2 step (csrc/roc_u2.h, U2_DEC_STEP bit 2), restated in csrc/u2_dec_ring_ref.h: the classified
// form against the reference form (u2_pops_one + the index push of codec.cpp:44-63) -- class, H, id, sp, carried word and the ring
// below sp -- for every precision 1 .. 20 and every nmax 1 .. 65 536 with heads on both sides of every threshold, for random heads,
// and in whole synthetic decodes (random stream words, uniform ranks) with a 64-slot ring that is refilled and spilled in 32-word
// halves as the C++ glue does.  Built and run by tests/test_u2_dec_ring_cpu.py (g++, no HIP, no GPU).
// usage: u2_dec_ring_test            the checks
//        u2_dec_ring_test eval N     N lines "head w w2 nmax P" on stdin (sp = 40, ring[39] = w, ring[38] = w2, every other slot 0)
//                                    -> "cls H x sp w wrote slot word" of both forms (the Python port is checked with it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/u2_dec_ring_ref.h"

using namespace vidc;

static int fails = 0;
static uint64_t cur_head;
static uint32_t cur_P, cur_nmax;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s (line %d, P %u, nmax %u, head %llx)\n", #c, __LINE__, cur_P, cur_nmax, (unsigned long long)cur_head); fails++; } } while (0)

static const uint64_t L = 1ull << 31;  // rans_l
static uint64_t seen[4] = {0, 0, 0, 0};

static bool same_below_sp(const uint32_t *a, const uint32_t *b, uint32_t lo, uint32_t sp) {
    for (uint32_t i = lo; i != sp; i++)
        if (a[i & 63u] != b[i & 63u]) return false;
    return true;
}

// one step of both forms on copies of one ring holding `res` words below sp
static void check_pair(uint64_t head, uint32_t sp, const uint32_t *ring, uint32_t res, uint32_t nmax, uint32_t P) {
    cur_head = head; cur_P = P; cur_nmax = nmax;
    const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P), lq = u2_ring_lq(nmax);
    uint32_t ra[64], rb[64];
    std::memcpy(ra, ring, sizeof ra); std::memcpy(rb, ring, sizeof rb);
    const U2DecRing a = u2_dec_ring_ref(head, sp, ra, lq, p1, p0);
    const U2DecRing b = u2_dec_ring_cls(head, sp, rb, ring[(sp - 1u) & 63u], lq, p1, p0);
    CHECK(a.cls == b.cls);
    CHECK(a.H == b.H);
    CHECK(a.x == b.x);
    CHECK(a.sp == b.sp);
    CHECK(a.w == b.w);
    CHECK(b.w == rb[(b.sp - 1u) & 63u]);                       // the carried word is the word below the top
    CHECK(same_below_sp(ra, rb, sp - res, a.sp));
    CHECK(same_below_sp(ring, rb, sp - res, sp < b.sp ? sp : b.sp));  // nothing below the old top changes
    CHECK((b.cls == U2_RING_QUIET) == (b.wrote == 0u));
    if (b.cls == U2_RING_QUIET) CHECK(b.sp == sp && std::memcmp(rb, ring, sizeof rb) == 0);
    if (b.wrote) CHECK(a.wrote && a.slot == b.slot && a.word == b.word);
    if (head >= (1ull << (31u + p1))) {                        // the class from h and lq alone
        const uint64_t h = head >> (p1 + p0);
        CHECK(b.cls == u2_ring_class(h, lq));
        CHECK((b.cls == U2_RING_QUIET) == (h >= lq && (h >> 32) < lq));
    } else {
        CHECK(b.cls == U2_RING_SIDE);
    }
    seen[b.cls & 3u]++;
}

// one synthetic decode of n steps; the ring holds words [lo, sp) and is kept at 22 .. 56 words between steps
struct Freq { uint64_t cls[4] = {0, 0, 0, 0}, steps = 0, exits = 0; };
static Freq synthetic(uint32_t n, uint32_t P, uint64_t seed) {
    std::mt19937_64 g(seed);
    uint32_t ra[64], rb[64];
    for (int i = 0; i < 64; i++) ra[i] = rb[i] = (uint32_t)g();
    uint32_t lo = 1u << 24, spa = lo + 40u, spb = spa;
    uint64_t ha = L, hb = L;
    uint32_t w = rb[(spb - 1u) & 63u];                          // U2_DEC_ENTRY_U
    const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P);
    Freq f;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t nmax = i + 1u, lq = u2_ring_lq(nmax);
        cur_head = ha; cur_P = P; cur_nmax = nmax;
        const U2DecRing a = u2_dec_ring_ref(ha, spa, ra, lq, p1, p0);
        const U2DecRing b = u2_dec_ring_cls(hb, spb, rb, w, lq, p1, p0);
        CHECK(a.cls == b.cls && a.H == b.H && a.x == b.x && a.sp == b.sp && a.w == b.w);
        CHECK(b.w == rb[(b.sp - 1u) & 63u]);
        CHECK(same_below_sp(ra, rb, lo, a.sp));
        f.cls[b.cls & 3u]++; f.steps++;
        spa = a.sp; spb = b.sp; w = b.w;
        const uint64_t rank = g() % nmax;
        ha = a.H * nmax + rank; hb = b.H * nmax + rank;
        if (ha < L) {                                           // second half of the index push: the loop exits, the glue pops, the entry reloads
            ha = (uint64_t)ra[--spa & 63u] | (ha << 32);
            hb = (uint64_t)rb[--spb & 63u] | (hb << 32);
            w = rb[(spb - 1u) & 63u];
            f.exits++;
        }
        CHECK(ha == hb && ha >= L);
        if (spb - lo > 56u) lo += 32u;                          // ws_spill32
        else if (spb - lo < 22u) {                              // ws_refill32: the slots of [lo - 32, lo) are free
            for (uint32_t j = lo - 32u; j != lo; j++) ra[j & 63u] = rb[j & 63u] = (uint32_t)g();
            lo -= 32u;
            w = rb[(spb - 1u) & 63u];                           // (the glue comes back through the entry)
        }
    }
    return f;
}

static int eval_mode(int n) {
    for (int i = 0; i < n; i++) {
        unsigned long long head; unsigned w, w2, nmax, P;
        if (std::scanf("%llu %u %u %u %u", &head, &w, &w2, &nmax, &P) != 5) return 1;
        const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P), lq = u2_ring_lq(nmax);
        uint32_t ra[64] = {0}, rb[64] = {0};
        ra[39] = rb[39] = w; ra[38] = rb[38] = w2;
        const U2DecRing a = u2_dec_ring_ref(head, 40u, ra, lq, p1, p0), b = u2_dec_ring_cls(head, 40u, rb, w, lq, p1, p0);
        std::printf("%u %llu %u %u %u %u %u %u %u %llu %u %u %u %u %u %u\n", a.cls, (unsigned long long)a.H, a.x, a.sp, a.w, a.wrote, a.slot, a.word,
                    b.cls, (unsigned long long)b.H, b.x, b.sp, b.w, b.wrote, b.slot, b.word);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 2 && !std::strcmp(argv[1], "eval")) return eval_mode(std::atoi(argv[2]));
    std::mt19937_64 g(20261126);
    uint32_t ring[64];
    for (auto &w : ring) w = (uint32_t)g();
    uint64_t heads = 0;
    // every precision, every nmax: heads on both sides of every threshold
    for (uint32_t P = 1; P <= 20; P++) {
        const uint32_t p1 = u2_pop_p1(P), p0 = u2_pop_p0(P), sh = p1 + p0;
        for (uint32_t nmax = 1; nmax <= 65536u; nmax++) {
            const uint64_t lq = u2_ring_lq(nmax);
            cur_P = P; cur_nmax = nmax; cur_head = 0;
            CHECK(lq >= (1u << 15) && lq <= (1u << 31));
            uint64_t thr[5] = {L, 1ull << (31u + p1), 1ull << (31u + sh), lq << sh, 0};
            int nt = 4;
            if (lq < (1ull << (32u - sh))) thr[nt++] = (lq << 32) << sh;  // (the spill-only class exists below 2^64 for this lq)
            const uint32_t sp = 40u + (nmax & 63u);
            ring[(sp - 1u) & 63u] = (uint32_t)(nmax * 2654435761u);     // the carried word varies with the case
            for (int t = 0; t < nt; t++)
                for (int d = -1; d <= 1; d++) {
                    const uint64_t h = thr[t] + (uint64_t)(int64_t)d;
                    if (h >= L) { check_pair(h, sp, ring, 30u, nmax, P); heads++; }
                }
            check_pair((1ull << 63) - 1u, sp, ring, 30u, nmax, P);
            check_pair(~0ull, sp, ring, 30u, nmax, P);
            heads += 2;
        }
    }
    const uint64_t spill_edges = seen[U2_RING_SPILL];
    cur_P = 0; cur_nmax = 0; cur_head = 0;
    CHECK(spill_edges > 0u);                                            // heads with h_hi >= lq, the class a set never reaches
    // random heads: 4 M over the precisions, every magnitude from 2^31 up equally often, nmax of every magnitude
    for (int i = 0; i < 4000000; i++) {
        const uint32_t P = 1u + (uint32_t)(g() % 20ull);
        uint32_t nmax = (uint32_t)(g() & 0xffffull) >> (g() % 17ull);
        nmax = (i & 7) == 0 ? 65536u - nmax : nmax + 1u;
        uint64_t h = g() >> (g() % 33ull);
        if (h < L) h |= L;
        const uint32_t sp = (uint32_t)g();
        ring[(sp - 1u) & 63u] = (uint32_t)g(); ring[(sp - 2u) & 63u] = (uint32_t)g();
        check_pair(h, sp, ring, 30u, nmax, P);
        heads++;
    }
    std::printf("forms agree on %llu heads: quiet %llu, refill only %llu, spill only %llu (%llu at the thresholds), side %llu\n", (unsigned long long)heads,
                (unsigned long long)seen[0], (unsigned long long)seen[1], (unsigned long long)seen[2], (unsigned long long)spill_edges, (unsigned long long)seen[3]);
    CHECK(seen[0] && seen[1] && seen[2] > spill_edges && seen[3]);
    // whole synthetic decodes: the list of the headline workload, 4100 steps at the precisions of the GPU cases, and lists longer than their
    // universe (nmax > 2^P: the streams of multisets), which reach the spill-only class
    std::printf("synthetic decode, steps per class (quiet / refill only / spill only / side), exits on head < 2^31:\n");
    const struct { uint32_t n, P; } runs[] = {{52114, 20}, {4100, 20}, {4100, 19}, {4100, 18}, {4100, 17}, {4100, 16}, {4100, 13}, {4161, 10}, {4161, 8}, {65536, 4}};
    for (auto r : runs) {
        const Freq f = synthetic(r.n, r.P, 11u + r.P);
        cur_P = r.P; cur_head = 0; cur_nmax = 0;
        CHECK(f.steps == r.n);
        if (r.P <= 16u) CHECK(f.cls[U2_RING_SIDE] == 0u);
        if (r.n <= (1u << r.P)) CHECK(f.cls[U2_RING_SPILL] == 0u);     // nmax <= 2^P: h_hi < 2^(31 - P) <= lq
        if (r.P <= 8u) CHECK(f.cls[U2_RING_SPILL] > 0u);
        std::printf("  n %6u P %2u: %6llu (%5.2f %%) / %6llu (%5.2f %%) / %6llu (%5.2f %%) / %6llu (%5.2f %%); %llu\n", r.n, r.P,
                    (unsigned long long)f.cls[0], 100.0 * f.cls[0] / f.steps, (unsigned long long)f.cls[1], 100.0 * f.cls[1] / f.steps,
                    (unsigned long long)f.cls[2], 100.0 * f.cls[2] / f.steps, (unsigned long long)f.cls[3], 100.0 * f.cls[3] / f.steps,
                    (unsigned long long)f.exits);
    }
    if (fails) { std::printf("%d checks FAILED\n", fails); return 1; }
    std::printf("u2 dec ring ok\n");
    return 0;
}
