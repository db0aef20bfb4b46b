// The word-granular decode geometry of the 20-bit ROC chain decoder (csrc/roc_u2_geom.h, U2DecWord) checked on the host for
// tests/test_roc_u2_decword_geom_cpu.py.  U2DecWord's functions are the address and data formation of the step of
// k_roc_decode_u2<20, true>; the program walks EVERY id below 2^20 and all 64 lanes through them: rows and bitmap disjoint and inside
// the 163 840 bytes of a workgroup, every read, the insertion (lane 0's bit and the other lanes' OR of 0) and the packed row update
// inside their regions, lane 0's insertion target no other lane's.  Then a model of the LDS runs one full level-1 block (16 384
// consecutive ids) through the packed add in ascending, descending and shuffled order and compares every step's row element and
// the final rows with per-word prefix counts computed the plain way; no carry may cross a field.  Last, 70 000 insertions below one
// word (what only a multiset stream can do) wrap a field: the model shows that nothing outside that row's 512 bytes changes.
// Built with g++ like tests/roc_u2_geom_test.cpp (no HIP, no GPU).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/roc_u2_geom.h"

using namespace vidc::dev;
using D = U2DecWord;

static int fails = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static const uint32_t WG_LDS = 163840u;  // LDS a workgroup can have on gfx950
static const uint32_t ROWS_BEGIN = 0u, ROWS_END = D::ROWS_BYTES, BM_BEGIN = D::BITMAP_OFF, BM_END = D::BITMAP_OFF + D::BITMAP_BYTES;

static void addresses() {
    for (uint32_t x = 0; x < (1u << D::UB); x++) {
        const uint32_t w = x >> 6, L1 = w >> 8;
        const uint32_t ra = D::row_addr(x), wa = D::word_addr(x);
        EXPECT(ra >= ROWS_BEGIN && ra + 2u <= ROWS_END && ra % 2u == 0u);
        EXPECT(ra == 2u * (L1 * 256u + (w & 255u)));                       // u16 row[64][256], element w
        EXPECT(wa >= BM_BEGIN && wa + 8u <= BM_END && wa % 8u == 0u);
        EXPECT(wa - 8u * w <= 65535u);                                     // the bitmap's start is the read's 16-bit offset field
        const uint32_t i0 = D::ins_addr(x, 0u);
        EXPECT(i0 >= BM_BEGIN && i0 + 4u <= BM_END && i0 % 4u == 0u);
        EXPECT(i0 == wa + 4u * ((x >> 5) & 1u));                           // the dword of the word the rank reads
        EXPECT(D::ins_data(x, 0u) == 1u << (x & 31u));
        if ((x & 63u) != 0u) continue;  // the other lanes' targets and the row update depend on x >> 6 only
        for (uint32_t lane = 0; lane < 64u; lane++) {
            if (lane) {
                const uint32_t ij = D::ins_addr(x, lane);
                EXPECT(ij >= ROWS_BEGIN && ij + 4u <= ROWS_END && ij % 4u == 0u);
                EXPECT(ij != i0 && ij == 4u * lane);                       // its own dword: no two lanes on one address
                EXPECT(D::ins_data(x, lane) == 0u);                        // an OR of 0
            }
            const uint32_t aa = D::add_addr(x, lane);
            EXPECT(aa >= ROWS_BEGIN && aa + 8u <= ROWS_END && aa % 8u == 0u);
            EXPECT(aa == 2u * (L1 * 256u + 4u * lane));                    // the fields of words 4 lane .. 4 lane + 3 of row L1
            EXPECT(D::add_shift(x, lane) <= 63u);                          // a 64-bit shift takes six bits of its count
            const uint64_t d = D::add_data(x, lane);
            for (uint32_t f = 0; f < 4u; f++)
                EXPECT(((d >> (16u * f)) & 0xffffu) == (4u * lane + f > (w & 255u) ? 1u : 0u));
        }
    }
}

// the LDS as the step sees it: ds_read_u16, ds_or_b32 and ds_add_u64 on one byte array (little endian, like the GPU)
struct Lds {
    std::vector<unsigned char> b = std::vector<unsigned char>(D::LDS_BYTES, 0);
    uint32_t read_u16(uint32_t a) const { uint16_t v; std::memcpy(&v, &b[a], 2); return v; }
    void or_b32(uint32_t a, uint32_t d) { uint32_t v; std::memcpy(&v, &b[a], 4); v |= d; std::memcpy(&b[a], &v, 4); }
    void add_u64(uint32_t a, uint64_t d) { uint64_t v; std::memcpy(&v, &b[a], 8); v += d; std::memcpy(&b[a], &v, 8); }
};

static void full_block(uint32_t L1, const std::vector<uint32_t> &order, const char *name) {
    Lds lds;
    std::vector<uint32_t> cnt(256u, 0u);  // ids per word of the block, the plain way
    for (uint32_t x : order) {
        const uint32_t wl = (x >> 6) & 255u;
        EXPECT((x >> 14) == L1);
        const uint32_t below = std::accumulate(cnt.begin(), cnt.begin() + wl, 0u);
        EXPECT(lds.read_u16(D::row_addr(x)) == below);                     // what the rank adds
        for (uint32_t lane = 0; lane < 64u; lane++) lds.or_b32(D::ins_addr(x, lane), D::ins_data(x, lane));
        for (uint32_t lane = 0; lane < 64u; lane++) lds.add_u64(D::add_addr(x, lane), D::add_data(x, lane));
        cnt[wl]++;
    }
    uint32_t below = 0, top = 0;
    for (uint32_t wl = 0; wl < 256u; wl++) {
        const uint32_t v = lds.read_u16(2u * (L1 * 256u + wl));
        EXPECT(v == below);                                                // no carry came in from the field below, none went out
        top = v > top ? v : top;
        below += cnt[wl];
    }
    EXPECT(top == 16320u);                                                 // 255 full words below the last one: fits u16
    for (uint32_t a = ROWS_BEGIN; a < ROWS_END; a += 2u)                    // every other row untouched (the ORs of 0 included)
        if (a / 512u != L1) EXPECT(lds.read_u16(a) == 0u);
    for (uint32_t a = BM_BEGIN; a < BM_END; a++) EXPECT(lds.b[a] == ((a - BM_BEGIN) / 2048u == L1 ? 0xffu : 0u));
    std::printf("  block %2u %-10s ok so far: %s\n", L1, name, fails ? "no" : "yes");
}

// a multiset stream may push a field past 65 535: the carry goes into the next field of the SAME u64 or out of its top, so nothing
// outside the row changes (and no address of a step depends on a counter)
static void wrap(uint32_t L1) {
    Lds lds;
    const uint32_t x = (L1 << 14) + 64u * 2u + 5u;  // word 2: lane 0 adds to one field, lanes 1 .. 63 to all four
    for (uint32_t i = 0; i < 70000u; i++) {
        for (uint32_t lane = 0; lane < 64u; lane++) lds.or_b32(D::ins_addr(x, lane), D::ins_data(x, lane));
        for (uint32_t lane = 0; lane < 64u; lane++) lds.add_u64(D::add_addr(x, lane), D::add_data(x, lane));
    }
    EXPECT(lds.read_u16(2u * (L1 * 256u + 3u)) == 70000u - 65536u);  // wrapped
    for (uint32_t a = ROWS_BEGIN; a < ROWS_END; a += 2u)
        if (a / 512u != L1) EXPECT(lds.read_u16(a) == 0u);
    for (uint32_t a = BM_BEGIN; a < BM_END; a++) EXPECT(lds.b[a] == (a == D::word_addr(x) ? 1u << 5 : 0u));
    std::printf("  wrap in row %2u ok so far: %s\n", L1, fails ? "no" : "yes");
}

int main() {
    std::printf("word-row decoder: %u bytes\n", D::LDS_BYTES);
    std::printf("  rows   [%6u, %6u)\n  bitmap [%6u, %6u)\n", ROWS_BEGIN, ROWS_END, BM_BEGIN, BM_END);
    EXPECT(ROWS_END <= BM_BEGIN && BM_END <= D::LDS_BYTES);
    EXPECT(D::LDS_BYTES == WG_LDS);
    EXPECT(D::LDS_BYTES % 16u == 0u);  // cleared in 16-byte pieces
    EXPECT(D::ROWS_BYTES == 64u * 256u * 2u && D::BITMAP_BYTES * 8u == 1u << D::UB);
    EXPECT(U2Geom<20>::DEC_LDS_BYTES == 147712u);  // the four-word geometry stays what it was
    addresses();
    for (uint32_t L1 : {0u, 37u, 63u}) {
        std::vector<uint32_t> ids(16384u);
        std::iota(ids.begin(), ids.end(), L1 << 14);
        full_block(L1, ids, "ascending");
        std::reverse(ids.begin(), ids.end());
        full_block(L1, ids, "descending");
        std::mt19937 g(20u + L1);
        std::shuffle(ids.begin(), ids.end(), g);
        full_block(L1, ids, "shuffled");
    }
    wrap(0u);
    wrap(63u);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("roc u2 word-row geometry ok\n");
    return 0;
}
