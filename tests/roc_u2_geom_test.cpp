// The LDS geometry of the round-2 ROC chain kernels as csrc/roc_u2_geom.h computes it, checked on the host for
// tests/test_roc_u2_geom_cpu.py: the dense encoder (base table, slots + pad, strip) and the bitmap decoder (u32 counter rows,
// bitmap in natural entry order, strip).  Every region is listed as [begin, end); the program checks that the
// regions of a kernel are disjoint, ascending and inside the launch's LDS bytes, that the launch fits a workgroup, and that
// everything a step addresses lies inside its region.  Built with g++ like tests/roc_rows_geom_test.cpp (no HIP, no GPU).
#include <cstdio>
#include <initializer_list>

#include "../vector_db_id_compression_amd/csrc/roc_u2_geom.h"

using namespace vidc::dev;

static int fails = 0;
#define EXPECT(c)                                                          \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static const uint32_t WG_LDS = 163840u;  // LDS a workgroup can have on gfx950

struct Region {
    const char *name;
    uint32_t begin, end;
};
static void disjoint_inside(const Region *r, int nr, uint32_t total) {
    for (int i = 0; i < nr; i++) {
        EXPECT(r[i].begin < r[i].end);
        EXPECT(r[i].end <= total);
        if (i) EXPECT(r[i - 1].end <= r[i].begin);
        std::printf("  %-10s [%6u, %6u)\n", r[i].name, r[i].begin, r[i].end);
    }
}

template <int UB>
static void decoder() {
    using U = U2Geom<UB>;
    std::printf("decoder UB %d: %u bytes\n", UB, U::DEC_LDS_BYTES);
    const Region r[3] = {{"rows", 0u, U::DEC_ROWS_BYTES},
                         {"bitmap", U::DEC_BITMAP_OFF, U::DEC_BITMAP_OFF + U::BITMAP_BYTES},
                         {"strip", U::DEC_STRIP_OFF, U::DEC_STRIP_OFF + 64u * 4u}};
    disjoint_inside(r, 3, U::DEC_LDS_BYTES);
    EXPECT(U::DEC_LDS_BYTES <= WG_LDS);
    EXPECT(U::DEC_LDS_BYTES % 16u == 0u);  // cleared in 16-byte pieces
    // natural order: id x sits in entry x >> ESH, bitmap word x >> 6, dword x >> 5; the row element of the entry is dword `entry`
    const uint32_t top = (1u << UB) - 1u;
    for (uint32_t x : {0u, 63u, 64u, top - 64u, top}) {
        const uint32_t e = x >> U::ESH;
        EXPECT(e < U::NE);
        EXPECT(4u * e + 4u <= U::DEC_ROWS_BYTES);
        const uint32_t dword = U::DEC_BITMAP_OFF + 4u * (x >> 5);
        EXPECT(dword >= r[1].begin && dword + 4u <= r[1].end);
        const uint32_t rd = U::DEC_BITMAP_OFF + e * U::G * 8u + (U::G - 1u) * 8u;  // the entry's last word, as the step's read forms it
        EXPECT(rd + 8u <= r[1].end);
        EXPECT((x >> 6) >= e * U::G && (x >> 6) < (e + 1u) * U::G);  // the insertion hits a word of the entry the rank reads
    }
    for (uint32_t L1 = 0; L1 < 64u; L1++)
        for (uint32_t lane = 0; lane < 64u; lane++) EXPECT((L1 << 8) + 4u * lane + 4u <= U::DEC_ROWS_BYTES);  // ds_add of the row update
}

int main() {
    using D = U2Dense;
    std::printf("dense encoder: %u bytes\n", D::LDS_BYTES);
    const Region r[4] = {{"base", D::BASE_OFF, D::BASE_OFF + 4096u * 4u},
                         {"slots", D::SLOT_OFF, D::SLOT_OFF + 4096u * 32u},
                         {"pad", D::SLOT_OFF + 4096u * 32u, D::STRIP_OFF},
                         {"strip", D::STRIP_OFF, D::STRIP_OFF + 64u * 4u}};
    disjoint_inside(r, 4, D::LDS_BYTES);
    EXPECT(D::LDS_BYTES <= WG_LDS);
    EXPECT(u2_enc_lds_bytes<20>(true) == D::LDS_BYTES);
    EXPECT(u2_enc_lds_bytes<20>(false) == U2Geom<20>::LDS_BYTES && u2_enc_lds_bytes<18>(true) == U2Geom<18>::LDS_BYTES);
    EXPECT(U2Geom<20>::LDS_BYTES <= WG_LDS && U2Geom<18>::LDS_BYTES <= WG_LDS);
    EXPECT(D::MAX_N == 65536u);
    // u32 level-2 rows behind the strip would not fit a workgroup (why the dense body keeps them in registers); u16 rows would
    EXPECT(D::LDS_BYTES + 64u * 64u * 4u > WG_LDS && D::LDS_BYTES + 64u * 64u * 2u <= WG_LDS);
    // the step's accesses: base[e] through the offset field, 64 u16 from the block's first slot on, the removal's store
    for (uint32_t e : {0u, 1u, 4094u, 4095u}) {
        EXPECT(4u * e + D::BASE_OFF + 4u <= r[0].end);
        for (uint32_t lane = 0; lane < 64u; lane++) {
            const uint32_t v28 = (e << 5) + 2u * lane + (D::SLOT_OFF - 2u);  // slot address minus 2
            EXPECT(v28 + 2u >= r[1].begin && v28 + 2u + 2u <= r[2].end);    // the read (offset:2)
            if (lane >= 1u && lane <= 15u) EXPECT(v28 >= r[1].begin && v28 + 2u <= r[1].end);  // the shift's store
            EXPECT(D::STRIP_OFF + 4u * lane + 2u <= r[3].end);              // every other lane's store
        }
    }
    decoder<20>();
    decoder<18>();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("roc u2 geometry ok\n");
    return 0;
}
