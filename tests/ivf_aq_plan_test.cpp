// The plans of vidc_ivf_aq_lut_dev and vidc_ivf_scan_aq_dev (csrc/ivf_aq_plan.h): the layout and the distance of a row, every
// refusal, the chunk rule, the LDS size at the limits.  Stand-alone: g++ -std=c++17 [-fsanitize=address,undefined]
// -I vector_db_id_compression_amd/csrc; exit status 0 and "ok".
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "ivf_aq_plan.h"

using namespace vidc;

#define CHECK(c) \
    if (!(c)) return fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c), 1

int main() {
    int x = 0;
    const void *p = &x;
    // the layout: the known row, the sizes, the distance (negative, -0 and NaN become +0)
    const uint8_t row[6] = {0x01, 0x02, 0x00, 0x00, 0x80, 0x3f};
    CHECK(iaq::code_size(2) == 6 && iaq::code_size(8) == 12 && iaq::code_size(64) == 68 && iaq::norm_of(row, 2) == 1.0f);
    float table[512] = {};
    table[1] = 3.f, table[256 + 2] = 4.f;
    CHECK(iaq::distance(row, 2, table, 100.f, 50.f, false) == 50.f + 1.f - 14.f && iaq::distance(row, 2, table, 2.f, 50.f, true) == 33.f);
    CHECK(iaq::distance(row, 2, table, 100.f, 50.f, true) == 0.f && !signbit(iaq::distance(row, 2, table, 100.f, 50.f, true)));
    CHECK(!signbit(iaq::clamp_dist(-0.f)) && iaq::clamp_dist(NAN) == 0.f && iaq::clamp_dist(INFINITY) == INFINITY);
    // the scan's refusals: k, nprobe, d, ntotal, nlist, NULL arrays; M; the codebooks; no d % M condition
    const iaq::Args a = {8, p, 100, p, 7, 5, p, nullptr, 4, p, 16, p, 20, p, p};
    CHECK(iaq::check_scan(a) == nullptr);
    iaq::Args b = a;
#define REFUSED(field, value) (b = a, b.field = value, iaq::check_scan(b) != nullptr)
    CHECK(REFUSED(k, 0) && REFUSED(k, 257) && REFUSED(nprobe, 0) && REFUSED(nprobe, 1025) && REFUSED(d, 0) && REFUSED(d, 2049));
    CHECK(REFUSED(ntotal, 1ull << 32) && REFUSED(nlist, 1ull << 31) && REFUSED(M, 0) && REFUSED(M, 65) && REFUSED(nq, 1ull << 32));
    CHECK(REFUSED(offsets, nullptr) && REFUSED(codes, nullptr) && REFUSED(codebooks, nullptr) && REFUSED(xq, nullptr));
    CHECK(REFUSED(probes, nullptr) && REFUSED(D, nullptr) && REFUSED(labels, nullptr));
    CHECK(!REFUSED(M, 64) && !REFUSED(M, 1) && !REFUSED(k, 256) && !REFUSED(centroids, p));
    b = a, b.nq = 0, b.xq = b.codes = nullptr;
    CHECK(iaq::check_scan(b) == nullptr);
    // the table call's
    const iaq::LutArgs l = {7, 5, p, 4, p, p};
    iaq::LutArgs m = l;
#define LUT_REFUSED(field, value) (m = l, m.field = value, iaq::check_lut(m) != nullptr)
    CHECK(iaq::check_lut(l) == nullptr && LUT_REFUSED(d, 0) && LUT_REFUSED(d, 2049) && LUT_REFUSED(M, 0) && LUT_REFUSED(M, 65));
    CHECK(LUT_REFUSED(codebooks, nullptr) && LUT_REFUSED(xq, nullptr) && LUT_REFUSED(lut, nullptr) && LUT_REFUSED(nq, 1ull << 32));
    // the chunk rule: 64 MiB of tables, a multiple of 16, at least 16
    CHECK(iaq::chunk_queries(1) == 65536 && iaq::chunk_queries(8) == 8192 && iaq::chunk_queries(64) == 1024 && iaq::chunk_queries(3) == 21840);
    const uint32_t Ms[3] = {1, 8, 64};
    for (uint32_t M : Ms) {
        const uint64_t c = iaq::chunk_queries(M);
        CHECK(iaq::chunks(c - 1, M) == 1 && iaq::chunks(c, M) == 1 && iaq::chunks(c + 1, M) == 2 && iaq::chunks(0, M) == 0);
        CHECK(iaq::lut_bytes(c, M) <= iaq::LUT_SCRATCH && c % 16 == 0);
    }
    // LDS: RQ8 at d = 128, and the M = 64 limit
    CHECK(iaq::lds_bytes(20, 16, 128, 8) == 1088 + 64 + 512 + 800 + 8192);
    CHECK(iaq::lds_bytes(256, 1024, 2048, 64) == 4864 + 4096 + 8192 + 4384 + 65536 && iaq::lds_bytes(256, 1024, 2048, 64) <= ivs::LDS_PER_CU);
    const iaq::Plan pl = iaq::scan_plan(256, 128, 8, 10000, 16, 20), cut = iaq::scan_plan(256, 128, 8, 10, 16, 20);
    CHECK(pl.lds == 10656 && pl.resident == 256 * 15 && pl.S == 1 && pl.nslots == 3840 && pl.scratch == 0);
    CHECK(cut.S == 16 && cut.items == 160 && cut.nslots == 160 && cut.scratch == ivs::scratch_bytes(10, 16, 20));
    // the table GEMM: tiles of 64 queries x 128 entries, 27648 bytes of LDS
    CHECK(iaq::lut_tiles(1, 1) == 2 && iaq::lut_tiles(65, 8) == 2 * 16 && iaq::lut_lds_bytes() == 27648 && iaq::lut_grid(1, 100) == 4);
    printf("ok\n");
    return 0;
}
