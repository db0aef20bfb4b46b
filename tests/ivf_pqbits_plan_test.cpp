// The plans of vidc_ivf_scan_pqbits_dev and vidc_ivf_pq_encode_bits_dev (csrc/ivf_pqbits_plan.h, csrc/ivf_pqbits_encode_plan.h): the
// layout, LDS and resident slots at PQ8x10, the LDS refusal, the nbits bounds.  Stand-alone: g++ -std=c++17
// [-fsanitize=address,undefined] -I vector_db_id_compression_amd/csrc; exit status 0 and "ok".
#include <stdio.h>
#include <string.h>

#include "ivf_pqbits_encode_plan.h"
#include "ivf_pqbits_plan.h"

using namespace vidc;

#define CHECK(c) \
    if (!(c)) return fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c), 1

int main() {
    int x = 0;
    const void *p = &x;
    // the layout: the known row, and the sizes
    const uint8_t row[4] = {0x01, 0x08, 0x30, 0x00};
    CHECK(ipb::field_of(row, 0, 10) == 1 && ipb::field_of(row, 1, 10) == 2 && ipb::field_of(row, 2, 10) == 3);
    CHECK(ipb::code_size(8, 10) == 10 && ipb::code_size(3, 10) == 4 && ipb::code_size(7, 1) == 1 && ipb::code_size(16, 8) == 16);
    // PQ8x10, d = 128, k = 20, nprobe = 16
    CHECK(ipb::lds_bytes(20, 16, 128, 8, 10, true) == 1088 + 64 + 1024 + 672 + 32768);
    CHECK(ipb::lds_bytes(20, 16, 128, 8, 10, false) == 1088 + 64 + 512 + 672 + 32768);
    const ipb::Plan pl = ipb::scan_plan(256, 128, 8, 10, true, 10000, 16, 20, 16);
    CHECK(pl.lds == 35616 && pl.resident == 256 * 4 && pl.S == 1 && pl.nslots == 1024 && pl.vec4 && pl.scratch == 0);
    const ipb::Plan cut = ipb::scan_plan(256, 128, 8, 10, true, 10, 16, 20, 4);
    CHECK(cut.S == 16 && cut.items == 160 && cut.nslots == 160 && !cut.vec4 && cut.scratch == ivs::scratch_bytes(10, 16, 20));
    // the refusals: the bits, d % M, the LDS limit (and its text names the limit)
    ipb::Args a = {8, p, 100, p, 128, 8, 10, p, p, 4, p, 16, p, 20, p, p};
    CHECK(ipb::check_scan(a) == nullptr);
    for (uint32_t nbits = 0; nbits <= 14; nbits++) {
        ipb::Args b = a;
        b.nbits = nbits;
        b.M = 2;
        CHECK((ipb::check_scan(b) == nullptr) == (nbits >= 1 && nbits <= 12));
        const ipbe::Args e = {5, p, 128, 2, nbits, p, 0, nullptr, nullptr, p};
        CHECK((ipbe::check_args(e) == nullptr) == (nbits >= 1 && nbits <= 12));
    }
    ipb::Args b = a;
    b.M = 7;
    CHECK(ipb::check_scan(b) != nullptr);
    b = a;
    b.M = 32;  // 32 x 1024 entries: 131072 bytes of table, passes
    CHECK(ipb::check_scan(b) == nullptr && ipb::lds_bytes(20, 16, 128, 32, 10, true) <= ipb::LDS_LIMIT);
    b.M = 64;  // 262144 bytes
    CHECK(ipb::check_scan(b) != nullptr && strstr(ipb::check_scan(b), "163840") && strstr(ipb::check_scan(b), "160 KB"));
    // the encoder: PQ8x10 streams, PQ16x4 is held; scratch = norms + uint16 indices
    const ipbe::Plan e10 = ipbe::make_plan(256, 1000000, 128, 8, 10, 16, 16, 0), e4 = ipbe::make_plan(256, 300, 64, 16, 4, 16, 16, 0);
    CHECK(!e10.whole && e10.lds == ikm::STREAM_LDS && e10.cs == 10 && e10.ksub == 1024 && e10.vec);
    CHECK(e10.scratch == 8u * 1024 * 4 + 1000000ull * 8 * 2);
    CHECK(e4.whole && e4.lds == 16u * 8 * 4 && e4.cs == 8 && e4.S >= 1 && e4.S <= e4.ntiles);
    printf("ok\n");
    return 0;
}
