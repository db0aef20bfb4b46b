// The plan of vidc_ivf_scan_wide_dev and vidc_ivf_scan_aq_wide_dev (csrc/ivf_wide_plan.h): every refusal, K2, the buffer and the LDS
// at the edges of k, the cut and the residency for a handful of shapes, the 160 KiB bound.  Stand-alone: g++ -std=c++17
// [-fsanitize=address,undefined] -I vector_db_id_compression_amd/csrc; exit status 0 and "ok".
#include <stdio.h>

#include "ivf_wide_plan.h"

using namespace vidc;

#define CHECK(c) \
    if (!(c)) return fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c), 1

int main() {
    int x = 0;
    const void *p = &x;
    // refusals: k's own range, then the narrow calls'
    const ivs::Args a = {8, p, 100, p, ivs::PQ8, 8, 4, p, 4, p, 16, p, 1000, p, p};
    ivs::Args b = a;
    CHECK(ivw::check_args(a) == nullptr && ivs::check_args(a) != nullptr);
#define REFUSED(field, value) (b = a, b.field = value, ivw::check_args(b) != nullptr)
    CHECK(REFUSED(k, 0) && REFUSED(k, 2049) && REFUSED(k, 0xffffffffu) && !REFUSED(k, 1) && !REFUSED(k, 256) && !REFUSED(k, 257) && !REFUSED(k, 2048));
    CHECK(REFUSED(nprobe, 0) && REFUSED(nprobe, 1025) && REFUSED(d, 0) && REFUSED(d, 2049) && REFUSED(ntotal, 1ull << 32));
    CHECK(REFUSED(nlist, 1ull << 31) && REFUSED(kind, 2) && REFUSED(M, 0) && REFUSED(M, 65) && REFUSED(M, 3) && REFUSED(codebooks, nullptr));
    CHECK(REFUSED(offsets, nullptr) && REFUSED(codes, nullptr) && REFUSED(xq, nullptr) && REFUSED(probes, nullptr) && REFUSED(D, nullptr) && REFUSED(labels, nullptr));
    b = a, b.nq = 0, b.offsets = b.xq = b.codes = b.probes = b.D = b.labels = nullptr;
    CHECK(ivw::check_args(b) == nullptr);
    const iaq::Args q = {8, p, 100, p, 7, 5, p, nullptr, 4, p, 16, p, 1000, p, p};
    iaq::Args r = q;
    CHECK(ivw::check_aq(q) == nullptr && iaq::check_scan(q) != nullptr);
#define AQ_REFUSED(field, value) (r = q, r.field = value, ivw::check_aq(r) != nullptr)
    CHECK(AQ_REFUSED(k, 0) && AQ_REFUSED(k, 2049) && !AQ_REFUSED(k, 2048) && !AQ_REFUSED(k, 20) && AQ_REFUSED(M, 0) && AQ_REFUSED(M, 65));
    CHECK(AQ_REFUSED(nprobe, 1025) && AQ_REFUSED(d, 2049) && AQ_REFUSED(codebooks, nullptr) && AQ_REFUSED(nq, 1ull << 32) && AQ_REFUSED(D, nullptr) && !AQ_REFUSED(centroids, p));
    // K2, the buffer, pool + buffer: 12 KiB at k = 257, 32 KiB at k = 2048
    const uint32_t ks[6] = {1, 256, 257, 512, 513, 2048}, k2s[6] = {512, 512, 512, 512, 1024, 2048}, bufs[6] = {1024, 1024, 1024, 1024, 1024, 2048};
    for (int i = 0; i < 6; i++) {
        CHECK(ivw::k2(ks[i]) == k2s[i] && ivw::buffer_keys(ks[i]) == bufs[i] && ivw::select_bytes(ks[i]) == (size_t)8 * (k2s[i] + bufs[i]));
        CHECK(ivw::merge_lds_bytes(ks[i]) == (size_t)16 * k2s[i] && ivw::buffer_keys(ks[i]) / ivw::WAVES >= 4 * ivs::TRIP);
        CHECK(ivw::lds_bytes(ivw::FLAT, ks[i], 16, 32, 0) == ivw::select_bytes(ks[i]) + 64 + 64 + 128 + 1024);
    }
    CHECK(ivw::select_bytes(257) == 12288 && ivw::select_bytes(2048) == 32768 && ivw::lds_bytes(ivw::PQ8, 1000, 16, 128, 16) == 16384 + 64 + 64 + 512 + 16384);
    CHECK(ivw::lds_bytes(ivw::FLAT, 1000, 16, 32, 0) == 17664 && ivw::lds_bytes(ivw::AQ, 1000, 64, 128, 8) == 28608);
    // at the limits pool + buffer + an M = 64 table (and four staged spans) stay inside a compute unit's 160 KiB
    CHECK(ivw::lds_bytes(ivw::PQ8, 2048, 1024, 2048, 64) == 110656 && ivw::lds_bytes(ivw::AQ, 2048, 1024, 2048, 64) == 128192);
    CHECK(ivw::lds_bytes(ivw::AQ, 2048, 1024, 2048, 64) <= ivs::LDS_PER_CU && ivw::wg_per_cu(128192) == 1 && ivw::wg_per_cu(110656) == 1);
    // residency = compute units x min(8, 160 KiB / LDS); S by the narrow rule over it
    CHECK(ivw::wg_per_cu(17664) == 8 && ivw::wg_per_cu(28608) == 5 && ivw::wg_per_cu(36800) == 4 && ivw::resident(0, 28608) == 5);
    const ivw::Plan f10 = ivw::make_plan(256, ivw::FLAT, 32, 0, 10, 16, 1000, 0, 0), f1e4 = ivw::make_plan(256, ivw::FLAT, 32, 0, 10000, 16, 1000, 0, 0);
    CHECK(f10.resident == 2048 && f10.S == 16 && f10.items == 160 && f10.nwg == 160 && f10.scratch == (uint64_t)10 * 16 * 1001 * 8);
    CHECK(f1e4.S == 1 && f1e4.nwg == 2048 && f1e4.scratch == 0 && f1e4.K2 == 1024 && f1e4.buffer == 1024 && f1e4.grp.V == 4);
    const ivw::Plan a1e3 = ivw::make_plan(256, ivw::AQ, 128, 8, 1000, 64, 500, 0, 0), one = ivw::make_plan(1, ivw::AQ, 16, 8, 3, 4, 257, 0, 0);
    CHECK(a1e3.lds == 12288 + 64 + 256 + 512 + 3200 + 8192 && a1e3.resident == 256 * 6 && a1e3.S == 2 && a1e3.nwg == 1536);
    CHECK(one.lds == 23824 && one.resident == 6 && one.S == 2 && one.items == 6 && one.nwg == 6 && ivw::make_plan(1, ivw::AQ, 16, 8, 20, 4, 257, 0, 0).S == 1);
    CHECK(ivw::make_plan(256, ivw::PQ8, 128, 16, 5, 3, 300, 4, 0).S == 2 && ivw::make_plan(256, ivw::PQ8, 128, 16, 5, 3, 300, 4, 0).W == 4);
    printf("ok\n");
    return 0;
}
