// ivf_wide_plan.h -- what the host decides for vidc_ivf_scan_wide_dev and vidc_ivf_scan_aq_wide_dev (1 <= k <= 2048) before any device
// work: the argument checks, the sizes of pool and candidate buffer, the LDS of one workgroup, the resident workgroups, the cut S and
// its scratch.  Host only, no HIP runtime: ivf_wide.hip includes it and tests/ivf_wide_plan_test.cpp builds it with g++.
//
// The rules of the result (key, probe row, clamp, drop test, label) are ivf_scan_ref.h's; the cut rule, the run layout and the
// refusals other than k's are ivf_scan_plan.h's and ivf_aq_plan.h's, called and not restated.
//
// One workgroup of THREADS = 256 (four wavefronts) takes an item (query, piece).  Its LDS, every part a multiple of 16 bytes:
//   pool     K2 keys, sorted, EMPTY padded: K2 = the power of two >= k, at least 512
//   buffer   max(1024, K2) keys, unsorted: a quarter per wavefront
//   control  64 bytes: the wavefronts' buffer counts of the even and the odd rounds
//   row, query vector
//   FLAT: 64 trip floats per wavefront.  PQ8: the M x 256 table.  AQ: a staged span per wavefront, the M x 256 table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_aq_plan.h"
#include "ivf_scan_plan.h"
#include "ivf_scan_ref.h"

namespace vidc {
namespace ivw {

constexpr uint32_t MAX_K = 2048;     // results per query
constexpr uint32_t THREADS = 256;    // a workgroup: four wavefronts
constexpr uint32_t WAVES = THREADS / ivs::TRIP;
constexpr uint32_t ROUND = THREADS;  // codes per round: wavefront w takes the trip at p0 + 64 w
constexpr uint32_t MIN_K2 = 512, MIN_BUFFER = 1024;
constexpr uint32_t MAX_WG_PER_CU = 8;  // 8 x 4 wavefronts: the hardware's cap
constexpr uint32_t CONTROL_BYTES = 64;

enum { FLAT = ivs::FLAT, PQ8 = ivs::PQ8, AQ = 2 };  // the table forms of the kernel

inline uint32_t k2(uint32_t k) {
    uint32_t p = MIN_K2;
    while (p < k) p <<= 1;
    return p;
}
inline uint32_t buffer_keys(uint32_t k) { return k2(k) > MIN_BUFFER ? k2(k) : MIN_BUFFER; }
inline size_t select_bytes(uint32_t k) { return ((size_t)k2(k) + buffer_keys(k)) * 8; }  // 12 KiB at k = 257, 32 KiB at k = 2048

inline size_t lds_bytes(int form, uint32_t k, uint32_t nprobe, uint32_t d, uint32_t M) {
    const size_t head = select_bytes(k) + CONTROL_BYTES + ivx::row_bytes(nprobe) + ivx::vec_bytes(d);
    if (form == PQ8) return head + ivx::table_bytes(M);
    if (form == AQ) return head + WAVES * iaq::stage_bytes(M) + iaq::table_bytes(M);
    return head + (size_t)WAVES * ivs::TRIP * 4;
}
// (FLAT d = 32, k = 1000, nprobe = 16: 16384 + 64 + 64 + 128 + 1024 = 17664 bytes, eight workgroups a compute unit; RQ8 d = 128,
// k = 1000, nprobe = 64: 16384 + 64 + 256 + 512 + 3200 + 8192 = 28608, five; PQ8 M = 64 at the limits: 32768 + 64 + 4096 + 8192 +
// 65536 = 110656, one; AQ M = 64 at the limits: 128192, one: the cap of a launch is raised above 64 KiB)
inline size_t merge_lds_bytes(uint32_t k) { return (size_t)2 * k2(k) * 8; }  // two runs at a time, never S

inline uint32_t wg_per_cu(size_t lds) {
    const size_t by_lds = lds ? ivs::LDS_PER_CU / lds : MAX_WG_PER_CU;
    return (uint32_t)(by_lds < 1 ? 1 : (by_lds > MAX_WG_PER_CU ? MAX_WG_PER_CU : by_lds));
}
inline uint32_t resident(uint32_t num_cu, size_t lds) { return (num_cu ? num_cu : 1) * wg_per_cu(lds); }

// -> NULL, or the text of the refusal: k's own range, then every other refusal of the narrow call
inline const char *check_k(uint32_t k) { return (k < 1 || k > MAX_K) ? "1 <= k <= 2048" : nullptr; }
inline const char *check_args(ivs::Args a) {
    if (const char *msg = check_k(a.k)) return msg;
    if (a.k > ivs::MAX_K) a.k = ivs::MAX_K;
    return ivs::check_args(a);
}
inline const char *check_aq(iaq::Args a) {
    if (const char *msg = check_k(a.k)) return msg;
    if (a.k > ivs::MAX_K) a.k = ivs::MAX_K;
    return iaq::check_scan(a);
}

struct Plan {
    size_t lds, merge_lds;
    uint32_t K2, buffer, resident, S, nwg, W;
    uint64_t items, scratch;
    gs::Group grp;  // FLAT: G lanes per vector, V components per load
};
inline Plan make_plan(uint32_t num_cu, int form, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uint32_t k, uintptr_t codes, uintptr_t xq) {
    Plan p = {};
    p.K2 = k2(k);
    p.buffer = buffer_keys(k);
    p.lds = lds_bytes(form, k, nprobe, d, M);
    p.merge_lds = merge_lds_bytes(k);
    p.resident = resident(num_cu, p.lds);
    p.S = ivs::pieces(nq, nprobe, p.resident);
    p.items = nq * p.S;
    p.nwg = ivs::slots(p.items, p.resident);
    p.scratch = ivs::scratch_bytes(nq, p.S, k);
    p.W = form == PQ8 ? ivs::code_load_bytes(M, codes) : 0;
    p.grp = gs::group(d, ((codes | xq) & 15u) == 0);
    return p;
}

}  // namespace ivw
}  // namespace vidc
