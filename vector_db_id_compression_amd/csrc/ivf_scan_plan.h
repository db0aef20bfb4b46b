// ivf_scan_plan.h -- what the host decides for vidc_ivf_scan_dev before any device work: the argument checks, the resident wavefront
// slots, the cut S of a probe row, the scratch of the cut, the lane grouping of the FLAT distance loop, the load width of a PQ code
// and the LDS of one wavefront.  Host only, no HIP runtime: ivf_scan.hip includes it and tests/ivf_scan_test.cpp builds it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "graph_search_plan.h"
#include "ivf_scan_ref.h"

namespace vidc {
namespace ivs {

constexpr uint32_t WAVES_PER_CU = 32;         // the hardware's cap on resident wavefronts of a compute unit
constexpr size_t LDS_PER_CU = 160u * 1024u;   // gfx950
constexpr uint32_t MAX_SLOTS = 8192;          // resident wavefronts of one call (256 compute units x 32)

// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work)
struct Args {
    uint64_t nlist;
    const void *offsets;
    uint64_t ntotal;
    const void *codes;
    int kind;
    uint32_t d, M;
    const void *codebooks;
    uint64_t nq;
    const void *xq;
    uint32_t nprobe;
    const void *probes;
    uint32_t k;
    const void *D, *labels;
};
inline const char *check_args(const Args &a) {
    if (a.nq && (!a.offsets || !a.xq || !a.probes || !a.D || !a.labels || (a.ntotal && !a.codes)))
        return "NULL offsets, code, query, probe, distance or label array";
    if (a.k < 1 || a.k > MAX_K) return "1 <= k <= 256";
    if (a.nprobe < 1 || a.nprobe > MAX_NPROBE) return "1 <= nprobe <= 1024";
    if (a.d < 1 || a.d > MAX_D) return "1 <= d <= 2048";
    if (a.ntotal >= (1ull << 32)) return "ntotal must be below 2^32 (a key packs a position in 32 bits)";
    if (a.nlist >= (1ull << 31)) return "nlist must be below 2^31";
    if (a.kind != FLAT && a.kind != PQ8) return "code_kind is VIDC_IVF_FLAT or VIDC_IVF_PQ8";
    if (a.kind == PQ8) {
        if (a.M < 1 || a.M > MAX_M) return "PQ8: 1 <= M <= 64";
        if (a.d % a.M) return "PQ8: d must be a multiple of M";
        if (!a.codebooks) return "PQ8: NULL codebooks";
    }
    return nullptr;
}

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// dynamic LDS of a scan wavefront.  FLAT: two pools of k keys (the insert writes the other one), the survivors' keys, the trip's
// distances, the probe row, the query vector.  PQ8: the query vector is needed only while the table is built and the pools only
// afterwards, so they share their bytes; behind them the probe row and the M x 256 table.
inline size_t lds_bytes(int kind, uint32_t k, uint32_t nprobe, uint32_t d, uint32_t M) {
    const size_t pools = (size_t)2 * k * 8 + (size_t)TRIP * 8 + (size_t)TRIP * 4, row = round16((size_t)nprobe * 4), q = round16((size_t)d * 4);
    if (kind == PQ8) return (pools > q ? pools : q) + row + (size_t)M * 256 * 4;
    return pools + row + q;
}
// (PQ8 at the limits: 8192 + 4096 + 65536 = 77824 bytes, two wavefronts per compute unit; M = 16, d = 128, k = 20, nprobe = 16:
// 1088 + 64 + 16384 = 17536 bytes, nine; FLAT d = 32, k = 20, nprobe = 16: 1280 bytes)
inline size_t merge_lds_bytes(uint32_t S, uint32_t k) { return (size_t)S * k * 8; }

// wavefronts of this LDS size that a compute unit holds, and the resident slots of the call
inline uint32_t slots_per_cu(size_t lds) {
    const size_t by_lds = lds ? LDS_PER_CU / lds : WAVES_PER_CU;
    return (uint32_t)(by_lds < 1 ? 1 : (by_lds > WAVES_PER_CU ? WAVES_PER_CU : by_lds));
}
inline uint32_t resident_slots(uint32_t num_cu, size_t lds) {
    const uint64_t s = (uint64_t)(num_cu ? num_cu : 1) * slots_per_cu(lds);
    return (uint32_t)(s > MAX_SLOTS ? MAX_SLOTS : s);
}
// the cut: the smallest S of 1, 2, 4, 8, 16 with nq * S >= the resident slots, and S <= nprobe
inline uint32_t pieces(uint64_t nq, uint32_t nprobe, uint32_t resident) {
    uint32_t S = 1;
    while (S < MAX_S && S * 2 <= nprobe && nq * S < resident) S *= 2;
    return S;
}
// one wavefront (= one workgroup) per slot; a slot takes items slot, slot + slots, ...; item = query * S + piece
inline uint32_t slots(uint64_t items, uint32_t resident) {
    const uint64_t s = items < resident ? items : resident;
    return (uint32_t)(s ? s : 1);
}
inline uint64_t slot_items(uint64_t items, uint32_t nslots, uint32_t s) { return s < items ? (items - 1 - s) / nslots + 1 : 0; }

// context scratch of a cut call: the pieces' keys [nq, S, k], behind them their counters [nq, S] = {lists, codes} (uint32 pairs)
inline uint64_t scratch_keys(uint64_t nq, uint32_t S, uint32_t k) { return S > 1 ? nq * S * k : 0; }
inline uint64_t scratch_bytes(uint64_t nq, uint32_t S, uint32_t k) { return S > 1 ? (nq * S * k + nq * S) * 8 : 0; }

// PQ8: the bytes one load of a code takes -- the widest power of two (<= 16) that divides both M and the address of the codes
inline uint32_t code_load_bytes(uint32_t M, uintptr_t base) {
    uint32_t w = 16;
    while (w > 1 && (M % w || base % w)) w >>= 1;
    return w;
}

struct Plan {
    size_t lds, merge_lds;
    uint32_t resident, S, nslots, W;
    uint64_t items, scratch;
    gs::Group grp;  // FLAT: G lanes per vector, V components per load (the rule of graph_search_plan.h)
};
inline Plan make_plan(uint32_t num_cu, int kind, uint32_t d, uint32_t M, uint64_t nq, uint32_t nprobe, uint32_t k, uintptr_t codes, uintptr_t xq) {
    Plan p;
    p.lds = lds_bytes(kind, k, nprobe, d, M);
    p.resident = resident_slots(num_cu, p.lds);
    p.S = pieces(nq, nprobe, p.resident);
    p.items = nq * p.S;
    p.nslots = slots(p.items, p.resident);
    p.scratch = scratch_bytes(nq, p.S, k);
    p.merge_lds = merge_lds_bytes(p.S, k);
    p.W = kind == PQ8 ? code_load_bytes(M, codes) : 0;
    p.grp = gs::group(d, ((codes | xq) & 15u) == 0);
    return p;
}

}  // namespace ivs
}  // namespace vidc
