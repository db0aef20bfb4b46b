// ivf_pqbits_encode_plan.h -- what the host decides for vidc_ivf_pq_encode_bits_dev before any device work: the argument checks,
// whether the codebook of a sub-quantiser is held whole in LDS or streamed, the LDS of a workgroup, the resident workgroups, the cut S
// of the vector range, the load width and the context scratch.  Host only, no HIP runtime: ivf_pqbits_encode.hip includes it and
// tests/ivf_pqbits_plan_test.cpp builds it with g++.
//
// The first stage is k_kmeans_assign's form (ivf_kmeans_plan.h: the tile and staging constants, held_whole, the cut, the load width)
// with ksub = 2^nbits in the place of k; the second packs the winning indices into the layout of ivf_pqbits_plan.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ivf_kmeans_plan.h"
#include "ivf_pq_encode_plan.h"
#include "ivf_pqbits_plan.h"

namespace vidc {
namespace ipbe {

struct Args {
    uint64_t n;
    const void *x;
    uint32_t d, M, nbits;
    const void *pq;
    uint64_t nlist;
    const void *centroids, *assign, *codes;
};
// -> NULL, or the text of the refusal (VIDC_ERR_INVALID, before any device work): the 8-bit encoder's refusals, and the bits
inline const char *check_args(const Args &a) {
    const ipe::Args e = {a.n, a.x, a.d, a.M, a.pq, a.nlist, a.centroids, a.assign, a.codes};
    if (const char *msg = ipe::check_args(e)) return msg;
    if (a.nbits < 1 || a.nbits > ipb::MAX_NBITS) return "1 <= nbits <= 12";
    return nullptr;
}

// context scratch: the norms |c|^2 [M, ksub] float32, behind them (16-byte aligned) the winning indices [n, M] uint16
inline uint64_t norm_bytes(uint32_t M, uint32_t nbits) { return ivs::round16((size_t)M * ipb::ksub_of(nbits) * 4); }
inline uint64_t scratch_bytes(uint64_t n, uint32_t M, uint32_t nbits) { return norm_bytes(M, nbits) + n * M * 2; }

struct Plan {
    uint32_t dsub, ksub, cs, S, resident, grid;
    bool whole, vec;
    size_t lds;
    uint64_t ntiles, items, scratch;
};
inline Plan make_plan(uint32_t num_cu, uint64_t n, uint32_t d, uint32_t M, uint32_t nbits, uintptr_t x, uintptr_t pq, uintptr_t centroids) {
    Plan p;
    p.dsub = d / M;
    p.ksub = ipb::ksub_of(nbits);
    p.cs = (uint32_t)ipb::code_size(M, nbits);
    p.whole = ikm::held_whole(p.dsub, p.ksub);
    p.lds = ikm::lds_bytes(p.dsub, p.ksub);
    p.resident = ikm::resident_workgroups(num_cu, p.lds);
    p.ntiles = ikm::tiles(n);
    p.S = ikm::pieces(M, p.ntiles, p.resident);
    p.items = (uint64_t)M * p.S;
    p.grid = (uint32_t)(p.items < p.resident ? p.items : p.resident);
    p.vec = ipe::vector_loads(d, p.dsub, x, pq, centroids);
    p.scratch = scratch_bytes(n, M, nbits);
    return p;
}
// (PQ8x10, d = 128: dsub = 16, 1024 x 20 floats = 81920 bytes: streamed, 36864 bytes of staging, two workgroups a compute unit;
// PQ16x4, d = 64: 16 x 8 floats = 512 bytes held; nbits = 12, dsub = 4: 4096 x 8 floats = 131072: streamed)

}  // namespace ipbe
}  // namespace vidc
