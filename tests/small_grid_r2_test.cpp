// small_grid_r2_test.cpp -- which lists csrc/roc_enc_plan.h sends to the position-bitmap chains (promote_r2) for a given compute-unit
// count, with the planner's own code: `prog num_cu max_id n0 n1 ...` prints the number of lists in the chain class.  The lists are
// classified as roc.hip does it for ascending lists without the row-per-list kernels: by length alone while no list reaches the bitmap
// kernels' minimum, else per list with the prepass maxima.  Host code only (g++); tests/test_small_grid_shapes_cpu.py runs it on the
// shapes of tests/test_gpu_small_grid.py.
#include <cstdio>
#include <cstdlib>

#include "../vector_db_id_compression_amd/csrc/roc_enc_plan.h"

using namespace vidc;

// the limits roc.hip fills in from the kernel headers (tests/roc_enc_plan_test.cpp holds the same row)
static const EncLimits LIM{64, 1024, 4096, 8192, 4097, 256, 262144, 8192, 8192, 2048};

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    EncPolicy p;
    p.num_cu = std::atoi(argv[1]);
    p.want_perm = true;
    p.gpol = GrpPolicy{~0ull, 4097, 32768, 16384, 4097};  // (never enough lists: the row-per-list kernels stay out)
    const uint32_t max_id = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const uint64_t nlist = (uint64_t)argc - 3;
    std::vector<uint64_t> off(nlist + 1, 0);
    for (uint64_t l = 0; l < nlist; l++) off[l + 1] = off[l] + std::strtoull(argv[3 + l], nullptr, 10);
    const EncCounts x = count_classes(off.data(), 0, nlist, p.gpol, LIM);
    const EncUse use = enc_families(x.c0, x.c1, x.c2, x.cg, p, LIM);
    EncWorkLists w;
    if (x.max_n < LIM.u_min_list) {
        std::vector<uint32_t> order;
        classify_by_length(off.data(), nlist, x.max_n, false, use, p, LIM, w, order);
    } else {
        std::vector<uint32_t> maxid(nlist, max_id), pflags(nlist, 0u), prec(nlist, 0u);
        auto par = [](uint64_t n, unsigned, auto &&f) { f((uint64_t)0, n, 0u); };
        if (classify_per_list(off.data(), nlist, maxid.data(), pflags.data(), VIDC_PREC_REFERENCE, use, p, LIM, x.c0, use.lane ? x.c1 : 0, 1u, par,
                              prec.data(), w) >= 0)
            return 3;
        for (int k = W_U18; k < W_COUNT; k++)
            std::stable_sort(w.wl[k].begin(), w.wl[k].end(), [&](uint32_t a, uint32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
    }
    promote_r2(w, off.data(), p, LIM);
    std::printf("%zu %zu %zu %zu\n", w.wl[W_R2].size(), w.wl[W_C1].size(), w.wl[W_C2].size(), w.wl[W_C3].size());
    return 0;
}
