// rocseg::make_plan, expand_request / collapse_request, fix_chunks_all and check_map (csrc/roc_seg_plan.h) -- the host plan of the
// segmented ROC container -- against values the calling test computed with numpy (tests/roc_seg_ref.py).  Stand-alone host program:
// g++ -std=c++17 (also with -fsanitize=address,undefined).  usage: roc_seg_plan_test CASES_FILE
//
// The file is whitespace-separated numbers behind a keyword per case:
//   PLAN T B nlist sizes[nlist] status   and for status 0: k[nlist] shift[nlist] seg_first[nlist + 1] tbl_base[nlist + 1] meta_segs
//        nchunks (list start)[nchunks]
//   REQ  T B nlist sizes[nlist] inner_sizes[n_inner] m list_nos[m]   then: m' inner_nos[m'] out_offsets[m + 1] nfix (start count base)[nfix]
//        nfix_all (start count base)[nfix_all]          (the request decoded back to back; then the fix-up of decode_all)
//   MAP  nlist seg_first[nlist + 1] shift[nlist] B inner_nlist prec[inner_nlist] expected
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/roc_seg_plan.h"

using namespace vidc::rocseg;

static std::ifstream in;
static long g_case = 0;

static uint64_t num() {
    uint64_t v;
    if (!(in >> v)) {
        std::fprintf(stderr, "case %ld: the cases file ends early\n", g_case);
        std::exit(2);
    }
    return v;
}
static std::vector<uint64_t> nums(uint64_t n) {
    std::vector<uint64_t> v(n);
    for (auto &x : v) x = num();
    return v;
}
static void fail(const char *what, uint64_t at) {
    std::fprintf(stderr, "case %ld: %s differs at %llu\n", g_case, what, (unsigned long long)at);
    std::exit(1);
}
static std::vector<uint64_t> offsets_of(const std::vector<uint64_t> &sizes) {
    std::vector<uint64_t> off(sizes.size() + 1, 0);
    for (size_t l = 0; l < sizes.size(); l++) off[l + 1] = off[l] + sizes[l];
    return off;
}
static void check_fix(const std::vector<FixChunk> &got, const char *what) {
    const uint64_t n = num();
    if (got.size() != n) fail(what, got.size());
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t start = num(), count = num(), base = num();
        if (got[i].start != start || got[i].count != count || got[i].base != base) fail(what, i);
        if (count == 0 || count > SEG_CHUNK) fail("fix chunk length", i);
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    in.open(argv[1]);
    if (!in) return 2;
    if (!valid_seg_ids(16) || !valid_seg_ids(65536) || valid_seg_ids(8) || valid_seg_ids(131072) || valid_seg_ids(48) || valid_seg_ids(0)) fail("valid_seg_ids", 0);
    if (ceil_log2(1) != 0 || ceil_log2(2) != 1 || ceil_log2(3) != 2 || ceil_log2(1024) != 10 || ceil_log2(1025) != 11 || bit_width(0) != 0 || bit_width(1023) != 10) fail("ceil_log2", 0);
    std::string kw;
    while (in >> kw) {
        g_case++;
        if (kw == "PLAN") {
            const uint32_t T = (uint32_t)num(), B = (uint32_t)num();
            const uint64_t nlist = num();
            const std::vector<uint64_t> off = offsets_of(nums(nlist));
            const uint64_t status = num();
            SegPlan p;
            uint64_t bad = ~0ull;
            if ((uint64_t)make_plan(off.data(), nlist, T, B, p, &bad) != status) fail("status", status);
            if (status) {
                if (bad >= nlist) fail("bad list", bad);
                continue;
            }
            const std::vector<uint64_t> k = nums(nlist), shift = nums(nlist), seg_first = nums(nlist + 1), tbl = nums(nlist + 1);
            for (uint64_t l = 0; l < nlist; l++) {
                const ListSeg &s = p.lists[l];
                if (s.k != k[l] || s.shift != shift[l] || p.shift[l] != shift[l]) fail("k / shift", l);
                if (s.seg_first != seg_first[l] || p.seg_first[l] != seg_first[l]) fail("seg_first", l);
                if (s.tbl_base != tbl[l] || s.off != off[l] || s.n != off[l + 1] - off[l]) fail("tbl_base / off / n", l);
                if (s.nchunks != (s.n + SEG_CHUNK - 1) / SEG_CHUNK) fail("nchunks", l);
            }
            if (p.seg_first[nlist] != seg_first[nlist] || p.n_inner != seg_first[nlist] || p.table_len != tbl[nlist]) fail("totals", 0);
            if (p.meta_segs != num()) fail("meta_segs", p.meta_segs);
            const uint64_t nchunks = num();
            if (p.chunks.size() != nchunks) fail("chunk count", p.chunks.size());
            for (uint64_t c = 0; c < nchunks; c++) {
                const uint64_t l = num(), start = num();
                if (p.chunks[c].list != l || p.chunks[c].start != start) fail("chunk", c);
                if (l >= nlist || start >= p.lists[l].n) fail("chunk out of its list", c);
            }
        } else if (kw == "REQ") {
            const uint32_t T = (uint32_t)num(), B = (uint32_t)num();
            const uint64_t nlist = num();
            const std::vector<uint64_t> off = offsets_of(nums(nlist));
            SegPlan p;
            uint64_t bad = 0;
            if (make_plan(off.data(), nlist, T, B, p, &bad) != PLAN_OK) fail("plan", bad);
            const std::vector<uint64_t> inner_off = offsets_of(nums(p.n_inner));
            const uint64_t m = num();
            const std::vector<uint64_t> req = nums(m);
            const std::vector<uint64_t> inner = expand_request(p.seg_first, m, req.data());
            if (inner.size() != num()) fail("expanded length", inner.size());
            std::vector<uint64_t> inner_out(inner.size() + 1, 0);
            for (size_t i = 0; i < inner.size(); i++) {
                if (inner[i] != num()) fail("expanded list", i);
                inner_out[i + 1] = inner_out[i] + (inner_off[inner[i] + 1] - inner_off[inner[i]]);
            }
            std::vector<uint64_t> out_off(m + 1, ~0ull);
            const std::vector<FixChunk> fix = collapse_request(p.seg_first, p.shift, m, req.data(), inner_out, out_off.data());
            for (uint64_t j = 0; j <= m; j++)
                if (out_off[j] != num()) fail("out_offsets", j);
            check_fix(fix, "request fix chunk");
            check_fix(fix_chunks_all(p.seg_first, p.shift, inner_off), "decode_all fix chunk");
        } else if (kw == "MAP") {
            const uint64_t nlist = num();
            const std::vector<uint64_t> seg_first = nums(nlist + 1), shift64 = nums(nlist);
            const uint32_t B = (uint32_t)num();
            const uint64_t inner_nlist = num();
            const std::vector<uint64_t> prec64 = nums(inner_nlist);
            const std::vector<uint8_t> shift(shift64.begin(), shift64.end());
            std::vector<uint32_t> prec(prec64.begin(), prec64.end());
            prec.push_back(0);  // (data() of an empty vector may be NULL)
            const uint64_t want = num();
            const uint64_t got = check_map(nlist, seg_first.data(), shift.data(), B, inner_nlist, prec.data());
            if (got != want) fail("check_map", got);
        } else {
            std::fprintf(stderr, "unknown keyword %s\n", kw.c_str());
            return 2;
        }
    }
    std::printf("roc seg plan ok: %ld cases\n", g_case);
    return 0;
}
