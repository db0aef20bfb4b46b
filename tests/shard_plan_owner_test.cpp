// shardplan::make_plan_for_owner (csrc/shard_plan.h) -- the plan of a GIVEN ownership, what an append to a sharded object re-plans with --
// against values the calling test computed with numpy.  Stand-alone host program: g++ -std=c++17 (also with
// -fsanitize=address,undefined).  usage: shard_plan_owner_test CASES_FILE
//
// The file is whitespace-separated numbers behind a keyword per case:
//   OWNER nshards nlist sizes[nlist] owner[nlist] is_lpt  local_no[nlist]  then per shard: nl lists[nl] local_offsets[nl + 1] nseg segs[3 nseg] load
// is_lpt = 1: the owner is the LPT one, and make_plan must give the same plan, field for field.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/shard_plan.h"

using namespace vidc::shardplan;

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
static void same(const char *what, const std::vector<uint64_t> &got, const std::vector<uint64_t> &want) {
    if (got.size() != want.size()) fail(what, (uint64_t)-1);
    for (size_t i = 0; i < got.size(); i++)
        if (got[i] != want[i]) fail(what, i);
}
static std::vector<uint64_t> flat(const std::vector<Segment> &s) {
    std::vector<uint64_t> v;
    for (const Segment &x : s) {
        v.push_back(x.src_start);
        v.push_back(x.dst_start);
        v.push_back(x.count);
    }
    return v;
}
static void same_plan(const ShardPlan &a, const ShardPlan &b) {
    if (a.nshards != b.nshards || a.nlist != b.nlist || a.ntotal != b.ntotal) fail("make_plan: sizes", 0);
    same("make_plan: offsets", a.offsets, b.offsets);
    same("make_plan: load", a.load, b.load);
    for (uint64_t l = 0; l < a.nlist; l++)
        if (a.owner[l] != b.owner[l] || a.local_no[l] != b.local_no[l]) fail("make_plan: map", l);
    for (size_t s = 0; s < (size_t)a.nshards; s++) {
        same("make_plan: lists", a.lists[s], b.lists[s]);
        same("make_plan: local offsets", a.local_offsets[s], b.local_offsets[s]);
        same("make_plan: cut", flat(a.cut[s]), flat(b.cut[s]));
    }
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    in.open(argv[1]);
    if (!in) return 2;
    std::string kw;
    while (in >> kw) {
        g_case++;
        if (kw != "OWNER") {
            std::fprintf(stderr, "unknown keyword %s\n", kw.c_str());
            return 2;
        }
        const int ns = (int)num();
        const uint64_t nlist = num();
        std::vector<uint64_t> off(nlist + 1, 0);
        for (uint64_t l = 0; l < nlist; l++) off[l + 1] = off[l] + num();
        const std::vector<uint64_t> owner64 = nums(nlist);
        const bool is_lpt = num() != 0;
        const std::vector<int32_t> owner(owner64.begin(), owner64.end());
        const ShardPlan p = make_plan_for_owner(off.data(), nlist, ns, owner);
        if (p.nshards != ns || p.nlist != nlist || p.ntotal != off[nlist]) fail("sizes", 0);
        same("offsets", p.offsets, off);
        const std::vector<uint64_t> local = nums(nlist);
        for (uint64_t l = 0; l < nlist; l++) {
            if ((uint64_t)p.owner[l] != owner64[l]) fail("owner", l);
            if (p.local_no[l] != local[l]) fail("local_no", l);
            if (p.packed(l) != (owner64[l] << 32 | local[l])) fail("packed map", l);
        }
        uint64_t total = 0;
        for (size_t s = 0; s < (size_t)ns; s++) {
            const uint64_t nl = num();
            same("lists of a shard", p.lists[s], nums(nl));
            same("local offsets", p.local_offsets[s], nums(nl + 1));
            const uint64_t nseg = num();
            same("cut segments", flat(p.cut[s]), nums(3 * nseg));
            if (p.load[s] != num()) fail("load", s);
            if (p.load[s] != p.local_offsets[s].back()) fail("load against the local offsets", s);
            total += p.load[s];
        }
        if (total != p.ntotal) fail("sum of loads", total);
        if (is_lpt) same_plan(make_plan(off.data(), nlist, ns), p);
    }
    std::printf("shard plan for owner ok: %ld cases\n", g_case);
    return 0;
}
