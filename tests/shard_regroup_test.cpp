// shardplan::regroup_plan and shardplan::moved_ids (csrc/shard_plan.h) -- the host plan of vidc_rebalance_sharded -- against values the
// calling test computed with numpy (tests/rebalance_ref.py).  Stand-alone host program: g++ -std=c++17 (also with
// -fsanitize=address,undefined).  usage: shard_regroup_test CASES_FILE
//
// The file is whitespace-separated numbers behind a keyword per case:
//   REGROUP nshards nlist sizes[nlist] old_owner[nlist] new_owner[nlist] moved_ids  then per NEW shard: nl src_no[nl] list_no[nl] load
// The old plan is make_plan_for_owner(old_owner), the new one make_plan of the same offsets: its owner must be new_owner.
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

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    in.open(argv[1]);
    if (!in) return 2;
    std::string kw;
    while (in >> kw) {
        g_case++;
        if (kw != "REGROUP") {
            std::fprintf(stderr, "unknown keyword %s\n", kw.c_str());
            return 2;
        }
        const int ns = (int)num();
        const uint64_t nlist = num();
        std::vector<uint64_t> off(nlist + 1, 0);
        for (uint64_t l = 0; l < nlist; l++) off[l + 1] = off[l] + num();
        const std::vector<uint64_t> old64 = nums(nlist), new64 = nums(nlist);
        const uint64_t moved = num();
        const ShardPlan old_p = make_plan_for_owner(off.data(), nlist, ns, std::vector<int32_t>(old64.begin(), old64.end()));
        const ShardPlan new_p = make_plan(off.data(), nlist, ns);
        for (uint64_t l = 0; l < nlist; l++)
            if ((uint64_t)new_p.owner[l] != new64[l]) fail("new owner", l);
        if (moved_ids(old_p, new_p) != moved) fail("moved_ids", moved_ids(old_p, new_p));
        if (moved_ids(old_p, old_p) != 0 || moved_ids(new_p, new_p) != 0) fail("moved_ids of a map against itself", 0);
        const std::vector<RegroupRows> rows = regroup_plan(old_p, new_p);
        if (rows.size() != (size_t)ns) fail("shard count", rows.size());
        uint64_t seen = 0;
        for (size_t d = 0; d < (size_t)ns; d++) {
            const uint64_t nl = num();
            const std::vector<uint64_t> src = nums(nl), lst = nums(nl);
            if (rows[d].src_no.size() != nl || rows[d].list_no.size() != nl || new_p.lists[d].size() != nl) fail("rows of a shard", d);
            for (uint64_t j = 0; j < nl; j++) {
                if (rows[d].src_no[j] != src[j]) fail("src_no", j);
                if (rows[d].list_no[j] != lst[j]) fail("list_no", j);
                // the row names the same global list under the old map, and a list of the same size
                if (src[j] >= (uint64_t)ns || lst[j] >= old_p.lists[src[j]].size()) fail("row out of range", j);
                const uint64_t g = old_p.lists[src[j]][lst[j]];
                if (g != new_p.lists[d][j]) fail("global list of a row", j);
                if (old_p.local_offsets[src[j]][lst[j] + 1] - old_p.local_offsets[src[j]][lst[j]] != new_p.size_of(g)) fail("size of a row", j);
            }
            if (new_p.load[d] != num()) fail("load", d);
            seen += nl;
        }
        if (seen != nlist) fail("every list in one row", seen);
        // a map that does not change: every row names its own shard and its own number
        const std::vector<RegroupRows> same = regroup_plan(new_p, new_p);
        for (size_t d = 0; d < (size_t)ns; d++)
            for (size_t j = 0; j < same[d].src_no.size(); j++)
                if (same[d].src_no[j] != d || same[d].list_no[j] != j) fail("identity rows", d);
    }
    std::printf("shard regroup ok: %ld cases\n", g_case);
    return 0;
}
