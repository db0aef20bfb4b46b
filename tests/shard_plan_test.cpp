// The host plan of vidc_shards (csrc/shard_plan.h) against values the calling test computed with sharding.lpt_partition and numpy.
// Stand-alone host program: g++ -std=c++17 (also with -fsanitize=address,undefined).  usage: shard_plan_test CASES_FILE
//
// The file is whitespace-separated numbers behind a keyword per case:
//   PLAN   nshards nlist sizes[nlist]  owner[nlist] local_no[nlist]  then per shard: nl local_offsets[nl + 1] nseg segs[3 nseg] nchunks
//   ROUTE  nshards nlist sizes[nlist]  m list_nos[m]  out_offsets[m + 1]  then per shard: k local_lists[k] nseg segs[3 nseg] staged
//   GATHER nshards nlist sizes[nlist]  m list_nos[m] n slot[n] off[n]  rc bad  then (rc == 0) per shard: k local_lists[k] ni slot[ni] off[ni] index[ni]
//   BADLIST nshards nlist sizes[nlist] m list_nos[m] bad
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
static ShardPlan read_plan(int &nshards) {
    nshards = (int)num();
    const uint64_t nlist = num();
    std::vector<uint64_t> off(nlist + 1, 0);
    for (uint64_t l = 0; l < nlist; l++) off[l + 1] = off[l] + num();
    return make_plan(off.data(), nlist, nshards);
}

// the chunk table covers every segment exactly once, in pieces of at most SHARD_COPY_UNIT, in order
static void check_chunks(const std::vector<Segment> &segs, uint64_t want_count) {
    const std::vector<CopyChunk> ch = build_copy_chunks(segs);
    if (ch.size() != want_count) fail("chunk count", ch.size());
    size_t c = 0;
    for (size_t i = 0; i < segs.size(); i++)
        for (uint64_t st = 0; st < segs[i].count; st += SHARD_COPY_UNIT, c++)
            if (c >= ch.size() || ch[c].seg != i || ch[c].start != st) fail("chunk table", c);
    if (c != ch.size()) fail("chunk table length", c);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    in.open(argv[1]);
    if (!in) return 2;
    std::string kw;
    while (in >> kw) {
        g_case++;
        int ns = 0;
        if (kw == "PLAN") {
            const ShardPlan p = read_plan(ns);
            const std::vector<uint64_t> owner = nums(p.nlist), local = nums(p.nlist);
            for (uint64_t l = 0; l < p.nlist; l++) {
                if ((uint64_t)p.owner[l] != owner[l]) fail("owner", l);
                if (p.local_no[l] != local[l]) fail("local_no", l);
                if (p.packed(l) != (owner[l] << 32 | local[l])) fail("packed map", l);
            }
            uint64_t total = 0;
            for (int s = 0; s < ns; s++) {
                const uint64_t nl = num();
                if (p.lists[(size_t)s].size() != nl) fail("lists of a shard", (uint64_t)s);
                same("local offsets", p.local_offsets[(size_t)s], nums(nl + 1));
                const uint64_t nseg = num();
                same("cut segments", flat(p.cut[(size_t)s]), nums(3 * nseg));
                check_chunks(p.cut[(size_t)s], num());
                if (p.load[(size_t)s] != p.local_offsets[(size_t)s].back()) fail("load", (uint64_t)s);
                total += p.load[(size_t)s];
            }
            if (total != p.ntotal) fail("sum of loads", total);
        } else if (kw == "ROUTE") {
            const ShardPlan p = read_plan(ns);
            const uint64_t m = num();
            const std::vector<uint64_t> req = nums(m);
            ListsRoute r;
            uint64_t bad = 0;
            if (!route_lists(p, m, req.data(), r, &bad)) fail("route_lists refused a valid request", bad);
            same("out_offsets", r.out_offsets, nums(m + 1));
            for (int s = 0; s < ns; s++) {
                same("routed local lists", r.local_lists[(size_t)s], nums(num()));
                same("place segments", flat(r.place[(size_t)s]), nums(3 * num()));
                if (r.staged[(size_t)s] != num()) fail("staged", (uint64_t)s);
            }
        } else if (kw == "GATHER") {
            const ShardPlan p = read_plan(ns);
            const uint64_t m = num();
            const std::vector<uint64_t> req = nums(m);
            const uint64_t n = num();
            const std::vector<uint64_t> slot = nums(n), off = nums(n);
            const uint64_t want_rc = num(), want_bad = num();
            GatherRoute r;
            uint64_t bad = 0;
            const int rc = route_gather(p, m, req.data(), n, slot.data(), off.data(), r, &bad);
            if ((uint64_t)rc != want_rc) fail("route_gather status", (uint64_t)rc);
            if (rc != 0) {
                if (bad != want_bad) fail("route_gather bad position", bad);
                continue;
            }
            for (int s = 0; s < ns; s++) {
                same("gather local lists", r.local_lists[(size_t)s], nums(num()));
                const uint64_t ni = num();
                same("gather slots", r.item_slot[(size_t)s], nums(ni));
                same("gather offsets", r.item_off[(size_t)s], nums(ni));
                same("gather index", r.item_index[(size_t)s], nums(ni));
            }
        } else if (kw == "BADLIST") {
            const ShardPlan p = read_plan(ns);
            const uint64_t m = num();
            const std::vector<uint64_t> req = nums(m);
            const uint64_t want_bad = num();
            ListsRoute r;
            uint64_t bad = ~0ull;
            if (route_lists(p, m, req.data(), r, &bad)) fail("route_lists accepted a bad list", 0);
            if (bad != want_bad) fail("bad list position", bad);
        } else {
            std::fprintf(stderr, "unknown keyword %s\n", kw.c_str());
            return 2;
        }
    }
    std::printf("shard plan ok: %ld cases\n", g_case);
    return 0;
}
