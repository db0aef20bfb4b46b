// shardplan::update_blocks (csrc/shard_plan.h) -- the byte offsets of the home scratch block of a routed call (translate_labels, append,
// remove) and of a far shard's own block -- walked over shard counts, request counts, every combination of optional sections and mask
// lengths around 16.  Stand-alone host program: g++ -std=c++17 (also with -fsanitize=address,undefined).  usage: shard_blocks_test
//
// Asserted for both blocks: 8-byte sections are 8-aligned, every mask starts at a multiple of 16, no two sections overlap, every section
// lies inside the block in front of 16 bytes of slack, and every section has the size of what is written into it: ns * n * 8 (local
// numbers, 8-byte answers), ns * n (found bytes), n (owner bytes), a mask's length rounded up to 16; n * 8, n and the rounded mask in
// a far block.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/shard_plan.h"

using namespace vidc::shardplan;

struct Section {
    std::string name;
    size_t off, bytes, align;
};

static long g_layouts = 0;

static void fail(const std::string &what, const std::string &a, const std::string &b = "") {
    std::fprintf(stderr, "layout %ld: %s: %s %s\n", g_layouts, what.c_str(), a.c_str(), b.c_str());
    std::exit(1);
}

// `total` includes the 16 bytes of slack
static void check(const char *block, const std::vector<Section> &secs, size_t total) {
    if (total < 16) fail(block, "no slack");
    for (size_t i = 0; i < secs.size(); i++) {
        const Section &a = secs[i];
        if (a.off % a.align) fail(std::string(block) + ": alignment", a.name);
        if (a.off + a.bytes > total - 16) fail(std::string(block) + ": outside the block", a.name);
        for (size_t j = 0; j < i; j++) {
            const Section &b = secs[j];
            if (a.bytes && b.bytes && a.off < b.off + b.bytes && b.off < a.off + a.bytes) fail(std::string(block) + ": overlap", a.name, b.name);
        }
    }
}

int main() {
    const uint32_t NS[] = {1, 2, 3, 8};
    const uint64_t N[] = {0, 1, 63, 64, 65, 1000};
    const uint64_t LOADS[] = {0, 1, 15, 16, 17, 1025};
    auto up16 = [](uint64_t b) { return (size_t)((b + 15) / 16 * 16); };
    for (uint32_t ns : NS)
        for (uint64_t n : N)
            for (int opt = 0; opt < 16; opt++)
                for (int m = -1; m < 6; m++) {  // -1: a call without masks; else shard i's mask holds LOADS[(m + i) % 6] bytes
                    const bool has_local = opt & 1, has_answers = opt & 2, has_found = opt & 4, has_owner = opt & 8;
                    std::vector<uint64_t> len(ns, 0);
                    for (uint32_t i = 0; m >= 0 && i < ns; i++) len[i] = LOADS[((uint32_t)m + i) % 6];
                    g_layouts++;
                    const UpdateBlocks B = update_blocks(ns, n, has_local, has_answers, m >= 0 ? len.data() : nullptr, has_found, has_owner);
                    if (B.mask.size() != ns || B.f_total.size() != ns) fail("per-shard arrays", "size");
                    if (B.found_bytes != (has_found ? (size_t)ns * n : 0)) fail("found_bytes", "value");
                    std::vector<Section> home = {{"invalid", 0, (size_t)ns * 8, 8},
                                                 {"local", B.local, has_local ? (size_t)ns * n * 8 : 0, 8},
                                                 {"answers", B.answers, has_answers ? (size_t)ns * n * 8 : 0, 8},
                                                 {"found", B.found, has_found ? (size_t)ns * n : 0, 1},
                                                 {"owner", B.owner, has_owner ? (size_t)n : 0, 1}};
                    for (uint32_t i = 0; i < ns; i++) home.push_back({"mask " + std::to_string(i), B.mask[i], up16(len[i]), 16});
                    check("home block", home, B.total);
                    for (uint32_t i = 0; i < ns; i++) {
                        const std::vector<Section> far = {{"invalid", 0, 8, 8},
                                                          {"local", B.f_local, has_local ? (size_t)n * 8 : 0, 8},
                                                          {"ids", B.f_ids, (size_t)n * 8, 8},
                                                          {"answers", B.f_answers, has_answers ? (size_t)n * 8 : 0, 8},
                                                          {"found", B.f_found, has_found ? (size_t)n : 0, 1},
                                                          {"mask", B.f_mask, up16(len[i]), 16}};
                        check("far block", far, B.f_total[i]);
                    }
                }
    std::printf("shard blocks ok: %ld layouts\n", g_layouts);
    return 0;
}
