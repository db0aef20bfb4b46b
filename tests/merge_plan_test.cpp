// merge_plan_test.cpp -- the deciding half of the merge calls (csrc/merge_plan.h) as a stand-alone host program: reads cases from a
// file, one per line, answers each and compares with the expectation the line carries (the numpy model's, tests/merge_ref.py).
//   CLASS a_n b_n shifted want
//   REFUSE any_null nlist_a nlist_b dev_ctx dev_a dev_b ntotal_a ntotal_b want
//   SHIFT max_b add_id bits want
// Built with g++, plain and under -fsanitize=address,undefined (tests/test_merge_abi_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../vector_db_id_compression_amd/csrc/merge_plan.h"

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: merge_plan_test cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string line;
    size_t ncases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string kind;
        ss >> kind;
        std::vector<unsigned long long> v;
        unsigned long long x;
        while (ss >> x) v.push_back(x);
        unsigned long long got = 0, want = 0;
        if (kind == "CLASS" && v.size() == 4) {
            got = vidc::merge_roc_class(v[0], v[1], v[2] != 0);
            want = v[3];
        } else if (kind == "REFUSE" && v.size() == 9) {
            got = (unsigned long long)vidc::merge_refusal(v[0] != 0, v[1], v[2], (int)v[3], (int)v[4], (int)v[5], v[6], v[7]);
            want = v[8];
        } else if (kind == "SHIFT" && v.size() == 4) {
            got = vidc::merge_shift_overflows(v[0], v[1], (uint32_t)v[2]) ? 1 : 0;
            want = v[3];
        } else {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        if (got != want) {
            std::fprintf(stderr, "case %zu (%s): got %llu, want %llu\n", ncases, line.c_str(), got, want);
            return 1;
        }
        ncases++;
    }
    std::printf("merge plan ok: %zu cases\n", ncases);
    return 0;
}
