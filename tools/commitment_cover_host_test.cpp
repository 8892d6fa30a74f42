// commitment_cover_host_test.cpp -- prints what csrc/commitment_proofs_plan.h
// computes, for tests/test_commitment_proofs_plan.py to compare with the
// oracle (proofs.subtree_root_coords) and the greedy definition:
//   C W w s0 e0 : level:index ...   subtree_cover_item for every item of the
//                                   range, after checking subtree_cover_count
//                                   against the items (every 0 <= s0 < e0 <= W
//                                   and power of two w <= W, W = 1 .. 32, and
//                                   spot ranges of W = 1024);
//   P k thr n : sizes               commitment_proofs_plan of the blobs on the
//   E k thr : text                  command line (start:len ...), or its error.
// Host only: g++ -std=c++20 -I csrc tools/commitment_cover_host_test.cpp
// csrc/square_plan.cpp; also built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "commitment_proofs_plan.h"

using namespace cda;

static int print_cover(uint32_t W, uint32_t w, uint32_t s0, uint32_t e0) {
    const uint32_t n = subtree_cover_count(s0, e0, w);
    std::printf("C %u %u %u %u :", W, w, s0, e0);
    uint32_t at = s0;
    for (uint32_t i = 0; i < n; i++) {
        const TreeNode t = subtree_cover_item(s0, e0, w, i);
        if ((t.index << t.level) != at) {
            std::fprintf(stderr, "W %u w %u [%u, %u): item %u does not start at %u\n", W, w, s0, e0, i, at);
            return 1;
        }
        at += 1u << t.level;
        std::printf(" %u:%u", t.level, t.index);
    }
    std::printf("\n");
    if (at != e0) {
        std::fprintf(stderr, "W %u w %u [%u, %u): the cover ends at %u\n", W, w, s0, e0, at);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3) {   // k threshold start:len ...
        const uint32_t k = (uint32_t)std::strtoul(argv[1], nullptr, 10), thr = (uint32_t)std::strtoul(argv[2], nullptr, 10);
        std::vector<uint32_t> starts, lens;
        for (int i = 3; i < argc; i++) {
            char* end = nullptr;
            starts.push_back((uint32_t)std::strtoul(argv[i], &end, 10));
            lens.push_back((uint32_t)std::strtoul(end + 1, nullptr, 10));
        }
        CommitmentProofsPlan p;
        const std::string bad = commitment_proofs_plan(k, starts.data(), lens.data(), (uint32_t)starts.size(), thr, &p);
        if (!bad.empty()) std::printf("E %u %u : %s\n", k, thr, bad.c_str());
        else
            std::printf("P %u %u %zu : %u %u %u %u %u\n", k, thr, starts.size(), p.n_segments, p.n_roots, p.n_nodes,
                        p.n_aunts, p.aunts_per_segment);
        return 0;
    }
    for (uint32_t W = 1; W <= 32; W *= 2)
        for (uint32_t w = 1; w <= W; w *= 2)
            for (uint32_t s0 = 0; s0 < W; s0++)
                for (uint32_t e0 = s0 + 1; e0 <= W; e0++)
                    if (print_cover(W, w, s0, e0)) return 1;
    // the widest row: runs of 1024 nodes, every height below, unaligned ends
    const uint32_t spot[][3] = {{1, 0, 1024},   {1, 0, 1023},  {1, 1, 1024},   {64, 0, 1024}, {64, 64, 1023},
                                {1024, 0, 1024}, {1024, 0, 1023}, {512, 512, 1023}, {16, 16, 1001}, {2, 2, 65},
                                {1, 63, 128},    {1, 64, 129},  {32, 7, 1000}};
    for (const auto& s : spot)
        if (print_cover(1024, s[0], s[1], s[2])) return 1;
    return 0;
}
