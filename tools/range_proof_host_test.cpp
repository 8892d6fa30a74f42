// Host dump and self-check of the closed-form range proof of csrc/tree_index.h
// (range_proof_count / range_proof_node) and of csrc/share_proofs_plan.h, for
// tests/test_range_proof_index.py.  Build: g++ -std=c++20 -I celestia-app_amd/csrc
// (plain host C++: also the program to build with -fsanitize=address,undefined).
//   R W s e : level index ...    range_proof_node for every range, W in 1..64 (powers of two),
//                                and the spot checks at W = 2048
//   P k n_ranges : n_segments n_nodes n_aunts aunts_per_segment n_shares     share_proofs_plan
//   E k : message                share_proofs_plan's error text
// Every R line is compared here with prove_nodes (order and count); a
// difference is reported on stderr and fails the program.
#include <cstdio>
#include <string>
#include <vector>

#include "share_proofs_plan.h"
#include "tree_index.h"

namespace {

int failures = 0;

void range_line(uint32_t W, uint32_t s, uint32_t e) {
    const uint32_t D = cda::ceil_log2(W);
    std::vector<std::pair<uint32_t, uint32_t>> want;
    cda::prove_nodes(0, W, s, e, want);
    const uint32_t n = cda::range_proof_count(D, s, e);
    printf("R %u %u %u :", W, s, e);
    bool same = n == want.size();
    for (uint32_t q = 0; q < n; q++) {
        const cda::TreeNode nd = cda::range_proof_node(D, s, e, q);
        printf(" %u %u", nd.level, nd.index);
        same = same && q < want.size() && want[q].first == nd.level && want[q].second == nd.index;
    }
    printf("\n");
    if (!same) {
        fprintf(stderr, "closed form differs from prove_nodes: W %u [%u, %u)\n", W, s, e);
        failures++;
    }
}

void plan_line(uint32_t k, const std::vector<uint32_t>& starts, const std::vector<uint32_t>& ends) {
    cda::ShareProofsPlan p;
    const std::string err = cda::share_proofs_plan(k, starts.data(), ends.data(), (uint32_t)starts.size(), &p);
    if (!err.empty()) {
        printf("E %u : %s\n", k, err.c_str());
        return;
    }
    printf("P %u %zu : %u %u %u %u %llu\n", k, starts.size(), p.n_segments, p.n_nodes, p.n_aunts, p.aunts_per_segment,
           (unsigned long long)p.n_shares);
    // the plan's closed sum over whole middle rows against the segments one by one
    uint64_t segs = 0, nodes = 0;
    for (size_t i = 0; i < starts.size(); i++)
        cda::for_each_segment(k, (uint32_t)i, starts[i], ends[i], [&](const cda::ShareProofSegment& g) {
            segs++;
            nodes += cda::range_proof_count(cda::ceil_log2(2 * k), g.s0, g.e0);
        });
    if (segs != p.n_segments || nodes != p.n_nodes) {
        fprintf(stderr, "plan differs from its segments: k %u\n", k);
        failures++;
    }
}

}  // namespace

int main() {
    static_assert(cda::popcount32(0) == 0 && cda::popcount32(0xFFFFFFFFu) == 32 && cda::popcount32(0x80000001u) == 2);
    static_assert(cda::range_proof_count(3, 5, 6) == 3 && cda::range_proof_node(3, 5, 6, 0).level == 2);
    for (uint32_t W = 1; W <= 64; W *= 2)
        for (uint32_t s = 0; s < W; s++)
            for (uint32_t e = s + 1; e <= W; e++) range_line(W, s, e);
    for (uint32_t s : {0u, 1u, 1023u, 1024u, 2047u})
        for (uint32_t e : {s + 1, 1024u, 2048u})
            if (e > s) range_line(2048, s, e);

    plan_line(1, {0}, {1});
    plan_line(2, {0, 1, 0, 3}, {2, 3, 4, 4});
    plan_line(4, {2, 4, 3, 0, 5}, {4, 6, 11, 16, 6});
    plan_line(4, {}, {});
    plan_line(128, {0, 0}, {128 * 128, 1});
    plan_line(4, {0, 5, 3}, {1, 5, 4});     // start == end
    plan_line(4, {0, 7}, {1, 6});           // start > end
    plan_line(8, {0, 1, 2, 3}, {1, 2, 3, 70});
    plan_line(3, {0}, {1});
    plan_line(2048, {0}, {1});
    plan_line(0, {0}, {1});
    // 349 526 whole k = 1024 squares: 357 914 624 segments of 12 aunts pass 2^32
    const std::vector<uint32_t> zeros(349526, 0), whole(349526, 1024u * 1024u);
    plan_line(1024, zeros, whole);
    return failures ? 1 : 0;
}
