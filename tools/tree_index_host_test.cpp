// Host dump of csrc/tree_index.h for tests/test_tree_index.py, which compares
// it with the oracle's split rule.  Build: g++ -std=c++20 -I celestia-app_amd/csrc.
//   P n start end : level index ...    prove_nodes for every range, n in 1..33
//   C n : count ...                    level_counts(n)
//   O W first L offset                 level_offset, rows (first 0) and columns (first 1)
#include <cstdio>

#include "tree_index.h"

int main() {
    static_assert(cda::is_pow2(1) && cda::is_pow2(2048) && !cda::is_pow2(0) && !cda::is_pow2(33));
    static_assert(cda::ceil_log2(1) == 0 && cda::ceil_log2(2) == 1 && cda::ceil_log2(33) == 6 &&
                  cda::ceil_log2(4096) == 12);
    for (uint32_t n = 1; n <= 33; n++) {
        printf("C %u :", n);
        for (uint32_t c : cda::level_counts(n)) printf(" %u", c);
        printf("\n");
        for (uint32_t s = 0; s < n; s++)
            for (uint32_t e = s + 1; e <= n; e++) {
                std::vector<std::pair<uint32_t, uint32_t>> nodes;
                cda::prove_nodes(0, n, s, e, nodes);
                printf("P %u %u %u :", n, s, e);
                for (const auto& [level, index] : nodes) printf(" %u %u", level, index);
                printf("\n");
            }
    }
    for (uint32_t W : {2u, 4u, 16u, 2048u})
        for (uint32_t first = 0; first < 2; first++)
            for (uint32_t L = first; L <= cda::ceil_log2(W) + 1; L++)
                printf("O %u %u %u %llu\n", W, first, L, (unsigned long long)cda::level_offset(W, L, first, 96));
    return 0;
}
