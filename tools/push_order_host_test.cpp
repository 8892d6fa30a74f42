// Host dump of csrc/push_order.h for tests/test_push_order.py, which compares
// it with the reference's order of checks (row trees before column trees,
// then the lower tree, then the earlier push).
// Build: g++ -std=c++20 -I celestia-app_amd/csrc.
//   (no arguments)          the corner words, kOrdered and fill_status:
//     E axis index pos word       encode, and what decode makes of the word:
//     D word axis index pos
//     S word status               fill_status
//   min a,i,p a,i,p ...     M word axis index pos   the minimum of the encoded
//                            violations, started from kOrdered as the kernels do
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "push_order.h"

namespace po = cda::push_order;

static void dump_decoded(char tag, uint32_t w) {
    const po::Violation v = po::decode(w);
    printf("%c %u %d %u %u\n", tag, w, v.axis, v.index, v.pos);
}

int main(int argc, char** argv) {
    static_assert(po::decode(po::kOrdered).axis == -1 && po::decode(po::kOrdered).index == 0 &&
                  po::decode(po::kOrdered).pos == 0);
    static_assert(po::encode(1, 4095, 4095) < po::kOrdered, "no violation word collides with kOrdered");
    if (argc > 1 && strcmp(argv[1], "min") == 0) {
        uint32_t key = po::kOrdered;
        for (int i = 2; i < argc; i++) {
            unsigned a, x, p;
            if (sscanf(argv[i], "%u,%u,%u", &a, &x, &p) != 3) return 2;
            key = std::min(key, po::encode(a, x, p));
        }
        dump_decoded('M', key);
        return 0;
    }
    std::vector<uint32_t> words;
    for (uint32_t axis : {0u, 1u})
        for (uint32_t index : {0u, 1u, 4095u})
            for (uint32_t pos : {1u, 3u, 4095u}) {
                const uint32_t w = po::encode(axis, index, pos);
                printf("E %u %u %u %u\n", axis, index, pos, w);
                words.push_back(w);
            }
    words.push_back(po::kOrdered);
    for (uint32_t w : words) dump_decoded('D', w);
    std::vector<int32_t> status(words.size(), 99);
    po::fill_status(words.data(), words.size(), status.data());
    po::fill_status(words.data(), words.size(), nullptr);   // no status wanted: a no-op
    for (size_t i = 0; i < words.size(); i++) printf("S %u %d\n", words[i], status[i]);
    return 0;
}
