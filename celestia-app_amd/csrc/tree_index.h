// tree_index.h -- index arithmetic of the proof paths: which nodes of a
// Merkle tree a range proof takes and where a level of a resident square's
// trees lies.  Plain C++ (no HIP headers), so a host compiler builds and tests
// it (tools/tree_index_host_test.cpp, tools/range_proof_host_test.cpp);
// level_offset and the closed-form range proof are also device code.
//
// The trees pair adjacent nodes level by level and promote an odd last node
// unchanged, which builds the RFC-6962 tree (split at the largest power of two
// below n): the subtree over leaves [lo, lo + 2^L) is node lo >> L of level L.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define CDA_INDEX_HD __host__ __device__
#else
#define CDA_INDEX_HD
#endif

namespace cda {

constexpr bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// The smallest l with 2^l >= x.
constexpr uint32_t ceil_log2(uint32_t x) {
    uint32_t l = 0;
    while ((uint64_t{1} << l) < x) l++;
    return l;
}

// Level sizes of the tree over n leaves: n, ceil(n/2), ..., 1.
inline std::vector<uint32_t> level_counts(uint32_t n) {
    std::vector<uint32_t> c{n};
    while (c.back() > 1) c.push_back((c.back() + 1) / 2);
    return c;
}

// nmt ProveRange / buildRangeProof node order for the range [start, end) of
// the tree over leaves [lo, hi): the maximal subtrees outside the range, depth
// first, left to right, as (level, index).
inline void prove_nodes(uint32_t lo, uint32_t hi, uint32_t start, uint32_t end,
                        std::vector<std::pair<uint32_t, uint32_t>>& out) {
    if (hi <= start || lo >= end) {
        const uint32_t L = ceil_log2(hi - lo);
        out.emplace_back(L, lo >> L);
        return;
    }
    if (hi - lo == 1) return;   // a leaf inside the range
    uint32_t k = 1;
    while (2 * k < hi - lo) k *= 2;   // largest power of two < n (RFC-6962 split)
    prove_nodes(lo, lo + k, start, end, out);
    prove_nodes(lo + k, hi, start, end, out);
}

// Bytes from the start of a resident square's level buffer to level L, for
// W trees of W leaves in slots of `slot` bytes: level l is [W][W >> l][slot].
// first: the lowest level the buffer holds (0 for the rows, whose buffer
// starts with the leaf slots; 1 for the columns).
CDA_INDEX_HD constexpr uint64_t level_offset(uint32_t W, uint32_t L, uint32_t first, uint32_t slot) {
    uint64_t off = 0;
    for (uint32_t l = first; l < L; l++) off += (uint64_t)W * (W >> l) * slot;
    return off;
}

// The closed form of prove_nodes for a perfect tree of 2^D leaves (a resident
// square's row trees), usable on the device: the proof of [s, e), 0 <= s < e
// <= 2^D, lists
//   left of the range:  for every set bit L of s, from L = D - 1 down to 0,
//                       node (s >> L) - 1 of level L;
//   right of the range: for every clear bit L of e - 1, from L = 0 up to
//                       D - 1, node ((e - 1) >> L) + 1 of level L.
// For e = s + 1 this is the sibling rule of sample.hip.  prove_nodes (any leaf
// count) is the check: tools/range_proof_host_test.cpp.
CDA_INDEX_HD constexpr uint32_t popcount32(uint32_t x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (((x + (x >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}

CDA_INDEX_HD constexpr uint32_t range_proof_count(uint32_t D, uint32_t s, uint32_t e) {
    return popcount32(s) + D - popcount32(e - 1);
}

struct TreeNode {
    uint32_t level, index;
};

// Node q of that proof, q < range_proof_count(D, s, e).  Every level is
// visited whatever q is, so lanes of one wavefront that ask for different q of
// the same range run the same instructions.
CDA_INDEX_HD constexpr TreeNode range_proof_node(uint32_t D, uint32_t s, uint32_t e, uint32_t q) {
    const uint32_t n_left = popcount32(s), last = e - 1;
    TreeNode node{0, 0};
    uint32_t seen = 0;
    for (uint32_t i = 0; i < D; i++) {   // left nodes, top down
        const uint32_t L = D - 1 - i;
        if ((s >> L) & 1u) {
            if (seen == q) node = TreeNode{L, (s >> L) - 1};
            seen++;
        }
    }
    seen = n_left;
    for (uint32_t L = 0; L < D; L++) {   // right nodes, bottom up
        if (!((last >> L) & 1u)) {
            if (seen == q) node = TreeNode{L, (last >> L) + 1};
            seen++;
        }
    }
    return node;
}

}  // namespace cda
