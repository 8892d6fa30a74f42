// share_proofs_plan.h -- the host side of a batch of share-range proofs of one
// square (share_proofs.hip, cda_square_share_proofs[_plan]): the ranges'
// checks, the rows ("segments") each range covers and the sizes of the flat
// arrays the batch fills.  Plain C++ (no HIP headers), so a host compiler
// builds and tests it (tools/range_proof_host_test.cpp).
//
// A range [start, end) of the k x k original square covers the rows start / k
// .. (end - 1) / k; in row r it is the leaf range [s0, e0) of the row tree of
// W = 2k leaves, s0 = start % k in the first row (else 0), e0 = (end - 1) % k
// + 1 in the last (else k).  The segment has range_proof_count(log2 W, s0, e0)
// proof nodes, log2(4k) aunts and e0 - s0 shares.
#pragma once
#include <cstdint>
#include <string>

#include "tree_index.h"

namespace cda {

struct ShareProofsPlan {
    uint32_t n_segments = 0, n_nodes = 0, n_aunts = 0, aunts_per_segment = 0;
    uint64_t n_shares = 0;
};

// One row of one range.
struct ShareProofSegment {
    uint32_t proof, row, s0, e0;
};

// fn(ShareProofSegment) for every segment of a checked range, in row order.
template <class F>
inline void for_each_segment(uint32_t k, uint32_t proof, uint32_t start, uint32_t end, F&& fn) {
    const uint32_t r0 = start / k, r1 = (end - 1) / k;
    for (uint32_t r = r0; r <= r1; r++)
        fn(ShareProofSegment{proof, r, r == r0 ? start % k : 0, r == r1 ? (end - 1) % k + 1 : k});
}

// Checks the batch and sizes it: "" and *out, or the text of the first error
// (which names the range and the field) with *out untouched.
inline std::string share_proofs_plan(uint32_t k, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                                     ShareProofsPlan* out) {
    if (!is_pow2(k) || k > 1024)
        return "square width " + std::to_string(k) + " is not a power of two <= 1024";
    if (n && (!starts || !ends)) return "null buffer";
    const uint32_t D = ceil_log2(2 * k), A = D + 1;
    const uint64_t limit = UINT32_MAX;
    uint64_t segments = 0, nodes = 0, shares = 0;
    for (uint32_t i = 0; i < n; i++) {
        const std::string at = "range " + std::to_string(i) + ": ";
        if (starts[i] >= ends[i])
            return at + "start " + std::to_string(starts[i]) + " is not below end " + std::to_string(ends[i]);
        if (ends[i] > k * k)
            return at + "end " + std::to_string(ends[i]) + " is beyond the " + std::to_string(k * k) +
                   " shares of the original square";
        // the rows between the first and the last are whole: [0, k), the same count each
        const uint32_t r0 = starts[i] / k, r1 = (ends[i] - 1) / k;
        const uint32_t s0 = starts[i] % k, e0 = (ends[i] - 1) % k + 1;
        segments += r1 - r0 + 1;
        if (r0 == r1)
            nodes += range_proof_count(D, s0, e0);
        else
            nodes += range_proof_count(D, s0, k) + range_proof_count(D, 0, e0) +
                     (uint64_t)(r1 - r0 - 1) * range_proof_count(D, 0, k);
        shares += ends[i] - starts[i];
        // seg_off, node_off and aunt_off of the batch are uint32_t
        if (segments > limit)
            return at + "segment offset " + std::to_string(segments) + " does not fit the batch's 32-bit offsets";
        if (nodes > limit)
            return at + "node offset " + std::to_string(nodes) + " does not fit the batch's 32-bit offsets";
        if (segments * A > limit)
            return at + "aunt offset " + std::to_string(segments * A) + " does not fit the batch's 32-bit offsets";
    }
    out->n_segments = (uint32_t)segments;
    out->n_nodes = (uint32_t)nodes;
    out->n_aunts = (uint32_t)(segments * A);
    out->aunts_per_segment = A;
    out->n_shares = shares;
    return "";
}

}  // namespace cda
