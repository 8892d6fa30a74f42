// commitment_proofs_plan.h -- the host side of a batch of blob commitment
// proofs of one square (share_proofs.hip, cda_square_commitment_proofs[_plan])
// and the cover both sides of the proof share: which nodes of a row tree are
// the subtree roots of a leaf range.  Plain C++ (no HIP headers), so a host
// compiler builds and tests it (tools/commitment_cover_host_test.cpp); the
// cover is also device code.
//
// A blob (start, share_len) of the k x k original square is normalised to
// inclusion.NextShareIndex: start rounded up to a multiple of w =
// SubTreeWidth(share_len, threshold).  w is a power of two <= k, so every row
// the blob touches holds a leaf range [s0, e0) whose s0 is a multiple of w
// (share_proofs_plan.h: for_each_segment).
//
// The cover.  The subtree roots of [s0, e0) with width w are the greedy
// aligned cover: from c = s0 take the largest power of two r <= w with c % r
// == 0 and c + r <= e0, emit node c / r of level log2 r, go on from c + r
// (pkg/inclusion/paths.go calculateSubTreeRootCoordinates, restated).  With s0
// a multiple of w that is (e0 - s0) / w nodes of level log2 w and then one
// node per set bit of (e0 - s0) % w, highest first; subtree_cover_item finds
// item i of any range in O(log w) steps without listing the run.
#pragma once
#include <cstdint>
#include <string>

#include "share_proofs_plan.h"
#include "tree_index.h"

namespace cda {

namespace square {
uint32_t subtree_width(uint32_t share_count, uint32_t threshold);   // square_plan.cpp: inclusion.SubTreeWidth
}

// One step of the cover at leaf c: the log2 of the largest power of two r <= w
// with c % r == 0 and c + r <= e0 (c < e0).
CDA_INDEX_HD constexpr uint32_t subtree_cover_step(uint32_t c, uint32_t e0, uint32_t log_w) {
    uint32_t l = log_w;
    while (l > 0 && ((c & ((1u << l) - 1u)) != 0 || c + (1u << l) > e0)) l--;
    return l;
}

// Item i of the cover of [s0, e0), 0 <= s0 < e0, w = 2^log_w: (level, index) of
// the row tree.  want == 0xFFFFFFFF counts instead: the result's index is the
// number of items.  A run of nodes of level log_w is skipped in one step.
CDA_INDEX_HD constexpr TreeNode subtree_cover_walk(uint32_t s0, uint32_t e0, uint32_t log_w, uint32_t want) {
    uint32_t c = s0, seen = 0;
    while (c < e0) {
        const uint32_t l = subtree_cover_step(c, e0, log_w);
        const uint32_t run = l == log_w ? (e0 - c) >> l : 1u;   // below log_w the next step differs
        if (want - seen < run) return TreeNode{l, (c >> l) + (want - seen)};
        seen += run;
        c += run << l;
    }
    return TreeNode{0, seen};
}

CDA_INDEX_HD constexpr uint32_t subtree_cover_count(uint32_t s0, uint32_t e0, uint32_t w) {
    return subtree_cover_walk(s0, e0, ceil_log2(w), 0xFFFFFFFFu).index;
}

CDA_INDEX_HD constexpr TreeNode subtree_cover_item(uint32_t s0, uint32_t e0, uint32_t w, uint32_t i) {
    return subtree_cover_walk(s0, e0, ceil_log2(w), i);
}

struct CommitmentProofsPlan {
    uint32_t n_segments = 0, n_roots = 0, n_nodes = 0, n_aunts = 0, aunts_per_segment = 0;
};

// One checked blob: its normalised start and its width.
struct NormalisedBlob {
    uint32_t start, end, w;
};

// Checks blob i and normalises it: "" and *out, or the error's text.
inline std::string normalise_blob(uint32_t k, uint32_t i, uint32_t start, uint32_t share_len, uint32_t threshold,
                                  NormalisedBlob* out) {
    const std::string at = "blob " + std::to_string(i) + ": ";
    const uint64_t cells = (uint64_t)k * k;
    if (share_len == 0) return at + "share_len is 0";
    if (share_len > cells)
        return at + "share_len " + std::to_string(share_len) + " is beyond the " + std::to_string(cells) +
               " shares of the original square";
    const uint32_t w = square::subtree_width(share_len, threshold);
    const uint64_t s = ((uint64_t)start + w - 1) / w * w;   // inclusion.NextShareIndex
    if (s + share_len > cells)
        return at + "start " + std::to_string(start) + " (normalised " + std::to_string(s) + ") with share_len " +
               std::to_string(share_len) + " ends beyond the " + std::to_string(cells) +
               " shares of the original square";
    *out = NormalisedBlob{(uint32_t)s, (uint32_t)(s + share_len), w};
    return "";
}

// Checks the batch and sizes it: "" and *out, or the text of the first error
// (which names the blob and the field) with *out untouched.
inline std::string commitment_proofs_plan(uint32_t k, const uint32_t* starts, const uint32_t* share_lens, uint32_t n,
                                          uint32_t threshold, CommitmentProofsPlan* out) {
    if (!is_pow2(k) || k > 1024)
        return "square width " + std::to_string(k) + " is not a power of two <= 1024";
    if (threshold == 0) return "subtree root threshold must be positive";
    if (n && (!starts || !share_lens)) return "null buffer";
    const uint32_t D = ceil_log2(2 * k), A = D + 1;
    const uint64_t limit = UINT32_MAX;
    uint64_t segments = 0, nodes = 0, roots = 0;
    for (uint32_t i = 0; i < n; i++) {
        NormalisedBlob b{};
        const std::string bad = normalise_blob(k, i, starts[i], share_lens[i], threshold, &b);
        if (!bad.empty()) return bad;
        const std::string at = "blob " + std::to_string(i) + ": ";
        // the rows between the first and the last are whole: [0, k), the same counts each
        const uint32_t r0 = b.start / k, r1 = (b.end - 1) / k;
        const uint32_t s0 = b.start % k, e0 = (b.end - 1) % k + 1;
        segments += r1 - r0 + 1;
        if (r0 == r1) {
            nodes += range_proof_count(D, s0, e0);
            roots += subtree_cover_count(s0, e0, b.w);
        } else {
            nodes += range_proof_count(D, s0, k) + range_proof_count(D, 0, e0) +
                     (uint64_t)(r1 - r0 - 1) * range_proof_count(D, 0, k);
            roots += subtree_cover_count(s0, k, b.w) + subtree_cover_count(0, e0, b.w) +
                     (uint64_t)(r1 - r0 - 1) * subtree_cover_count(0, k, b.w);
        }
        // seg_off, root_off, node_off and aunt_off of the batch are uint32_t
        if (segments > limit)
            return at + "segment offset " + std::to_string(segments) + " does not fit the batch's 32-bit offsets";
        if (roots > limit)
            return at + "subtree root offset " + std::to_string(roots) + " does not fit the batch's 32-bit offsets";
        if (nodes > limit)
            return at + "node offset " + std::to_string(nodes) + " does not fit the batch's 32-bit offsets";
        if (segments * A > limit)
            return at + "aunt offset " + std::to_string(segments * A) + " does not fit the batch's 32-bit offsets";
    }
    out->n_segments = (uint32_t)segments;
    out->n_roots = (uint32_t)roots;
    out->n_nodes = (uint32_t)nodes;
    out->n_aunts = (uint32_t)(segments * A);
    out->aunts_per_segment = A;
    return "";
}

}  // namespace cda
