// namespace_proofs_plan.h -- the host side of a batch of namespace queries of
// one resident square (namespace_proofs.hip, cda_square_namespace_plan /
// _proofs): the queries' check, the word the search kernel returns per (query,
// row) and the pass that turns those words into the segments of the answer and
// the sizes of its flat arrays.  Plain C++ (no HIP headers), so a host compiler
// builds and tests it (tools/namespace_plan_host_test.cpp).
//
// nmt v0.22.0 ProveNamespace of a row tree: with `less` leaves of a namespace
// below ns and `equal` leaves of ns itself, the proof is the inclusion proof of
// [less, less + equal) if equal > 0, else the absence proof of leaf `less`,
// ProveRange(less, less + 1) with that leaf's node.  A row takes part iff
// min(root) <= ns <= max(root) (GetSharesByNamespace's row selection).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "tree_index.h"

namespace cda {

constexpr uint32_t kNamespaceBytes = 29;

// The search's word of one (query, row): 0 when the row is not selected.
constexpr uint32_t kNsSelected = 1u << 31, kNsCountBits = 12, kNsCountMask = (1u << kNsCountBits) - 1;
CDA_INDEX_HD constexpr uint32_t namespace_word(uint32_t less, uint32_t equal) {
    return kNsSelected | (equal << kNsCountBits) | less;
}

constexpr uint8_t kNsInclusion = 1, kNsAbsence = 2;   // CDA_NAMESPACE_* of include/cda.h

// One row of one query's answer: the leaf range [s0, e0) of the row tree.
struct NamespaceSegment {
    uint32_t query, row, s0, e0;
    uint8_t kind;
    uint32_t shares() const { return kind == kNsInclusion ? e0 - s0 : 0; }
};

struct NamespacePlan {
    uint64_t n_segments = 0, n_nodes = 0, n_shares = 0;
};

// "" or the text of the first error, which names the query.
inline std::string namespace_queries_check(uint32_t k, const uint8_t* namespaces, uint32_t n) {
    if (!is_pow2(k) || k > 1024)
        return "square width " + std::to_string(k) + " is not a power of two <= 1024";
    if (n && !namespaces) return "null buffer";
    uint8_t parity[kNamespaceBytes];
    std::memset(parity, 0xFF, sizeof(parity));
    for (uint32_t q = 0; q < n; q++)
        if (!std::memcmp(namespaces + (size_t)q * kNamespaceBytes, parity, kNamespaceBytes))
            return "query " + std::to_string(q) + ": namespace is the parity shares namespace";
    return "";
}

// The answer of n queries from the search's n * k words (query-major): the
// sizes into *out and, if segs is not NULL, the segments in query then row
// order with seg_off[q] .. seg_off[q + 1] those of query q (n + 1 entries).
// "" or the text of the first error with *out untouched: a word that no search
// of a width-k square returns, or offsets beyond the arrays' 32-bit offsets.
inline std::string namespace_proofs_plan(uint32_t k, const uint32_t* words, uint32_t n, NamespacePlan* out,
                                         std::vector<NamespaceSegment>* segs = nullptr,
                                         std::vector<uint32_t>* seg_off = nullptr) {
    const uint32_t D = ceil_log2(2 * k);
    NamespacePlan p;
    if (segs) segs->clear();
    if (seg_off) seg_off->assign(1, 0);
    for (uint32_t q = 0; q < n; q++) {
        for (uint32_t r = 0; r < k; r++) {
            const uint32_t w = words[(size_t)q * k + r];
            if (!(w & kNsSelected)) continue;
            const uint32_t less = w & kNsCountMask, equal = (w >> kNsCountBits) & kNsCountMask;
            // a selected row has a leaf of a namespace >= ns among its first k
            if (less + equal > k || (equal == 0 && less >= k))
                return "query " + std::to_string(q) + ": row " + std::to_string(r) + ": search word " +
                       std::to_string(w) + " is not one of a square of width " + std::to_string(k);
            const NamespaceSegment sg{q, r, less, equal ? less + equal : less + 1, equal ? kNsInclusion : kNsAbsence};
            p.n_segments++;
            p.n_nodes += range_proof_count(D, sg.s0, sg.e0);
            p.n_shares += sg.shares();
            if (segs) segs->push_back(sg);
        }
        // seg_off and node_off are uint32_t; the proof kernel counts share units in 32 bits
        if (p.n_segments > UINT32_MAX || p.n_nodes > UINT32_MAX || p.n_shares / 16 + 2 * p.n_segments > (uint64_t)INT32_MAX)
            return "query " + std::to_string(q) + ": the answers up to here do not fit the batch's 32-bit offsets";
        if (seg_off) seg_off->push_back((uint32_t)p.n_segments);
    }
    *out = p;
    return "";
}

}  // namespace cda
