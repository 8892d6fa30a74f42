// Host test of csrc/namespace_proofs_plan.h (no GPU): the queries' check and the
// pass from the search's words to segments, offsets and sizes, for a k = 4
// square.  Prints one line per case; tests/test_namespace_plan.py compares them
// with values worked out by hand.
//   P name : n_segments n_nodes n_shares | seg_off... | query row s0 e0 kind ...
//   E name : the error text
#include <cstdio>
#include <cstring>
#include <vector>

#include "namespace_proofs_plan.h"

using namespace cda;

static void run(const char* name, uint32_t k, const std::vector<uint32_t>& words, uint32_t n) {
    NamespacePlan p;
    p.n_segments = 77;   // must stay on an error
    std::vector<NamespaceSegment> segs;
    std::vector<uint32_t> off;
    const std::string bad = namespace_proofs_plan(k, words.data(), n, &p, &segs, &off);
    if (!bad.empty()) {
        std::printf("E %s : %s%s\n", name, bad.c_str(), p.n_segments == 77 ? "" : " (plan touched)");
        return;
    }
    NamespacePlan sizes_only;
    if (!namespace_proofs_plan(k, words.data(), n, &sizes_only).empty() || sizes_only.n_segments != p.n_segments ||
        sizes_only.n_nodes != p.n_nodes || sizes_only.n_shares != p.n_shares || segs.size() != p.n_segments) {
        std::printf("E %s : the sizes-only pass differs\n", name);
        return;
    }
    std::printf("P %s : %llu %llu %llu |", name, (unsigned long long)p.n_segments, (unsigned long long)p.n_nodes,
                (unsigned long long)p.n_shares);
    for (uint32_t o : off) std::printf(" %u", o);
    std::printf(" |");
    for (const NamespaceSegment& s : segs) std::printf(" %u %u %u %u %u", s.query, s.row, s.s0, s.e0, s.kind);
    std::printf("\n");
}

int main() {
    const uint32_t k = 4;
    run("none", k, {}, 0);
    run("unselected", k, {0, 0, 0, 0}, 1);
    // query 0: row 1 holds leaves [1, 4) of it, row 2 the whole row, row 3 its first leaf;
    // query 1: nothing; query 2: absent before leaf 2 of row 0, present as leaf 0 of row 1
    run("mixed", k,
        {0, namespace_word(1, 3), namespace_word(0, 4), namespace_word(0, 1),
         0, 0, 0, 0,
         namespace_word(2, 0), namespace_word(0, 1), 0, 0}, 3);
    run("absence_at_k", k, {namespace_word(4, 0), 0, 0, 0}, 1);
    run("too_many", k, {0, 0, 0, 0, 0, namespace_word(3, 2), 0, 0}, 2);

    uint8_t ns[3 * 29];
    std::memset(ns, 0, sizeof(ns));
    std::memset(ns + 29, 0xFF, 29);
    ns[2 * 29 - 1] = 0xFE;   // the tail padding namespace is a namespace like any other
    std::printf("E check_ok : %s\n", namespace_queries_check(k, ns, 3).c_str());
    ns[2 * 29 - 1] = 0xFF;
    std::printf("E check_parity : %s\n", namespace_queries_check(k, ns, 3).c_str());
    std::printf("E check_null : %s\n", namespace_queries_check(k, nullptr, 1).c_str());
    std::printf("E check_width : %s\n", namespace_queries_check(3, ns, 0).c_str());
    return 0;
}
