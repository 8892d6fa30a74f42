// namespace_proofs.hip -- all shares of many namespaces of a resident square
// with nmt ProveNamespace's proofs (EXT nmt v0.22.0: inclusion of the whole run,
// or absence), the rows chosen as GetSharesByNamespace chooses them from the
// DAH: cda_square_namespace_plan / cda_square_namespace_proofs.
//
// Two launches per call, whatever the number of queries and the run lengths:
//   1. namespace_search_kernel (here): where each namespace lies in each row.
//   2. the proof kernel of share_proofs.hip, driven by the segment table the
//      host makes of the search's words (namespace_proofs_plan.h,
//      Engine::emit_segments): an inclusion segment is a share range's segment,
//      an absence segment has no share units and one more staged slot, its leaf.
//
// Search mapping.  One wavefront per (query, block of 64 rows), one lane per
// row.  Each lane compares ns with the min and the max namespace of its row's
// root slot; a ballot gives the selected rows of the block.  For each of them
// in turn the 64 lanes stride over the row's first k leaf slots (level 0 of the
// row levels: the namespace is the slot's first 29 bytes) and count the leaves
// below ns and the leaves of ns by ballot and popcount: no sortedness is
// assumed, and every branch is uniform over the wave.  The result is one word
// per (query, row < k) (namespace_word: selected, equal, less), n * k * 4 bytes
// in one copy back; rows >= k are never selected (their min is the parity
// namespace, which no query may be).
//
// Sets.  The same two launches serve queries across a set of resident squares
// (cda_square_set_namespace_plan / _proofs): query q names its member in
// squares[q], namespace_search_kernel<true> reads that member's root slots and
// leaf level from the arenas' bases and strides, the words stay [n][k], and
// every segment of the table names its square beside its row (segment_table.h).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "namespace_proofs_plan.h"
#include "out_regions.h"
#include "push_order.h"
#include "resident_proof_dev.h"
#include "segment_table.h"
#include "sha256_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

static_assert(kNamespaceBytes == (uint32_t)kNs && kNsInclusion == CDA_NAMESPACE_INCLUSION &&
              kNsAbsence == CDA_NAMESPACE_ABSENCE);

constexpr uint32_t kSearchWaves = 4;   // (query, row block) pairs per workgroup

struct SearchArgs {
    ResidentView sq;
    const uint8_t* namespaces;   // [n][29]
    uint32_t n, row_blocks;
    uint32_t* words;             // [n][k]
    const uint32_t* squares;     // a set: [n], the member each query is of
};

// A namespace as eight big-endian words (the last holds byte 28 in its top byte), from any address ...
__device__ __forceinline__ void load_ns_bytes(const uint8_t* p, uint32_t (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (4 * j + q < kNs) v |= (uint32_t)p[4 * j + q] << (24 - 8 * q);
        w[j] = v;
    }
}
// ... and from the start of a node slot (16-byte aligned).
__device__ __forceinline__ void load_ns_slot(const uint8_t* slot, uint32_t (&w)[8]) {
    const uint4 lo = reinterpret_cast<const uint4*>(slot)[0], hi = reinterpret_cast<const uint4*>(slot)[1];
    w[0] = bswap32(lo.x), w[1] = bswap32(lo.y), w[2] = bswap32(lo.z), w[3] = bswap32(lo.w);
    w[4] = bswap32(hi.x), w[5] = bswap32(hi.y), w[6] = bswap32(hi.z), w[7] = bswap32(hi.w) & 0xFF000000u;
}
// bytes.Compare of two namespaces: -1, 0, 1.
__device__ __forceinline__ int cmp_ns(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    int c = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (a[j] != b[j]) c = a[j] < b[j] ? -1 : 1;
    return c;
}

// kSet = false: the queries of the square a.sq.  kSet = true: queries across a set of resident squares --
// a.sq holds the arenas' bases, query q is of member a.squares[q] (validated on the host) and the wave reads
// that member's strides of the root slots and the row levels.
template <bool kSet>
__global__ __launch_bounds__(64 * kSearchWaves) void namespace_search_kernel(const SearchArgs a, const SetStrides sq) {
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t g = blockIdx.x * kSearchWaves + wave;
    if (g >= a.n * a.row_blocks) return;   // uniform over the wave; the kernel has no barrier
    const uint32_t k = a.sq.k, W = 2 * k;
    const uint32_t q = g / a.row_blocks, row0 = (g % a.row_blocks) * 64, r = row0 + lane;
    const uint8_t* root_slots = a.sq.root_slots;
    const uint8_t* levels = a.sq.levels;
    if constexpr (kSet) {
        const uint64_t y = a.squares[q];
        root_slots += y * sq.root_slots;
        levels += y * sq.levels;
    }
    uint32_t ns[8];
    load_ns_bytes(a.namespaces + (uint64_t)q * kNs, ns);
    bool selected = false;
    if (r < k) {
        const uint8_t* root = root_slots + (uint64_t)r * kSlot;
        uint32_t mn[8], mx[8];
        load_ns_slot(root, mn);
        load_ns_bytes(root + kNs, mx);
        selected = cmp_ns(mn, ns) <= 0 && cmp_ns(ns, mx) <= 0;
    }
    unsigned long long rows = __ballot(selected);
    uint32_t word = 0;
    while (rows) {
        const uint32_t rl = (uint32_t)__ffsll(rows) - 1;
        rows &= rows - 1;
        const uint8_t* leaves = levels + (uint64_t)(row0 + rl) * W * kSlot;
        uint32_t less = 0, equal = 0;
        for (uint32_t base = 0; base < k; base += 64) {
            const uint32_t j = base + lane;
            int c = 1;
            if (j < k) {
                uint32_t leaf[8];
                load_ns_slot(leaves + (uint64_t)j * kSlot, leaf);
                c = cmp_ns(leaf, ns);
            }
            less += (uint32_t)__popcll(__ballot(c < 0));
            equal += (uint32_t)__popcll(__ballot(c == 0));
        }
        if (lane == rl) word = namespace_word(less, equal);
    }
    if (r < k) a.words[(uint64_t)q * k + r] = word;
}

}  // namespace

// What the calls that need nmt's own trees answer for a square whose push order failed.
int Engine::fail_unordered_square(const ResidentSquare* sq, const char* why) {
    return fail_unordered_square(sq->push_err, "", why);
}

// `who`: "" or what names the square among the call's requests, ending in ": ".
int Engine::fail_unordered_square(uint32_t push_err, const std::string& who, const char* why) {
    const push_order::Violation v = push_order::decode(push_err);
    po_axis = v.axis;
    po_index = v.index;
    po_pos = v.pos;
    return fail(CDA_ERR_PUSH_ORDER, who + "the square's " + (v.axis == 0 ? "row " : "column ") +
                                        std::to_string(v.index) + " is not ordered by namespace at position " +
                                        std::to_string(v.pos) + ": " + why);
}

int Engine::square_namespace_search(ResidentSquare* sq, const uint8_t* namespaces, uint32_t n,
                                    std::vector<uint32_t>* words) {
    const uint32_t k = sq->k;
    const std::string bad = namespace_queries_check(k, namespaces, n);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    if (sq->push_err != push_order::kOrdered)
        return fail_unordered_square(sq, "nmt builds no tree of it, so no namespace proof");
    words->assign((size_t)n * k, 0);
    if (n == 0) return CDA_OK;
    const uint32_t row_blocks = (k + 63) / 64;
    if ((uint64_t)n * row_blocks > (uint64_t)INT32_MAX)
        return fail(CDA_ERR_INVALID, "too many queries for one launch");
    const size_t ns_bytes = OutRegions::align((size_t)n * kNs), word_bytes = (size_t)n * k * 4;
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->scratch, ns_bytes + word_bytes, "hipMalloc"));
    uint8_t* scr = sq->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, namespaces, (size_t)n * kNs, s, "H2D namespaces"));
    const SearchArgs a{sq->view(), scr, n, row_blocks, reinterpret_cast<uint32_t*>(scr + ns_bytes), nullptr};
    hipLaunchKernelGGL(namespace_search_kernel<false>, dim3((n * row_blocks + kSearchWaves - 1) / kSearchWaves),
                       dim3(64 * kSearchWaves), 0, s, a, SetStrides{});
    CDA_TRY(launched("namespace search"));
    CDA_TRY(d2h(words->data(), a.words, word_bytes, s, "D2H namespace search"));
    return sync(s);
}

// Query q is (squares[q], namespaces + 29 q): one upload of the namespaces with the squares behind them, one
// launch of the set instantiation over the arenas' bases, the n * k words back.
int Engine::square_set_namespace_search(ResidentSquareSet* set, const uint32_t* squares, const uint8_t* namespaces,
                                        uint32_t n, std::vector<uint32_t>* words) {
    const uint32_t k = set->k;
    if (n && !squares) return fail(CDA_ERR_INVALID, "null squares");
    if (n && !namespaces) return fail(CDA_ERR_INVALID, "null buffer");   // the single square's text
    for (uint32_t q = 0; q < n; q++)
        if (squares[q] >= set->n)
            return fail(CDA_ERR_INVALID, "query " + std::to_string(q) + ": square " + std::to_string(squares[q]) +
                                             " is not below the set's " + std::to_string(set->n) + " squares");
    const std::string bad = namespace_queries_check(k, namespaces, n);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    for (uint32_t q = 0; q < n; q++)
        if (set->push_err[squares[q]] != push_order::kOrdered)
            return fail_unordered_square(set->push_err[squares[q]],
                                         "query " + std::to_string(q) + ": square " + std::to_string(squares[q]) + ": ",
                                         "nmt builds no tree of it, so no namespace proof");
    words->assign((size_t)n * k, 0);
    if (n == 0) return CDA_OK;
    const uint32_t row_blocks = (k + 63) / 64;
    if ((uint64_t)n * row_blocks > (uint64_t)INT32_MAX)
        return fail(CDA_ERR_INVALID, "too many queries for one launch");
    // the upload: the namespaces, padded to a word, then the squares
    const size_t ns_words = ((size_t)n * kNs + 3) / 4, up_bytes = OutRegions::align((ns_words + n) * 4),
                 word_bytes = (size_t)n * k * 4;
    std::vector<uint32_t> up(ns_words + n, 0);
    std::memcpy(up.data(), namespaces, (size_t)n * kNs);
    std::memcpy(up.data() + ns_words, squares, (size_t)n * 4);
    hipStream_t s = stream_;
    CDA_TRY(ensure(set->scratch, up_bytes + word_bytes, "hipMalloc"));
    uint8_t* scr = set->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, up.data(), up.size() * 4, s, "H2D namespace queries"));
    const ResidentView base{set->eds.as<uint8_t>(), set->levels.as<uint8_t>(), set->col_levels.as<uint8_t>(),
                            set->roots_slots.as<uint8_t>(), set->rfc.as<uint32_t>(), k, set->log_w};
    const SearchArgs a{base, scr, n, row_blocks, reinterpret_cast<uint32_t*>(scr + up_bytes),
                       reinterpret_cast<const uint32_t*>(scr) + ns_words};
    const SetStrides st{set->eds_sq, set->levels_sq, set->col_levels_sq, set->roots_slots_sq, set->rfc_sq};
    hipLaunchKernelGGL(namespace_search_kernel<true>, dim3((n * row_blocks + kSearchWaves - 1) / kSearchWaves),
                       dim3(64 * kSearchWaves), 0, s, a, st);
    CDA_TRY(launched("namespace search of a set"));
    // `up` is pageable: complete before returning
    CDA_TRY(d2h(words->data(), a.words, word_bytes, s, "D2H namespace search"));
    return sync(s);
}

int Engine::square_namespace_plan(ResidentSquare* sq, const uint8_t* namespaces, uint32_t n,
                                  cda_namespace_plan_t* out) {
    std::vector<uint32_t> words;
    CDA_TRY(square_namespace_search(sq, namespaces, n, &words));
    NamespacePlan p;
    const std::string bad = namespace_proofs_plan(sq->k, words.data(), n, &p);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    *out = cda_namespace_plan_t{p.n_segments, p.n_nodes, p.n_shares};
    return CDA_OK;
}

int Engine::square_set_namespace_plan(ResidentSquareSet* set, const uint32_t* squares, const uint8_t* namespaces,
                                      uint32_t n, cda_namespace_plan_t* out) {
    std::vector<uint32_t> words;
    CDA_TRY(square_set_namespace_search(set, squares, namespaces, n, &words));
    NamespacePlan p;
    const std::string bad = namespace_proofs_plan(set->k, words.data(), n, &p);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    *out = cda_namespace_plan_t{p.n_segments, p.n_nodes, p.n_shares};
    return CDA_OK;
}

int Engine::square_namespace_proofs(ResidentSquare* sq, const uint8_t* namespaces, uint32_t n,
                                    const cda_namespace_proofs_out& o) {
    std::vector<uint32_t> words;
    CDA_TRY(square_namespace_search(sq, namespaces, n, &words));
    return namespace_segments(sq, nullptr, nullptr, words, n, o);
}

int Engine::square_set_namespace_proofs(ResidentSquareSet* set, const uint32_t* squares, const uint8_t* namespaces,
                                        uint32_t n, const cda_namespace_proofs_out& o) {
    std::vector<uint32_t> words;
    CDA_TRY(square_set_namespace_search(set, squares, namespaces, n, &words));
    return namespace_segments(nullptr, set, squares, words, n, o);
}

// The host pass and the proof launch of both: the search's words of one square (sq), or of the members
// squares[q] of a set, to the segment table; a set's segments name their squares beside their rows.
int Engine::namespace_segments(ResidentSquare* sq, ResidentSquareSet* set, const uint32_t* squares,
                               const std::vector<uint32_t>& words, uint32_t n, const cda_namespace_proofs_out& o) {
    const uint32_t k = sq ? sq->k : set->k, D = sq ? sq->log_w : set->log_w;
    std::vector<uint32_t> seg_off;
    NamespacePlan p;
    std::vector<NamespaceSegment> found;
    const std::string bad = namespace_proofs_plan(k, words.data(), n, &p, &found, &seg_off);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    const uint32_t S = (uint32_t)p.n_segments;
    if (o.seg_off)
        for (uint32_t q = 0; q <= n; q++) o.seg_off[q] = seg_off[q];
    if (o.node_off) o.node_off[0] = 0;
    if (o.share_off) o.share_off[0] = 0;
    if (S == 0) return CDA_OK;
    SegmentEmit em;
    em.up.resize((size_t)S * kSegWords);
    SegEntry* segs = em.segs();
    uint32_t node_at = 0, unit_at = 0;
    uint64_t share_at = 0;
    for (uint32_t g = 0; g < S; g++) {
        const NamespaceSegment& sg = found[g];
        const bool absence = sg.kind == kNsAbsence;
        segs[g] = SegEntry{seg_row_word(sg.row, squares ? squares[sg.query] : 0u),
                           sg.s0 | (sg.e0 << 16) | (absence ? kSegAbsence : 0u), node_at, unit_at, share_at,
                           sg.query, kNoFirstCell};
        if (o.row) o.row[g] = sg.row;
        if (o.kind) o.kind[g] = sg.kind;
        if (o.nmt_start) o.nmt_start[g] = (int32_t)sg.s0;
        if (o.nmt_end) o.nmt_end[g] = (int32_t)sg.e0;
        node_at += range_proof_count(D, sg.s0, sg.e0);
        unit_at += seg_units(sg.shares());
        share_at += sg.shares();
        if (o.node_off) o.node_off[g + 1] = node_at;
        if (o.share_off) o.share_off[g + 1] = share_at;
    }
    em.n_segs = S;
    em.n_units = unit_at;
    em.node_slots = p.n_nodes;
    em.n_shares = p.n_shares;
    em.nodes = o.nodes;
    em.shares = o.shares;
    em.absence_leaf = o.absence_leaf;
    return emit_segments(sq, set, em);
}

}  // namespace cda
