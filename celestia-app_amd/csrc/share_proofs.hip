// share_proofs.hip -- the one producer of share-inclusion proofs of a resident
// square (proof.NewShareInclusionProofFromEDS, pkg/proof/proof.go:77-145):
// any number of ranges in ONE launch, laid out as the flat batch that
// Engine::share_proofs_verify takes (cda_share_proof_batch), and the
// single-range call (cda_square_share_proof) as the same plan, table and
// kernel with n = 1 and its own layout of the nodes.
//
// Proof shape.  A range covers one segment per row (share_proofs_plan.h).  The
// row trees are perfect trees of W = 2k leaves, so the nodes of nmt
// ProveRange(s0, e0) have the closed form of tree_index.h (range_proof_count /
// range_proof_node): the kernel derives every source address from the segment
// table, that closed form and level_offset.  The merkle proof of the row root
// among rowRoots || colRoots is the one of sample.hip with Index = row
// (store_root_proof, resident_proof_dev.h).
//
// Mapping.  Two kinds of workgroup in the one launch, four wavefronts each.
//   Proof workgroups: one wavefront per segment.  The nodes and the row root
//   are read as six 16-byte loads per 96-byte slot into LDS in proof order
//   (stage_slots) and written packed (store_packed); the leaf hash and the
//   aunts leave as big-endian words, one word per lane.  The wave of a proof's first segment
//   also writes the proof's namespace.
//   Share workgroups: one wavefront per unit of at most kUnitShares shares of
//   one segment (8 KiB), found by a binary search of the table's unit prefix
//   sums, copied with 16-byte loads and stores.  A whole-square proof (128
//   segments of 64 KiB at k = 128) and 4 096 one-share proofs both spread over
//   the device this way.  The lanes that hold a share's first 32 bytes compare
//   its namespace with the proof's first share; a unit that sees another
//   namespace clears the proof's one_namespace byte with an atomic AND on the
//   aligned word around it.  Those bytes are uploaded as 1 behind the table, so
//   the call needs no launch or fill of its own for them.
// Every index the kernel uses was validated on the host
// (share_proofs_plan.h).
//
// The kernel is driven by a segment table (segment_table.h), and the half that
// uploads a table, launches and copies back is Engine::emit_segments, which the
// namespace proofs end in too (namespace_proofs.hip).  Their absence segments
// (kSegAbsence) have no share units, and their leaf is one more staged slot
// behind the row root, written packed to absence_leaf.
//
// Blob commitment proofs (cda_square_commitment_proofs) are a third producer,
// here: segments of kind kSegSubtree have no shares, and beside the nodes and
// the row proof their wave gathers the subtree roots of the segment's range --
// node `index` of row level `level` for every item of the cover of
// commitment_proofs_plan.h -- through the same stage row in tiles of
// kProofSlots slots, written packed to subtree_roots; with root_dig each root
// also leaves as its RFC-6962 leaf digest for the commitments' one launch
// (commit.hip).  That half is the SUB instantiation of the kernel, so the
// share and namespace proofs run the code they ran without it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "commitment_proofs_plan.h"
#include "engine.h"
#include "out_regions.h"
#include "resident_proof_dev.h"
#include "segment_table.h"
#include "sha256_dev.h"
#include "share_proofs_plan.h"
#include "tree_index.h"

namespace cda {

namespace {

static_assert(kSegMaxSquares == CDA_SET_MAX_SQUARES, "a segment's row word names every square a set can hold");

constexpr uint32_t kProofWaves = 4;       // segments, or share units, per workgroup
constexpr uint32_t kProofSlots = 2 * kProofMaxD + 2;   // proof nodes, the row root, the namespace or absence leaf
// The single-range call returns outputs of up to this many bytes in one copy (regions_out): measured against one
// copy per output, it is faster up to 1 MiB of shares and slower from 2 MiB (profiles/resident_proof_refactor.txt).
constexpr size_t kOneCopyBytes = 3 << 19;

struct ShareProofsArgs {
    ResidentView sq;
    const SegEntry* segs;
    uint32_t n_segs, n_units, proof_blocks;
    uint8_t* nodes;             // any output may be NULL
    uint8_t* row_roots;
    uint8_t* leaf_hash;
    uint8_t* aunts;
    uint8_t* shares;
    uint8_t* namespaces;
    uint32_t* flags;            // one_namespace bytes, preset to 1
    uint8_t* absence_leaf;      // the namespace proofs' output (namespaces and flags are then NULL)
    uint8_t* subtree_roots;     // the commitment proofs' outputs (SUB)
    uint32_t* root_dig;         // 8 state words per subtree root: sha256(0x00 || root)
};

__device__ __forceinline__ SegEntry load_seg(const SegEntry* p) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    return SegEntry{lo.x, lo.y, lo.z, lo.w, (uint64_t)hi.x | ((uint64_t)hi.y << 32), hi.z, hi.w};
}

// The square a segment is served from: a.sq itself, or (kSet) the member of the set that the segment's row
// word names, a.sq then holding the arenas' bases (square_set.hip) -- with the segment's row.
template <bool kSet>
__device__ __forceinline__ ResidentView seg_view(const ShareProofsArgs& a, const SetStrides& sq, const SegEntry& e,
                                                 uint32_t* row) {
    if constexpr (kSet) {
        *row = seg_row(e.row);
        return member_view(a.sq, sq, seg_square(e.row));
    } else {
        *row = e.row;
        return a.sq;
    }
}

// One wavefront per segment; every wave of the workgroup reaches every barrier.
template <bool SUB, bool kSet>
__device__ __forceinline__ void proof_part(const ShareProofsArgs& a, const SetStrides& sq,
                                           uint4 (*stage)[stage_row(kProofSlots)], uint32_t* tiles) {
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t g = blockIdx.x * kProofWaves + wave;
    const bool live = g < a.n_segs;   // uniform over the wave
    const uint32_t W = 2 * a.sq.k, D = a.sq.log_w, A = D + 1;   // one width for every member of a set
    SegEntry e{};
    if (live) e = load_seg(a.segs + g);
    uint32_t row;
    const ResidentView v = seg_view<kSet>(a, sq, e, &row);
    const uint32_t s0 = e.range & 0xFFFFu, e0 = live ? (e.range >> 16) & kSegEndMask : 1u;
    const uint32_t cnt = live ? range_proof_count(D, s0, e0) : 0u;
    const bool first = live && e.first_cell == row * W + s0;   // the proof's first segment
    const bool absent = (e.range & kSegAbsence) != 0;          // an absence segment: its leaf follows the row root
    uint4* st = stage[wave];
    if (live) {
        // the nodes in proof order, then the row root, then the leaf of an absence segment
        stage_slots(st, cnt + 1 + (absent ? 1u : 0u), lane, [&](uint32_t j) {
            if (j == cnt) return StagedSlot{v.root_slots + (uint64_t)row * kSlot, j};
            if (j == cnt + 1) return StagedSlot{v.levels + ((uint64_t)row * W + s0) * kSlot, j};
            const TreeNode nd = range_proof_node(D, s0, e0, j);
            return StagedSlot{v.levels + level_offset(W, nd.level, 0, kSlot) +
                                  ((uint64_t)row * (W >> nd.level) + nd.index) * kSlot, j};
        });
        // the namespace of the proof's first share
        if (first && lane < 2)
            st[stage_row(cnt + 1) + lane] = reinterpret_cast<const uint4*>(v.eds + (uint64_t)e.first_cell * kShare)[lane];
        // absence_leaf of any other segment is zero
        if (a.absence_leaf && !absent && lane < kSlotPieces) st[stage_row(cnt + 1) + lane] = make_uint4(0, 0, 0, 0);
        store_root_proof(v.rfc, W, A, row, g, a.leaf_hash, a.aunts, lane);   // Index = row among the 4k roots
    }
    __syncthreads();
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(st);
    if (live) {
        if (a.nodes) store_packed<kNode>(sb, cnt, a.nodes + (uint64_t)e.node_off * kNode, lane);
        if (a.row_roots) store_packed<kNode>(sb + cnt * kSlot, 1, a.row_roots + (uint64_t)g * kNode, lane);
        if (a.namespaces && first)
            store_packed<kNs>(sb + (cnt + 1) * kSlot, 1, a.namespaces + (uint64_t)e.proof * kNs, lane);
        if (a.absence_leaf) store_packed<kNode>(sb + (cnt + 1) * kSlot, 1, a.absence_leaf + (uint64_t)g * kNode, lane);
    }
    if constexpr (SUB) {
        // The subtree roots of [s0, e0), kProofSlots at a time through the stage row.  The workgroup's waves
        // run the most tiles any of them needs, so that the barriers are uniform over the workgroup.
        const bool sub = live && (e.range & kSegSubtree) != 0;
        const uint32_t log_w = e.unit_off;
        const uint32_t n_roots = sub ? subtree_cover_walk(s0, e0, log_w, 0xFFFFFFFFu).index : 0u;
        if (lane == 0) tiles[wave] = (n_roots + kProofSlots - 1) / kProofSlots;
        __syncthreads();   // also: the stores above have read the stage row
        uint32_t n_tiles = 0;
        for (uint32_t w = 0; w < kProofWaves; w++) n_tiles = max(n_tiles, tiles[w]);
        for (uint32_t t = 0; t < n_tiles; t++) {
            const uint32_t at = t * kProofSlots;
            const uint32_t here = at < n_roots ? min(kProofSlots, n_roots - at) : 0u;   // uniform over the wave
            if (here)
                stage_slots(st, here, lane, [&](uint32_t j) {
                    const TreeNode nd = subtree_cover_walk(s0, e0, log_w, at + j);
                    return StagedSlot{v.levels + level_offset(W, nd.level, 0, kSlot) +
                                          ((uint64_t)row * (W >> nd.level) + nd.index) * kSlot, j};
                });
            __syncthreads();
            if (here) {
                const uint64_t first_root = e.share_off + at;
                if (a.subtree_roots) store_packed<kNode>(sb, here, a.subtree_roots + first_root * kNode, lane);
                if (a.root_dig && lane < here) {
                    uint32_t I[kSlotWords], d[8];
                    load_slot_be(sb + lane * kSlot, I);
                    rfc_leaf_u<false>(I, d, false);
                    uint4* o = reinterpret_cast<uint4*>(a.root_dig + (first_root + lane) * 8);
                    o[0] = make_uint4(d[0], d[1], d[2], d[3]);
                    o[1] = make_uint4(d[4], d[5], d[6], d[7]);
                }
            }
            __syncthreads();   // the row is read before the next tile overwrites it
        }
    }
}

// One wavefront per unit of at most kUnitShares shares of one segment.
template <bool kSet>
__device__ __forceinline__ void share_part(const ShareProofsArgs& a, const SetStrides& sq) {
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t u = (blockIdx.x - a.proof_blocks) * kProofWaves + wave;
    if (u >= a.n_units) return;   // uniform over the wave; this part has no barrier
    // the last segment whose first unit is not beyond u
    uint32_t lo = 0, hi = a.n_segs - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (a.segs[mid].unit_off <= u) lo = mid;
        else hi = mid - 1;
    }
    const SegEntry e = load_seg(a.segs + lo);
    uint32_t row;
    const ResidentView v = seg_view<kSet>(a, sq, e, &row);
    const uint32_t W = 2 * v.k, s0 = e.range & 0xFFFFu, e0 = (e.range >> 16) & kSegEndMask;
    const uint32_t at = (u - e.unit_off) * kUnitShares;   // first share of the unit within the segment
    const uint32_t cnt = min(kUnitShares, e0 - s0 - at);
    const uint4* src = reinterpret_cast<const uint4*>(v.eds + ((uint64_t)row * W + s0 + at) * kShare);
    uint4* dst = a.shares ? reinterpret_cast<uint4*>(a.shares + (e.share_off + at) * kShare) : nullptr;
    constexpr uint32_t V = kShare / 16;   // 16-byte pieces per share
    const uint32_t part = lane % V;
    // the proof's first namespace: bytes 0..28 are pieces 0 and 1 without the last three bytes
    const bool ns_lane = a.flags && part < 2;
    uint4 ref = make_uint4(0, 0, 0, 0);
    if (ns_lane) ref = reinterpret_cast<const uint4*>(v.eds + (uint64_t)e.first_cell * kShare)[part];
    const uint32_t last_mask = part == 1 ? 0x000000FFu : 0xFFFFFFFFu;
    bool differs = false;
    constexpr uint32_t kIters = kUnitShares * V / 64;   // pieces per lane: all loads in flight, then the stores
    const bool wanted = dst || ns_lane;
    uint4 x[kIters];
#pragma unroll
    for (uint32_t it = 0; it < kIters; it++) {
        const uint32_t q = it * 64 + lane;   // piece q of the unit: share q / V
        x[it] = make_uint4(0, 0, 0, 0);
        if (q < cnt * V && wanted) x[it] = src[q];
    }
#pragma unroll
    for (uint32_t it = 0; it < kIters; it++) {
        const uint32_t q = it * 64 + lane;
        if (q < cnt * V && wanted) {
            if (dst) dst[q] = x[it];
            if (ns_lane)
                differs |= x[it].x != ref.x || x[it].y != ref.y || x[it].z != ref.z ||
                           ((x[it].w ^ ref.w) & last_mask) != 0;
        }
    }
    if (a.flags && __ballot(differs) != 0 && lane == 0)
        atomicAnd(a.flags + e.proof / 4, ~(0xFFu << (8 * (e.proof % 4))));
}

// kSet: the table's segments name their squares (segment_table.h seg_row_word), a.sq holds the bases of a
// set's arenas and sq their per-square strides; else every segment is of the square a.sq and sq is unused.
template <bool SUB, bool kSet>
__global__ __launch_bounds__(64 * kProofWaves) void share_proofs_kernel(const ShareProofsArgs a, const SetStrides sq) {
    __shared__ uint4 stage[kProofWaves][stage_row(kProofSlots)];
    __shared__ uint32_t tiles[kProofWaves];
    if (blockIdx.x < a.proof_blocks) proof_part<SUB, kSet>(a, sq, stage, tiles);   // uniform over the workgroup
    else share_part<kSet>(a, sq);
}

}  // namespace

// One range per call (cda_square_share_proof): the batch with n = 1, the nodes of row i in their documented
// place, slot i * M of nmt_nodes.  A proof of a few shares is a few KiB over five buffers, where every pageable
// copy costs more than its bytes: small outputs come back in one copy (kOneCopyBytes).
int Engine::square_share_proof(ResidentSquare* sq, uint32_t start, uint32_t end, const cda_share_proofs_out& o,
                               uint32_t* nmt_count) {
    if (start >= end || end > sq->k * sq->k) return fail(CDA_ERR_INVALID, "share range out of the original square");
    return square_share_proofs(sq, &start, &end, 1, o, nmt_count, kOneCopyBytes);
}

// nmt_count == NULL: the nodes packed, node_off beside them.  Else segment g's nodes start at slot g * M,
// M = 2 log2 W, and nmt_count[g] of them are valid.  one_copy_max: outputs up to this size return in one copy.
int Engine::square_share_proofs(ResidentSquare* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                                const cda_share_proofs_out& o, uint32_t* nmt_count, size_t one_copy_max) {
    return range_share_proofs(sq, nullptr, nullptr, starts, ends, n, o, nmt_count, one_copy_max);
}

// cda_square_set_share_proofs: range i of member squares[i].  The sizes of a range do not depend on the
// square, so plan, table and outputs are the single square's; every segment names its square beside its row.
int Engine::square_set_share_proofs(ResidentSquareSet* set, const uint32_t* squares, const uint32_t* starts,
                                    const uint32_t* ends, uint32_t n, const cda_share_proofs_out& o) {
    if (n && !squares) return fail(CDA_ERR_INVALID, "null squares");
    if (n && (!starts || !ends)) return fail(CDA_ERR_INVALID, "null buffer");   // the single square's text
    for (uint32_t i = 0; i < n; i++)
        if (squares[i] >= set->n)
            return fail(CDA_ERR_INVALID, "range " + std::to_string(i) + ": square " + std::to_string(squares[i]) +
                                             " is not below the set's " + std::to_string(set->n) + " squares");
    return range_share_proofs(nullptr, set, squares, starts, ends, n, o, nullptr, 0);
}

// The ranges of one square (sq), or of the members squares[i] of a set.
int Engine::range_share_proofs(ResidentSquare* sq, ResidentSquareSet* set, const uint32_t* squares,
                               const uint32_t* starts, const uint32_t* ends, uint32_t n,
                               const cda_share_proofs_out& o, uint32_t* nmt_count, size_t one_copy_max) {
    const uint32_t k = sq ? sq->k : set->k, W = 2 * k, D = sq ? sq->log_w : set->log_w, A = D + 1, M = 2 * D;
    ShareProofsPlan plan;
    const std::string bad = share_proofs_plan(k, starts, ends, n, &plan);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    if (o.seg_off) o.seg_off[0] = 0;
    if (o.node_off) o.node_off[0] = 0;
    if (o.aunt_off) o.aunt_off[0] = 0;
    if (n == 0) return CDA_OK;
    const uint32_t S = plan.n_segments;
    const uint64_t n_units_max = plan.n_shares / kUnitShares + S;
    if (n_units_max + S > (uint64_t)INT32_MAX)
        return fail(CDA_ERR_INVALID, "the batch has too many shares for one launch");
    // the table, then the one_namespace bytes (1 until a unit finds another namespace), in one upload
    const size_t flag_words = ((size_t)n + 3) / 4;
    SegmentEmit em;
    em.up.resize((size_t)S * kSegWords + flag_words);
    SegEntry* segs = em.segs();
    std::memset(em.up.data() + (size_t)S * kSegWords, 1, flag_words * 4);
    uint32_t g = 0, node_at = 0, unit_at = 0;
    uint64_t share_at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t first_cell = (starts[i] / k) * W + starts[i] % k, square = squares ? squares[i] : 0u;
        for_each_segment(k, i, starts[i], ends[i], [&](const ShareProofSegment& sg) {
            const uint32_t count = range_proof_count(D, sg.s0, sg.e0);
            segs[g] = SegEntry{seg_row_word(sg.row, square), sg.s0 | (sg.e0 << 16), nmt_count ? g * M : node_at,
                               unit_at, share_at, i, first_cell};
            if (nmt_count) nmt_count[g] = count;
            if (o.nmt_start) o.nmt_start[g] = (int32_t)sg.s0;
            if (o.nmt_end) o.nmt_end[g] = (int32_t)sg.e0;
            if (o.rfc_total) o.rfc_total[g] = 2ll * W;
            if (o.rfc_index) o.rfc_index[g] = sg.row;
            node_at += count;
            unit_at += seg_units(sg.e0 - sg.s0);
            share_at += sg.e0 - sg.s0;
            g++;
            if (o.node_off) o.node_off[g] = node_at;
            if (o.aunt_off) o.aunt_off[g] = g * A;
        });
        if (o.seg_off) o.seg_off[i + 1] = g;
        if (o.start_row) o.start_row[i] = starts[i] / k;
        if (o.end_row) o.end_row[i] = (ends[i] - 1) / k;
    }
    em.n_segs = S;
    em.n_units = unit_at;
    em.n_flags = n;
    em.node_slots = nmt_count ? (size_t)S * M : plan.n_nodes;
    em.n_aunts = plan.n_aunts;
    em.n_shares = plan.n_shares;
    em.nodes = o.nodes;
    em.row_roots = o.row_roots;
    em.leaf_hash = o.rfc_leaf_hash;
    em.aunts = o.aunts;
    em.shares = o.shares;
    em.namespaces = o.namespaces;
    em.one_namespace = o.one_namespace;
    em.one_copy_max = one_copy_max;
    return emit_segments(sq, set, em);
}

// cda_square_commitment_proofs: a blob is the share range [start, start + share_len) after NextShareIndex, and
// its segments are the share proof's of that range with the subtree roots in the place of the shares.
int Engine::square_commitment_proofs(ResidentSquare* sq, const uint32_t* starts, const uint32_t* share_lens,
                                     uint32_t n, uint32_t threshold, const cda_commitment_proofs_out& o) {
    const uint32_t k = sq->k, W = 2 * k, D = sq->log_w, A = D + 1;
    CommitmentProofsPlan plan;
    const std::string bad = commitment_proofs_plan(k, starts, share_lens, n, threshold, &plan);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    if (sq->push_err != push_order::kOrdered)
        return fail_unordered_square(sq, "nmt builds no tree of it, so no commitment proof");
    if (o.seg_off) o.seg_off[0] = 0;
    if (o.node_off) o.node_off[0] = 0;
    if (o.root_off) o.root_off[0] = 0;
    if (o.aunt_off) o.aunt_off[0] = 0;
    if (n == 0) return CDA_OK;
    const uint32_t S = plan.n_segments;
    // the table, the (unused) one_namespace bytes, the first root of every proof for the commitments
    const size_t flag_words = ((size_t)n + 3) / 4;
    SegmentEmit em;
    em.up.resize((size_t)S * kSegWords + flag_words + n + 1);
    SegEntry* segs = em.segs();
    uint32_t* first_root = em.up.data() + (size_t)S * kSegWords + flag_words;
    uint32_t g = 0, node_at = 0, root_at = 0;
    for (uint32_t i = 0; i < n; i++) {
        NormalisedBlob b{};
        (void)normalise_blob(k, i, starts[i], share_lens[i], threshold, &b);   // checked by the plan
        const uint32_t first_cell = (b.start / k) * W + b.start % k, log_w = ceil_log2(b.w);
        first_root[i] = root_at;
        for_each_segment(k, i, b.start, b.end, [&](const ShareProofSegment& sg) {
            const uint32_t count = range_proof_count(D, sg.s0, sg.e0);
            segs[g] = SegEntry{sg.row, sg.s0 | (sg.e0 << 16) | kSegSubtree, node_at, log_w, root_at, i, first_cell};
            if (o.nmt_start) o.nmt_start[g] = (int32_t)sg.s0;
            if (o.nmt_end) o.nmt_end[g] = (int32_t)sg.e0;
            if (o.rfc_total) o.rfc_total[g] = 2ll * W;
            if (o.rfc_index) o.rfc_index[g] = sg.row;
            node_at += count;
            root_at += subtree_cover_count(sg.s0, sg.e0, b.w);
            g++;
            if (o.node_off) o.node_off[g] = node_at;
            if (o.root_off) o.root_off[g] = root_at;
            if (o.aunt_off) o.aunt_off[g] = g * A;
        });
        em.max_roots = std::max(em.max_roots, root_at - first_root[i]);
        if (o.seg_off) o.seg_off[i + 1] = g;
        if (o.start_row) o.start_row[i] = b.start / k;
        if (o.end_row) o.end_row[i] = (b.end - 1) / k;
        if (o.norm_start) o.norm_start[i] = b.start;
    }
    first_root[n] = root_at;
    if (o.commitments && em.max_roots > kMerkleRootsMaxItems)
        return fail(CDA_ERR_INVALID, "a blob has " + std::to_string(em.max_roots) + " subtree roots; commitments takes at most " +
                                         std::to_string(kMerkleRootsMaxItems) + " per blob");
    em.n_segs = S;
    em.n_flags = n;
    em.node_slots = plan.n_nodes;
    em.n_aunts = plan.n_aunts;
    em.n_roots = plan.n_roots;
    em.nodes = o.nodes;
    em.row_roots = o.row_roots;
    em.leaf_hash = o.rfc_leaf_hash;
    em.aunts = o.aunts;
    em.namespaces = o.namespaces;
    em.subtree_roots = o.subtree_roots;
    em.commitments = o.commitments;
    em.stage = kStageCommitmentProofs;
    return emit_segments(sq, nullptr, em);
}

// The table-to-launch half of both producers (share ranges above, namespaces in namespace_proofs.hip): one
// upload, one launch whatever the table holds, the requested outputs back.  A square, or a set (sq == NULL):
// the table's segments then name their squares, the kernel is the set instantiation over the arenas' bases
// and the scratch is the set's own.
int Engine::emit_segments(ResidentSquare* sq, ResidentSquareSet* set, const SegmentEmit& em) {
    const uint32_t S = em.n_segs;
    DevBuf& scratch = sq ? sq->scratch : set->scratch;
    // SUB has no set instantiation: refuse such a table before anything is enqueued
    if (!sq && (em.subtree_roots || em.commitments))
        return fail(CDA_ERR_INVALID, "subtree segments are not served across a set");
    const ResidentView view = sq ? sq->view()
                                 : ResidentView{set->eds.as<uint8_t>(), set->levels.as<uint8_t>(),
                                                set->col_levels.as<uint8_t>(), set->roots_slots.as<uint8_t>(),
                                                set->rfc.as<uint32_t>(), set->k, set->log_w};
    const SetStrides st = sq ? SetStrides{}
                             : SetStrides{set->eds_sq, set->levels_sq, set->col_levels_sq, set->roots_slots_sq,
                                          set->rfc_sq};
    // scratch: the upload, then one region per requested output; the flags lie inside the upload
    OutRegions out(em.up.size() * 4);
    const auto r_nd = out.add(em.nodes, em.node_slots * kNode), r_rt = out.add(em.row_roots, (size_t)S * kNode),
               r_lh = out.add(em.leaf_hash, (size_t)S * 32), r_au = out.add(em.aunts, em.n_aunts * 32),
               r_sh = out.add(em.shares, (size_t)em.n_shares * kShare),
               r_ns = out.add(em.namespaces, (size_t)em.n_flags * kNs),
               r_al = out.add(em.absence_leaf, (size_t)S * kNode),
               r_fl = out.add_at(em.one_namespace, (size_t)S * sizeof(SegEntry), em.n_flags),
               r_sr = out.add(em.subtree_roots, em.n_roots * kNode),
               r_cm = out.add(em.commitments, (size_t)em.n_flags * 32);
    // scratch behind the outputs: the subtree roots' leaf digests
    const size_t dig_off = out.total(), dig_bytes = em.commitments ? em.n_roots * 32 : 0;
    hipStream_t s = stream_;
    CDA_TRY(ensure(scratch, out.total() + dig_bytes, "hipMalloc"));
    uint8_t* scr = scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, em.up.data(), em.up.size() * 4, s, "H2D share proofs"));
    ShareProofsArgs a{view, reinterpret_cast<const SegEntry*>(scr), S, 0, 0, r_nd.dev(scr), r_rt.dev(scr),
                      r_lh.dev(scr), r_au.dev(scr), r_sh.dev(scr), r_ns.dev(scr),
                      reinterpret_cast<uint32_t*>(r_fl.dev(scr)), r_al.dev(scr), r_sr.dev(scr),
                      em.commitments ? reinterpret_cast<uint32_t*>(scr + dig_off) : nullptr};
    const bool sub = a.subtree_roots || a.root_dig;
    const bool proof_half = a.nodes || a.row_roots || a.leaf_hash || a.aunts || a.namespaces || a.absence_leaf || sub;
    a.proof_blocks = proof_half ? (S + kProofWaves - 1) / kProofWaves : 0;
    a.n_units = a.shares || a.flags ? em.n_units : 0;
    const uint32_t blocks = a.proof_blocks + (a.n_units + kProofWaves - 1) / kProofWaves;
    if (blocks) {
        if (em.stage >= 0) mark_begin(em.stage, s);
        const dim3 grid(blocks), wg(64 * kProofWaves);
        if (!sq) hipLaunchKernelGGL((share_proofs_kernel<false, true>), grid, wg, 0, s, a, st);
        else if (sub) hipLaunchKernelGGL((share_proofs_kernel<true, false>), grid, wg, 0, s, a, st);
        else hipLaunchKernelGGL((share_proofs_kernel<false, false>), grid, wg, 0, s, a, st);
        if (em.stage >= 0) mark_end(s);
        CDA_TRY(launched("share proofs"));
    }
    if (em.commitments) {
        // the first roots of the proofs lie behind the table and the flag words of the upload
        const uint32_t* bt = reinterpret_cast<const uint32_t*>(scr) + (size_t)S * kSegWords + ((size_t)em.n_flags + 3) / 4;
        if (em.stage >= 0) mark_begin(em.stage, s);
        const hipError_t err = launch_digest_merkle_roots(a.root_dig, bt, em.n_flags, em.max_roots, r_cm.dev(scr), s);
        if (em.stage >= 0) mark_end(s);
        CDA_TRY(check(err, "commitments of the subtree roots"));
    }
    // the table is pageable and the outputs are the caller's: complete before returning
    return regions_out(out, scr, out.span().bytes <= em.one_copy_max, s, "D2H share proofs");
}

}  // namespace cda
