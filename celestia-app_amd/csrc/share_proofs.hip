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
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "out_regions.h"
#include "resident_proof_dev.h"
#include "segment_table.h"
#include "sha256_dev.h"
#include "share_proofs_plan.h"
#include "tree_index.h"

namespace cda {

namespace {

constexpr uint32_t kProofWaves = 4;        // segments, or share units, per workgroup
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
};

__device__ __forceinline__ SegEntry load_seg(const SegEntry* p) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    return SegEntry{lo.x, lo.y, lo.z, lo.w, (uint64_t)hi.x | ((uint64_t)hi.y << 32), hi.z, hi.w};
}

// One wavefront per segment; every wave of the workgroup reaches the barrier.
__device__ __forceinline__ void proof_part(const ShareProofsArgs& a, uint4 (*stage)[stage_row(kProofSlots)]) {
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t g = blockIdx.x * kProofWaves + wave;
    const bool live = g < a.n_segs;   // uniform over the wave
    const ResidentView& v = a.sq;
    const uint32_t W = 2 * v.k, D = v.log_w, A = D + 1;
    SegEntry e{};
    if (live) e = load_seg(a.segs + g);
    const uint32_t row = e.row, s0 = e.range & 0xFFFFu, e0 = live ? (e.range >> 16) & kSegEndMask : 1u;
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
    if (!live) return;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(st);
    if (a.nodes) store_packed<kNode>(sb, cnt, a.nodes + (uint64_t)e.node_off * kNode, lane);
    if (a.row_roots) store_packed<kNode>(sb + cnt * kSlot, 1, a.row_roots + (uint64_t)g * kNode, lane);
    if (a.namespaces && first) store_packed<kNs>(sb + (cnt + 1) * kSlot, 1, a.namespaces + (uint64_t)e.proof * kNs, lane);
    if (a.absence_leaf) store_packed<kNode>(sb + (cnt + 1) * kSlot, 1, a.absence_leaf + (uint64_t)g * kNode, lane);
}

// One wavefront per unit of at most kUnitShares shares of one segment.
__device__ __forceinline__ void share_part(const ShareProofsArgs& a) {
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
    const uint32_t W = 2 * a.sq.k, s0 = e.range & 0xFFFFu, e0 = (e.range >> 16) & kSegEndMask;
    const uint32_t at = (u - e.unit_off) * kUnitShares;   // first share of the unit within the segment
    const uint32_t cnt = min(kUnitShares, e0 - s0 - at);
    const uint4* src = reinterpret_cast<const uint4*>(a.sq.eds + ((uint64_t)e.row * W + s0 + at) * kShare);
    uint4* dst = a.shares ? reinterpret_cast<uint4*>(a.shares + (e.share_off + at) * kShare) : nullptr;
    constexpr uint32_t V = kShare / 16;   // 16-byte pieces per share
    const uint32_t part = lane % V;
    // the proof's first namespace: bytes 0..28 are pieces 0 and 1 without the last three bytes
    const bool ns_lane = a.flags && part < 2;
    uint4 ref = make_uint4(0, 0, 0, 0);
    if (ns_lane) ref = reinterpret_cast<const uint4*>(a.sq.eds + (uint64_t)e.first_cell * kShare)[part];
    const uint32_t last_mask = part == 1 ? 0x000000FFu : 0xFFFFFFFFu;
    bool differs = false;
    constexpr uint32_t kIters = kUnitShares * V / 64;   // pieces per lane: all loads in flight, then the stores
    const bool wanted = dst || ns_lane;
    uint4 v[kIters];
#pragma unroll
    for (uint32_t it = 0; it < kIters; it++) {
        const uint32_t q = it * 64 + lane;   // piece q of the unit: share q / V
        v[it] = make_uint4(0, 0, 0, 0);
        if (q < cnt * V && wanted) v[it] = src[q];
    }
#pragma unroll
    for (uint32_t it = 0; it < kIters; it++) {
        const uint32_t q = it * 64 + lane;
        if (q < cnt * V && wanted) {
            if (dst) dst[q] = v[it];
            if (ns_lane)
                differs |= v[it].x != ref.x || v[it].y != ref.y || v[it].z != ref.z ||
                           ((v[it].w ^ ref.w) & last_mask) != 0;
        }
    }
    if (a.flags && __ballot(differs) != 0 && lane == 0)
        atomicAnd(a.flags + e.proof / 4, ~(0xFFu << (8 * (e.proof % 4))));
}

__global__ __launch_bounds__(64 * kProofWaves) void share_proofs_kernel(const ShareProofsArgs a) {
    __shared__ uint4 stage[kProofWaves][stage_row(kProofSlots)];
    if (blockIdx.x < a.proof_blocks) proof_part(a, stage);   // uniform over the workgroup
    else share_part(a);
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
    const uint32_t k = sq->k, W = 2 * k, D = sq->log_w, A = D + 1, M = 2 * D;
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
        const uint32_t first_cell = (starts[i] / k) * W + starts[i] % k;
        for_each_segment(k, i, starts[i], ends[i], [&](const ShareProofSegment& sg) {
            const uint32_t count = range_proof_count(D, sg.s0, sg.e0);
            segs[g] = SegEntry{sg.row, sg.s0 | (sg.e0 << 16), nmt_count ? g * M : node_at, unit_at, share_at, i,
                               first_cell};
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
    return emit_segments(sq, em);
}

// The table-to-launch half of both producers (share ranges above, namespaces in namespace_proofs.hip): one
// upload, one launch whatever the table holds, the requested outputs back.
int Engine::emit_segments(ResidentSquare* sq, const SegmentEmit& em) {
    const uint32_t S = em.n_segs;
    // scratch: the upload, then one region per requested output; the flags lie inside the upload
    OutRegions out(em.up.size() * 4);
    const auto r_nd = out.add(em.nodes, em.node_slots * kNode), r_rt = out.add(em.row_roots, (size_t)S * kNode),
               r_lh = out.add(em.leaf_hash, (size_t)S * 32), r_au = out.add(em.aunts, em.n_aunts * 32),
               r_sh = out.add(em.shares, (size_t)em.n_shares * kShare),
               r_ns = out.add(em.namespaces, (size_t)em.n_flags * kNs),
               r_al = out.add(em.absence_leaf, (size_t)S * kNode),
               r_fl = out.add_at(em.one_namespace, (size_t)S * sizeof(SegEntry), em.n_flags);
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->scratch, out.total(), "hipMalloc"));
    uint8_t* scr = sq->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, em.up.data(), em.up.size() * 4, s, "H2D share proofs"));
    ShareProofsArgs a{sq->view(), reinterpret_cast<const SegEntry*>(scr), S, 0, 0, r_nd.dev(scr), r_rt.dev(scr),
                      r_lh.dev(scr), r_au.dev(scr), r_sh.dev(scr), r_ns.dev(scr),
                      reinterpret_cast<uint32_t*>(r_fl.dev(scr)), r_al.dev(scr)};
    const bool proof_half = a.nodes || a.row_roots || a.leaf_hash || a.aunts || a.namespaces || a.absence_leaf;
    a.proof_blocks = proof_half ? (S + kProofWaves - 1) / kProofWaves : 0;
    a.n_units = a.shares || a.flags ? em.n_units : 0;
    const uint32_t blocks = a.proof_blocks + (a.n_units + kProofWaves - 1) / kProofWaves;
    if (blocks) {
        hipLaunchKernelGGL(share_proofs_kernel, dim3(blocks), dim3(64 * kProofWaves), 0, s, a);
        CDA_TRY(launched("share proofs"));
    }
    // the table is pageable and the outputs are the caller's: complete before returning
    return regions_out(out, scr, out.span().bytes <= em.one_copy_max, s, "D2H share proofs");
}

}  // namespace cda
