// share_proofs.hip -- share-inclusion proofs of many ranges of a resident
// square in ONE launch (proof.NewShareInclusionProofFromEDS, pkg/proof/
// proof.go:77-145, for a batch of ranges), laid out as the flat batch that
// Engine::share_proofs_verify takes (cda_share_proof_batch).
//
// Proof shape.  A range covers one segment per row (share_proofs_plan.h).  The
// row trees are perfect trees of W = 2k leaves, so the nodes of nmt
// ProveRange(s0, e0) have the closed form of tree_index.h (range_proof_count /
// range_proof_node): the kernel derives every source address from the segment
// table, that closed form and level_offset.  The merkle proof of the row root
// among rowRoots || colRoots is the one of sample.hip with Index = row.
//
// Mapping.  Two kinds of workgroup in the one launch, four wavefronts each.
//   Proof workgroups: one wavefront per segment.  The nodes and the row root
//   are read as six 16-byte loads per 96-byte slot into LDS in proof order and
//   written packed (store_packed); the leaf hash and the aunts leave as
//   big-endian words, one word per lane.  The wave of a proof's first segment
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
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "packed_store_dev.h"
#include "sha256_dev.h"
#include "share_proofs_plan.h"
#include "tree_index.h"

namespace cda {

namespace {

constexpr uint32_t kProofWaves = 4;        // segments, or share units, per workgroup
constexpr uint32_t kProofMaxD = 11;        // log2(2 * 1024)
constexpr uint32_t kProofSlots = 2 * kProofMaxD + 2;   // proof nodes, the row root, the namespace
constexpr uint32_t kUnitShares = 16;       // shares one wave copies

// One segment, as uploaded: 32 bytes.
struct SegEntry {
    uint32_t row;
    uint32_t range;        // s0 | e0 << 16: the leaf range in the row tree
    uint32_t node_off;     // first node of the segment in `nodes`
    uint32_t unit_off;     // first share unit of the segment
    uint64_t share_off;    // first share of the segment in `shares`
    uint32_t proof;
    uint32_t first_cell;   // EDS cell (row * W + col) of the proof's first share
};
static_assert(sizeof(SegEntry) == 32);

struct ShareProofsArgs {
    const SegEntry* segs;
    uint32_t n_segs, n_units, proof_blocks, k, log_w;
    const uint8_t* eds;         // [W][W][512]
    const uint8_t* levels;      // row levels, level 0 = the leaf slots
    const uint8_t* root_slots;  // [2W][96]: row roots, then column roots
    const uint32_t* rfc;        // RFC-6962 levels of the data-root tree, state words
    uint8_t* nodes;             // any output may be NULL
    uint8_t* row_roots;
    uint8_t* leaf_hash;
    uint8_t* aunts;
    uint8_t* shares;
    uint8_t* namespaces;
    uint32_t* flags;            // one_namespace bytes, preset to 1
};

__device__ __forceinline__ SegEntry load_seg(const SegEntry* p) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    return SegEntry{lo.x, lo.y, lo.z, lo.w, (uint64_t)hi.x | ((uint64_t)hi.y << 32), hi.z, hi.w};
}

// One wavefront per segment; every wave of the workgroup reaches the barrier.
__device__ __forceinline__ void proof_part(const ShareProofsArgs& a, uint4 (*stage)[kProofSlots * (kSlot / 16)]) {
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t g = blockIdx.x * kProofWaves + wave;
    const bool live = g < a.n_segs;   // uniform over the wave
    const uint32_t W = 2 * a.k, D = a.log_w, A = D + 1;
    SegEntry e{};
    if (live) e = load_seg(a.segs + g);
    const uint32_t row = e.row, s0 = e.range & 0xFFFFu, e0 = live ? e.range >> 16 : 1u;
    const uint32_t cnt = live ? range_proof_count(D, s0, e0) : 0u;
    const bool first = live && e.first_cell == row * W + s0;   // the proof's first segment
    uint4* st = stage[wave];
    if (live) {
        // the nodes in proof order, then the row root: six 16-byte loads per slot
        for (uint32_t q = lane; q < (cnt + 1) * (kSlot / 16); q += 64) {
            const uint32_t j = q / (kSlot / 16), part = q % (kSlot / 16);
            const uint8_t* src;
            if (j == cnt) {
                src = a.root_slots + (uint64_t)row * kSlot;
            } else {
                const TreeNode nd = range_proof_node(D, s0, e0, j);
                src = a.levels + level_offset(W, nd.level, 0, kSlot) +
                      ((uint64_t)row * (W >> nd.level) + nd.index) * kSlot;
            }
            st[q] = reinterpret_cast<const uint4*>(src)[part];
        }
        // the namespace of the proof's first share
        if (first && lane < 2)
            st[(cnt + 1) * (kSlot / 16) + lane] = reinterpret_cast<const uint4*>(a.eds + (uint64_t)e.first_cell * kShare)[lane];
        // leaf hash and aunts: state words out as big-endian bytes, one word per lane
        const uint32_t idx = row, T = 2 * W;   // Index among the Total = 4k roots
        for (uint32_t q = lane; q < (A + 1) * 8; q += 64) {
            const uint32_t item = q / 8, word = q % 8;
            if (item == 0) {
                if (a.leaf_hash)
                    reinterpret_cast<uint32_t*>(a.leaf_hash + (uint64_t)g * 32)[word] = bswap32(a.rfc[(uint64_t)idx * 8 + word]);
            } else if (a.aunts) {
                const uint32_t l = item - 1;
                const uint64_t entry = (uint64_t)(2 * T - ((2 * T) >> l)) + ((idx >> l) ^ 1u);
                reinterpret_cast<uint32_t*>(a.aunts + ((uint64_t)g * A + l) * 32)[word] = bswap32(a.rfc[entry * 8 + word]);
            }
        }
    }
    __syncthreads();
    if (!live) return;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(st);
    if (a.nodes) store_packed<kNode>(sb, cnt, a.nodes + (uint64_t)e.node_off * kNode, lane);
    if (a.row_roots) store_packed<kNode>(sb + cnt * kSlot, 1, a.row_roots + (uint64_t)g * kNode, lane);
    if (a.namespaces && first) store_packed<kNs>(sb + (cnt + 1) * kSlot, 1, a.namespaces + (uint64_t)e.proof * kNs, lane);
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
    const uint32_t W = 2 * a.k, s0 = e.range & 0xFFFFu, e0 = e.range >> 16;
    const uint32_t at = (u - e.unit_off) * kUnitShares;   // first share of the unit within the segment
    const uint32_t cnt = min(kUnitShares, e0 - s0 - at);
    const uint4* src = reinterpret_cast<const uint4*>(a.eds + ((uint64_t)e.row * W + s0 + at) * kShare);
    uint4* dst = a.shares ? reinterpret_cast<uint4*>(a.shares + (e.share_off + at) * kShare) : nullptr;
    constexpr uint32_t V = kShare / 16;   // 16-byte pieces per share
    const uint32_t part = lane % V;
    // the proof's first namespace: bytes 0..28 are pieces 0 and 1 without the last three bytes
    const bool ns_lane = a.flags && part < 2;
    uint4 ref = make_uint4(0, 0, 0, 0);
    if (ns_lane) ref = reinterpret_cast<const uint4*>(a.eds + (uint64_t)e.first_cell * kShare)[part];
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
    __shared__ uint4 stage[kProofWaves][kProofSlots * (kSlot / 16)];
    if (blockIdx.x < a.proof_blocks) proof_part(a, stage);   // uniform over the workgroup
    else share_part(a);
}

}  // namespace

int Engine::square_share_proofs(ResidentSquare* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                                const cda_share_proofs_out& o) {
    const uint32_t k = sq->k, W = 2 * k, D = sq->log_w, A = D + 1;
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
    std::vector<uint32_t> up((size_t)S * (sizeof(SegEntry) / 4) + flag_words);
    SegEntry* segs = reinterpret_cast<SegEntry*>(up.data());
    std::memset(up.data() + (size_t)S * (sizeof(SegEntry) / 4), 1, flag_words * 4);
    uint32_t g = 0, node_at = 0, unit_at = 0;
    uint64_t share_at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t first_cell = (starts[i] / k) * W + starts[i] % k;
        for_each_segment(k, i, starts[i], ends[i], [&](const ShareProofSegment& sg) {
            segs[g] = SegEntry{sg.row, sg.s0 | (sg.e0 << 16), node_at, unit_at, share_at, i, first_cell};
            if (o.nmt_start) o.nmt_start[g] = (int32_t)sg.s0;
            if (o.nmt_end) o.nmt_end[g] = (int32_t)sg.e0;
            if (o.rfc_total) o.rfc_total[g] = 2ll * W;
            if (o.rfc_index) o.rfc_index[g] = sg.row;
            node_at += range_proof_count(D, sg.s0, sg.e0);
            unit_at += (sg.e0 - sg.s0 + kUnitShares - 1) / kUnitShares;
            share_at += sg.e0 - sg.s0;
            g++;
            if (o.node_off) o.node_off[g] = node_at;
            if (o.aunt_off) o.aunt_off[g] = g * A;
        });
        if (o.seg_off) o.seg_off[i + 1] = g;
        if (o.start_row) o.start_row[i] = starts[i] / k;
        if (o.end_row) o.end_row[i] = (ends[i] - 1) / k;
    }
    // scratch: the upload, then one region per requested output, each at a 16-byte boundary
    struct Region {
        uint8_t* host;
        size_t bytes, off;
    };
    const size_t table_bytes = (size_t)S * sizeof(SegEntry);
    size_t total = (up.size() * 4 + 15) & ~(size_t)15;
    auto region = [&](uint8_t* host, size_t bytes) {
        Region r{host, host ? bytes : 0, total};
        total += (r.bytes + 15) & ~(size_t)15;
        return r;
    };
    const Region r_nd = region(o.nodes, (size_t)plan.n_nodes * kNode), r_rt = region(o.row_roots, (size_t)S * kNode),
                 r_lh = region(o.rfc_leaf_hash, (size_t)S * 32), r_au = region(o.aunts, (size_t)plan.n_aunts * 32),
                 r_sh = region(o.shares, (size_t)plan.n_shares * kShare), r_ns = region(o.namespaces, (size_t)n * kNs);
    const Region r_fl{o.one_namespace, o.one_namespace ? (size_t)n : 0, table_bytes};   // inside the upload
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->scratch, total, "hipMalloc"));
    uint8_t* scr = sq->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, up.data(), up.size() * 4, s, "H2D share proofs"));
    auto dev = [&](const Region& r) -> uint8_t* { return r.host ? scr + r.off : nullptr; };
    ShareProofsArgs a{};
    a.segs = reinterpret_cast<const SegEntry*>(scr);
    a.n_segs = S;
    a.k = k;
    a.log_w = D;
    a.eds = sq->eds.as<uint8_t>();
    a.levels = sq->levels.as<uint8_t>();
    a.root_slots = sq->roots_slots.as<uint8_t>();
    a.rfc = sq->rfc.as<uint32_t>();
    a.nodes = dev(r_nd);
    a.row_roots = dev(r_rt);
    a.leaf_hash = dev(r_lh);
    a.aunts = dev(r_au);
    a.shares = dev(r_sh);
    a.namespaces = dev(r_ns);
    a.flags = reinterpret_cast<uint32_t*>(dev(r_fl));
    const bool proof_half = a.nodes || a.row_roots || a.leaf_hash || a.aunts || a.namespaces;
    a.proof_blocks = proof_half ? (S + kProofWaves - 1) / kProofWaves : 0;
    a.n_units = a.shares || a.flags ? unit_at : 0;
    const uint32_t blocks = a.proof_blocks + (a.n_units + kProofWaves - 1) / kProofWaves;
    if (blocks) {
        hipLaunchKernelGGL(share_proofs_kernel, dim3(blocks), dim3(64 * kProofWaves), 0, s, a);
        CDA_TRY(launched("share proofs"));
    }
    for (const Region* r : {&r_nd, &r_rt, &r_lh, &r_au, &r_sh, &r_ns, &r_fl})
        if (r->bytes) CDA_TRY(d2h(r->host, scr + r->off, r->bytes, s, "D2H share proofs"));
    // `up` is pageable and the outputs are the caller's: complete before returning
    return sync(s);
}

}  // namespace cda
