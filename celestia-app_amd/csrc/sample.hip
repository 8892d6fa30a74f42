// sample.hip -- data-availability samples of a resident square: a batch of
// (row, column, axis) cells of the EDS, each with its NMT inclusion proof
// against the row or the column root and the merkle proof of that root against
// the data root, answered by ONE launch from the nodes square_create keeps
// (proof.hip), and the host side of checking such samples (the batch goes
// through Engine::share_proofs_verify, verify.hip).
//
// Proof shape.  The axis trees are perfect trees of W = 2k leaves, so nmt
// ProveRange(p, p + 1) always has D = log2 W nodes, one sibling per level:
// node (p >> L) ^ 1 of level L.  nmt orders them depth first, left to right:
// the left siblings top-down (L from D - 1 down to 0 where bit L of p is set),
// then the right siblings bottom-up (L from 0 up to D - 1 where bit L is
// clear).  The sibling of level L therefore goes to proof position
//     bit L set:    popcount(p >> (L + 1))
//     bit L clear:  popcount(p) + L - popcount(p & ((1 << L) - 1)).
// The merkle proof of the root among rowRoots || colRoots (Total 4k = 2W) has
// A = D + 1 aunts, bottom-up: digest ((idx >> l) ^ 1) of RFC level l.
//
// Mapping.  One wavefront per sample, four samples per workgroup.  A sample is
// 512 + 29 + 90 D + 90 + 32 (A + 1) bytes of output (about 1.7 KiB at k = 128)
// from D + A + 3 scattered places, so the work is latency and store bound, not
// arithmetic: a wave gives every sample 64 independent 16-byte loads in flight
// and keeps all its control flow (axis, level, bit tests) uniform.  The 90-byte
// packed nodes start at any even address; the wave first puts the D + 1 slots
// (16-byte loads, proof order) into LDS and then writes the packed bytes with
// one aligned 4-byte store per lane, consecutive lanes on consecutive words
// (256 B per wave instruction), the at most three bytes at either end of a
// region singly.  Shares and digests are aligned and go out directly.  The
// staging, the merkle proof of the root and the view of the square are the ones
// share_proofs.hip uses (resident_proof_dev.h); the scratch layout and the
// copies back are out_regions.h's.
// Every index the kernel uses was validated on the host
// (Engine::square_sample_proofs).
//
// Sets.  The same kernel with a square index per sample serves a set of
// resident squares (square_set.hip) in one launch: sample_kernel<true> takes
// the arenas' bases and per-square strides and derives each wave's view from
// them (Engine::square_set_sample_proofs).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "out_regions.h"
#include "resident_proof_dev.h"
#include "sha256_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

constexpr uint32_t kSampleWaves = 4;      // samples per workgroup
constexpr uint32_t kSampleSlots = kProofMaxD + 2;   // proof nodes, the axis root, the namespace

struct SampleArgs {
    ResidentView sq;
    const uint32_t* coords;     // n words: row | col << 12 | axis << 24 (a set: n pairs, the square second)
    uint32_t n;
    uint8_t* shares;            // any output may be NULL
    uint8_t* namespaces;
    uint8_t* nodes;
    uint8_t* roots;
    uint8_t* leaf_hash;
    uint8_t* aunts;
};

// One wave's sample i of the square `v` (live: i is a sample of the batch; uniform over the wave, and no early
// return before the barrier the workgroup meets at).  c: row | col << 12 | axis << 24.
__device__ __forceinline__ void sample_wave(const ResidentView& v, const SampleArgs& a, uint32_t i, bool live,
                                            uint32_t c, uint4* st, uint32_t lane) {
    const uint32_t W = 2 * v.k, D = v.log_w, A = D + 1;
    uint32_t row = 0, col = 0, axis = 0;
    if (live) {
        row = c & 0xFFFu;
        col = (c >> 12) & 0xFFFu;
        axis = c >> 24;
    }
    const uint32_t p = axis ? row : col;      // leaf position in the axis tree
    const uint32_t tree = axis ? col : row;   // which tree of the axis
    const uint64_t cell = (uint64_t)row * W + col;
    if (live) {
        // the share: 32 lanes x 16 bytes; its first two words also give the Q0 namespace
        uint4 sh = make_uint4(0, 0, 0, 0);
        if (lane < 32) sh = reinterpret_cast<const uint4*>(v.eds + cell * kShare)[lane];
        if (a.shares && lane < 32) reinterpret_cast<uint4*>(a.shares + (uint64_t)i * kShare)[lane] = sh;
        if (lane < 2) {
            const bool q0 = row < v.k && col < v.k;   // else ParitySharesNamespace: 29 bytes of 0xFF
            st[stage_row(D + 1) + lane] = q0 ? sh : make_uint4(~0u, ~0u, ~0u, ~0u);
        }
        // the D siblings in proof order, then the axis root
        stage_slots(st, D + 1, lane, [&](uint32_t L) {
            if (L == D) return StagedSlot{v.root_slots + (uint64_t)(axis * W + tree) * kSlot, D};
            const uint32_t sib = (p >> L) ^ 1u;
            const uint8_t* src;
            if (L == 0)   // the leaf level: shared by both axes, a column reads it with stride W
                src = v.levels + (axis ? (uint64_t)sib * W + tree : (uint64_t)tree * W + sib) * kSlot;
            else if (axis)
                src = v.col_levels + level_offset(W, L, 1, kSlot) + ((uint64_t)tree * (W >> L) + sib) * kSlot;
            else
                src = v.levels + level_offset(W, L, 0, kSlot) + ((uint64_t)tree * (W >> L) + sib) * kSlot;
            return StagedSlot{src, ((p >> L) & 1u) ? (uint32_t)__popc(p >> (L + 1))
                                                   : (uint32_t)__popc(p) + L - (uint32_t)__popc(p & ((1u << L) - 1u))};
        });
        store_root_proof(v.rfc, W, A, axis * W + tree, i, a.leaf_hash, a.aunts, lane);   // Index among the 4k roots
    }
    __syncthreads();
    if (!live) return;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(st);
    if (a.nodes) store_packed<kNode>(sb, D, a.nodes + (uint64_t)i * D * kNode, lane);
    if (a.roots) store_packed<kNode>(sb + D * kSlot, 1, a.roots + (uint64_t)i * kNode, lane);
    if (a.namespaces) store_packed<kNs>(sb + (D + 1) * kSlot, 1, a.namespaces + (uint64_t)i * kNs, lane);
}

// kSet = false: the samples of the square a.sq.  kSet = true: samples across a set of resident squares --
// a.sq holds the arenas' bases, sample i names its square in word 2i + 1 of the requests (word 2i: the
// coordinates) and the wave reads that square's strides of the arenas.
template <bool kSet>
__global__ __launch_bounds__(64 * kSampleWaves) void sample_kernel(const SampleArgs a, const SetStrides sq) {
    __shared__ uint4 stage[kSampleWaves][stage_row(kSampleSlots)];
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t i = blockIdx.x * kSampleWaves + wave;
    const bool live = i < a.n;   // uniform over the wave
    if constexpr (kSet) {
        const uint2 req = live ? reinterpret_cast<const uint2*>(a.coords)[i] : make_uint2(0u, 0u);
        sample_wave(member_view(a.sq, sq, req.y), a, i, live, req.x, stage[wave], lane);
    } else {
        sample_wave(a.sq, a, i, live, live ? a.coords[i] : 0u, stage[wave], lane);
    }
}

// The first bad coordinate of a batch ("" if none): the text names the sample and the field.
std::string check_coords(const uint32_t* rows, const uint32_t* cols, const uint8_t* axes, uint32_t n, uint32_t W) {
    auto at = [](uint32_t i, const char* field, uint32_t v) {
        return "sample " + std::to_string(i) + ": " + field + " " + std::to_string(v);
    };
    for (uint32_t i = 0; i < n; i++) {
        if (rows[i] >= W) return at(i, "row", rows[i]) + " is not below the EDS width " + std::to_string(W);
        if (cols[i] >= W) return at(i, "col", cols[i]) + " is not below the EDS width " + std::to_string(W);
        if (axes && axes[i] > 1) return at(i, "axis", axes[i]) + " is neither 0 (row) nor 1 (column)";
    }
    return "";
}

}  // namespace

int Engine::square_sample_proofs(ResidentSquare* sq, const uint32_t* rows, const uint32_t* cols, const uint8_t* axes,
                                 uint32_t n, const SampleOut& o) {
    if (n == 0) return CDA_OK;
    if (!rows || !cols) return fail(CDA_ERR_INVALID, "null buffer");
    const uint32_t k = sq->k, W = 2 * k, D = sq->log_w, A = D + 1;
    const std::string bad = check_coords(rows, cols, axes, n, W);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    std::vector<uint32_t> packed(n);
    for (uint32_t i = 0; i < n; i++) packed[i] = rows[i] | (cols[i] << 12) | ((axes ? axes[i] : 0u) << 24);
    // scratch: the packed coordinates, then one struct-of-arrays region per requested output
    OutRegions out((size_t)n * 4);
    const auto r_sh = out.add(o.shares, (size_t)n * kShare), r_ns = out.add(o.namespaces, (size_t)n * kNs),
               r_nd = out.add(o.nmt_nodes, (size_t)n * D * kNode), r_rt = out.add(o.axis_roots, (size_t)n * kNode),
               r_lh = out.add(o.leaf_hash, (size_t)n * 32), r_au = out.add(o.aunts, (size_t)n * A * 32);
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->scratch, out.total(), "hipMalloc"));
    uint8_t* scr = sq->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, packed.data(), (size_t)n * 4, s, "H2D samples"));
    const SampleArgs a{sq->view(), reinterpret_cast<const uint32_t*>(scr), n, r_sh.dev(scr), r_ns.dev(scr),
                       r_nd.dev(scr), r_rt.dev(scr), r_lh.dev(scr), r_au.dev(scr)};
    hipLaunchKernelGGL(sample_kernel<false>, dim3((n + kSampleWaves - 1) / kSampleWaves), dim3(64 * kSampleWaves), 0, s,
                       a, SetStrides{});
    CDA_TRY(launched("sample proofs"));
    // `packed` is pageable and the outputs are the caller's: complete before returning
    return regions_out(out, scr, false, s, "D2H samples");
}

int Engine::square_set_sample_proofs(ResidentSquareSet* set, const uint32_t* squares, const uint32_t* rows,
                                     const uint32_t* cols, const uint8_t* axes, uint32_t n, const SampleOut& o) {
    if (n == 0) return CDA_OK;
    if (!squares || !rows || !cols) return fail(CDA_ERR_INVALID, "null buffer");
    const uint32_t k = set->k, W = 2 * k, D = set->log_w, A = D + 1;
    for (uint32_t i = 0; i < n; i++)
        if (squares[i] >= set->n)
            return fail(CDA_ERR_INVALID, "sample " + std::to_string(i) + ": square " + std::to_string(squares[i]) +
                                             " is not below the set's " + std::to_string(set->n) + " squares");
    const std::string bad = check_coords(rows, cols, axes, n, W);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    std::vector<uint32_t> packed((size_t)2 * n);
    for (uint32_t i = 0; i < n; i++) {
        packed[2 * i] = rows[i] | (cols[i] << 12) | ((axes ? axes[i] : 0u) << 24);
        packed[2 * i + 1] = squares[i];
    }
    // scratch: the packed requests, then one struct-of-arrays region per requested output
    OutRegions out((size_t)n * 8);
    const auto r_sh = out.add(o.shares, (size_t)n * kShare), r_ns = out.add(o.namespaces, (size_t)n * kNs),
               r_nd = out.add(o.nmt_nodes, (size_t)n * D * kNode), r_rt = out.add(o.axis_roots, (size_t)n * kNode),
               r_lh = out.add(o.leaf_hash, (size_t)n * 32), r_au = out.add(o.aunts, (size_t)n * A * 32);
    hipStream_t s = stream_;
    CDA_TRY(ensure(set->scratch, out.total(), "hipMalloc"));
    uint8_t* scr = set->scratch.as<uint8_t>();
    CDA_TRY(h2d(scr, packed.data(), (size_t)n * 8, s, "H2D samples"));
    const ResidentView base{set->eds.as<uint8_t>(), set->levels.as<uint8_t>(), set->col_levels.as<uint8_t>(),
                            set->roots_slots.as<uint8_t>(), set->rfc.as<uint32_t>(), k, D};
    const SampleArgs a{base, reinterpret_cast<const uint32_t*>(scr), n, r_sh.dev(scr), r_ns.dev(scr),
                       r_nd.dev(scr), r_rt.dev(scr), r_lh.dev(scr), r_au.dev(scr)};
    const SetStrides st{set->eds_sq, set->levels_sq, set->col_levels_sq, set->roots_slots_sq, set->rfc_sq};
    hipLaunchKernelGGL(sample_kernel<true>, dim3((n + kSampleWaves - 1) / kSampleWaves), dim3(64 * kSampleWaves), 0, s,
                       a, st);
    CDA_TRY(launched("sample proofs of a set"));
    // `packed` is pageable and the outputs are the caller's: complete before returning
    return regions_out(out, scr, false, s, "D2H samples");
}

int Engine::sample_proofs_verify(uint32_t k, uint32_t n, const uint8_t* data_roots, const uint32_t* rows,
                                 const uint32_t* cols, const uint8_t* axes, const uint8_t* shares,
                                 const uint8_t* nmt_nodes, const uint8_t* axis_roots, const uint8_t* leaf_hash,
                                 const uint8_t* aunts, uint8_t* verdict) {
    if (!is_pow2(k) || k > 1024)
        return fail(CDA_ERR_INVALID, "square width must be a power of two <= 1024");
    if (n == 0) return CDA_OK;
    if (!data_roots || !rows || !cols || !shares || !nmt_nodes || !axis_roots || !leaf_hash || !aunts || !verdict)
        return fail(CDA_ERR_INVALID, "null buffer");
    const uint32_t W = 2 * k, D = ceil_log2(W), A = D + 1;
    const std::string bad = check_coords(rows, cols, axes, n, W);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    // Everything a prover could lie about is derived here from (row, col, axis): the leaf namespace, the
    // leaf position and the merkle Index / Total.  One segment per proof, fixed strides.
    std::vector<uint8_t> ns((size_t)n * kNs);
    std::vector<uint32_t> seg_off(n + 1), node_off(n + 1), aunt_off(n + 1);
    std::vector<int32_t> st(n), en(n);
    std::vector<int64_t> total(n, 2ll * W), index(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t axis = axes ? axes[i] : 0u;
        if (rows[i] < k && cols[i] < k) std::memcpy(&ns[(size_t)i * kNs], shares + (size_t)i * kShare, kNs);
        else std::memset(&ns[(size_t)i * kNs], 0xFF, kNs);
        const uint32_t p = axis ? rows[i] : cols[i];
        st[i] = (int32_t)p;
        en[i] = (int32_t)p + 1;
        index[i] = axis ? (int64_t)W + cols[i] : (int64_t)rows[i];
    }
    for (uint32_t i = 0; i <= n; i++) {
        seg_off[i] = i;
        node_off[i] = i * D;
        aunt_off[i] = i * A;
    }
    cda_share_proof_batch b{};
    b.n_proofs = n;
    b.ns_len = kNs;
    b.share_len = kShare;
    b.data_roots = data_roots;
    b.namespaces = ns.data();
    b.seg_off = seg_off.data();
    b.nmt_start = st.data();
    b.nmt_end = en.data();
    b.node_off = node_off.data();
    b.nodes = nmt_nodes;
    b.n_nodes = n * D;
    b.row_roots = axis_roots;
    b.rfc_total = total.data();
    b.rfc_index = index.data();
    b.rfc_leaf_hash = leaf_hash;
    b.aunt_off = aunt_off.data();
    b.aunts = aunts;
    b.n_aunts = n * A;
    b.shares = shares;
    b.n_shares = n;
    return share_proofs_verify(&b, verdict);
}

}  // namespace cda
