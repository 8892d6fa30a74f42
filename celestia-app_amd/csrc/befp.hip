// befp.hip -- bad-encoding fraud proofs: what a node builds when repair names a
// byzantine row or column, and what a light node checks when it receives one.
//
// Reference: the protocol's own text only -- specs/src/specs/fraud_proofs.md,
// specs/src/specs/networking.md "BadEncodingFraudProof", proto/types.proto:247-259
// -- with rsmt2d v0.14.0 ErrByzantineData (EXT) as the producer's input and
// celestia-node's BadEncodingProof.Validate (EXT) as the order of the checks.
// There is no reference vector; the CPU restatement is tests/befp_ref.py.
//
// Builder.  Vector (axis, index) of an EDS is proven cell by cell against the
// roots of the ORTHOGONAL axis: cell p lies in orthogonal tree p at leaf
// position `index`.  The leaf slots of the whole square and every level of the
// W orthogonal trees are hashed with the square's own kernels (launch_leaves /
// launch_level, no push-order check: the blind roots) into context scratch;
// one more launch, a wave per orthogonal tree, then compares the tree's root
// slot with the DAH root (the flag that tells a complete, committed vector
// from one with holes), stages the D path siblings in nmt's proof order and
// packs the nodes and the share, as sample.hip does from a resident square.
// The host keeps the flagged positions, ascending, after the one copy back.
//
// Verifier.  Step 2 (inclusion of every share) is Engine::share_proofs_verify
// over all shares of the batch, one single-leaf segment each, with the
// namespace, the tree and the leaf position derived here.  The host picks the
// proofs that survive; their shares -- still in the verifier's upload buffer --
// are scattered into an [n'][W][512] grid with its presence mask, the grid's
// rows are Leopard-decoded (repair.hip) and re-encoded (the square's RS
// kernels), hashed as erasured trees with one push-order word each (tree.hip)
// and compared with the DAH roots.  No launch is per proof.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "resident_proof_dev.h"
#include "sha256_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

constexpr uint32_t kBefpWaves = 4;   // trees (builder) / shares (scatter) / proofs (compare) per workgroup

struct BefpBuildArgs {
    const uint8_t* eds;          // [W][W][512]
    const uint8_t* leaves;       // [W][W][96]: level 0, shared by both axes
    const uint8_t* levels;       // levels 1.. of the orthogonal trees: level L = [W trees][W >> L][96]
    const uint8_t* root_slots;   // [W][96]: the orthogonal trees' roots
    const uint8_t* dah;          // [W][90]: the DAH's roots of the orthogonal axis
    uint32_t W, D, axis, index;
    uint8_t* flags;              // [W]: 1 = the tree's root is the DAH's
    uint8_t* shares;             // [W][512]
    uint8_t* nodes;              // [W][D][90]
};

__global__ __launch_bounds__(64 * kBefpWaves) void befp_build_kernel(const BefpBuildArgs a) {
    __shared__ uint4 stage[kBefpWaves][stage_row(kProofMaxD)];
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const uint32_t t = blockIdx.x * kBefpWaves + wave;   // orthogonal tree = position along the accused vector
    const bool live = t < a.W;   // uniform over the wave; no early return: the workgroup meets at the barrier
    const uint32_t W = a.W, D = a.D, p = a.index;   // p: the leaf position in every orthogonal tree
    uint4* st = stage[wave];
    if (live) {
        // accused row i: cell (i, t), in column tree t; accused column i: cell (t, i), in row tree t
        const uint64_t cell = a.axis == 0 ? (uint64_t)p * W + t : (uint64_t)t * W + p;
        if (lane < 32)
            reinterpret_cast<uint4*>(a.shares + (uint64_t)t * kShare)[lane] =
                reinterpret_cast<const uint4*>(a.eds + cell * kShare)[lane];
        bool diff = false;
        for (uint32_t b = lane; b < (uint32_t)kNode; b += 64)
            diff = diff || a.root_slots[(uint64_t)t * kSlot + b] != a.dah[(uint64_t)t * kNode + b];
        const bool any = __any(diff);
        if (lane == 0) a.flags[t] = any ? 0 : 1;
        stage_slots(st, D, lane, [&](uint32_t L) {
            const uint32_t sib = (p >> L) ^ 1u;
            const uint8_t* src;
            if (L == 0)   // a column tree reads the leaf level with stride W
                src = a.leaves + (a.axis == 0 ? (uint64_t)sib * W + t : (uint64_t)t * W + sib) * kSlot;
            else
                src = a.levels + level_offset(W, L, 1, kSlot) + ((uint64_t)t * (W >> L) + sib) * kSlot;
            return StagedSlot{src, ((p >> L) & 1u) ? (uint32_t)__popc(p >> (L + 1))
                                                   : (uint32_t)__popc(p) + L - (uint32_t)__popc(p & ((1u << L) - 1u))};
        });
    }
    __syncthreads();
    if (!live) return;
    store_packed<kNode>(reinterpret_cast<const uint8_t*>(st), D, a.nodes + (uint64_t)t * D * kNode, lane);
}

// Share i of the verifier's upload to cell dest[i] of the grid (~0: the share's proof did not survive),
// and the cell's presence byte: one wave per share.
__global__ __launch_bounds__(64 * kBefpWaves) void befp_scatter_kernel(const uint8_t* __restrict__ shares,
                                                                        const uint32_t* __restrict__ dest, uint32_t m,
                                                                        uint8_t* __restrict__ grid,
                                                                        uint8_t* __restrict__ present) {
    const uint32_t i = blockIdx.x * kBefpWaves + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (i >= m) return;
    const uint32_t d = dest[i];
    if (d == 0xFFFFFFFFu) return;
    if (lane < 32)
        reinterpret_cast<uint4*>(grid + (uint64_t)d * kShare)[lane] =
            reinterpret_cast<const uint4*>(shares + (uint64_t)i * kShare)[lane];
    if (lane == 32) present[d] = 1;
}

// Rebuilt root j against the DAH's: 3 = equal and pushed in order (no fraud), 0 = the fraud is confirmed.
// One wave per proof; the rebuilt root goes out packed.
__global__ __launch_bounds__(64 * kBefpWaves) void befp_compare_kernel(const uint8_t* __restrict__ root_slots,
                                                                        const uint32_t* __restrict__ err,
                                                                        const uint8_t* __restrict__ dah, uint32_t n,
                                                                        uint8_t* __restrict__ verdict,
                                                                        uint8_t* __restrict__ rebuilt) {
    const uint32_t j = blockIdx.x * kBefpWaves + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (j >= n) return;
    bool diff = false;
    for (uint32_t b = lane; b < (uint32_t)kNode; b += 64) {
        const uint8_t v = root_slots[(uint64_t)j * kSlot + b];
        rebuilt[(uint64_t)j * kNode + b] = v;
        diff = diff || v != dah[(uint64_t)j * kNode + b];
    }
    const bool any = __any(diff);
    if (lane == 0) verdict[j] = (!any && err[j] == 0xFFFFFFFFu) ? 3 : 0;
}

constexpr size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

std::string befp_batch_check(const cda_befp_batch* b) {
    if (!b) return "null batch";
    const uint32_t n = b->n_proofs, k = b->k, W = 2 * k;
    if (n == 0) return "";
    if (!is_pow2(k) || k > 512) return "k " + std::to_string(k) + " is not a power of two <= 512";
    if (!b->axes || !b->indexes || !b->row_roots || !b->col_roots || !b->share_off)
        return "null axes / indexes / row_roots / col_roots / share_off";
    auto at = [](uint32_t p, const std::string& what) { return "proof " + std::to_string(p) + ": " + what; };
    if (b->share_off[0] != 0) return at(0, "share_off must start at 0");
    for (uint32_t p = 0; p < n; p++)
        if (b->share_off[p + 1] < b->share_off[p]) return at(p, "share_off decreases");
    if (b->share_off[n] && (!b->positions || !b->shares || !b->nmt_nodes)) return "null positions / shares / nmt_nodes";
    for (uint32_t p = 0; p < n; p++) {
        if (b->axes[p] > 1)
            return at(p, "axis " + std::to_string(b->axes[p]) + " is neither 0 (row) nor 1 (column)");
        if (b->indexes[p] >= W)
            return at(p, "index " + std::to_string(b->indexes[p]) + " is not below the EDS width " + std::to_string(W));
        for (uint32_t i = b->share_off[p]; i < b->share_off[p + 1]; i++) {
            const std::string share = "share " + std::to_string(i - b->share_off[p]) + ": ";
            if (b->positions[i] >= W)
                return at(p, share + "position " + std::to_string(b->positions[i]) + " is not below the EDS width " +
                                 std::to_string(W));
            if (i > b->share_off[p] && b->positions[i] <= b->positions[i - 1])
                return at(p, share + "position " + std::to_string(b->positions[i]) +
                                 " is not above the one before it, " + std::to_string(b->positions[i - 1]) +
                                 ": positions must be strictly ascending");
            if (b->proof_axes && b->proof_axes[i] > 1)
                return at(p, share + "proof_axis " + std::to_string(b->proof_axes[i]) +
                                 " is neither 0 (row) nor 1 (column)");
        }
    }
    return "";
}

// One of `eds` (host, staged in h_eds_) / `d_eds` (device, read where it lies) is set.
int Engine::befp_build(const uint8_t* eds, const uint8_t* d_eds, uint32_t W, int axis, uint32_t index,
                       const uint8_t* row_roots, const uint8_t* col_roots, uint32_t* n_out, uint32_t* positions,
                       uint8_t* shares, uint8_t* nmt_nodes) {
    if (W < 2 || !is_pow2(W) || W > 1024) return fail(CDA_ERR_INVALID, "EDS width must be a power of two in [2, 1024]");
    if (axis != 0 && axis != 1)
        return fail(CDA_ERR_INVALID, "axis " + std::to_string(axis) + " is neither 0 (row) nor 1 (column)");
    if (index >= W)
        return fail(CDA_ERR_INVALID, "index " + std::to_string(index) + " is not below the EDS width " + std::to_string(W));
    const uint32_t k = W / 2, D = ceil_log2(W);
    const size_t eds_b = (size_t)W * W * kShare;
    hipStream_t s = stream_;
    const uint8_t* E = d_eds;
    if (!d_eds) {
        CDA_TRY(ensure(h_eds_, eds_b, "hipMalloc"));
        CDA_TRY(h2d(h_eds_.ptr, eds, eds_b, s, "H2D"));
        E = h_eds_.as<uint8_t>();
    }
    // scratch: leaf slots | levels 1.. of the orthogonal trees | their root slots | the DAH's roots | a push-order
    // word nobody reads (the leaf kernel wants one)
    const size_t leaf_b = (size_t)W * W * kSlot, lev_b = level_offset(W, D + 1, 1, kSlot), roots_b = (size_t)W * kSlot,
                 dah_b = pad16((size_t)W * kNode);
    CDA_TRY(ensure(bf_levels_, leaf_b + lev_b + roots_b + dah_b + 16, "hipMalloc"));
    uint8_t* leaf = bf_levels_.as<uint8_t>();
    uint8_t* lev = leaf + leaf_b;
    uint8_t* root_slots = lev + lev_b;
    uint8_t* dah = root_slots + roots_b;
    uint32_t* d_err = reinterpret_cast<uint32_t*>(dah + dah_b);
    // outputs: flags | shares | nodes, one copy back
    const size_t flags_b = pad16(W), shares_b = (size_t)W * kShare, nodes_b = (size_t)W * D * kNode,
                 out_b = flags_b + shares_b + nodes_b;
    CDA_TRY(ensure(bf_out_, out_b, "hipMalloc"));
    uint8_t* out = bf_out_.as<uint8_t>();
    CDA_TRY(h2d(dah, axis == 0 ? col_roots : row_roots, (size_t)W * kNode, s, "H2D roots"));
    CDA_TRY(fill(d_err, 0xFF, 4, s, "hipMemsetAsync"));
    const CellGrid g{E, 0, W, W, W, 0, 0, k};
    CDA_TRY(check(launch_leaves(g, 1, leaf, d_err, false, false, s), "leaf hashing"));
    // the orthogonal forest: column trees (stride W through the leaf level) for a row, row trees for a column
    Forest f = axis == 0 ? Forest{leaf, 0, W, 1, W, nullptr, 0, nullptr, 0, root_slots, 0, 0}
                         : Forest{leaf, 0, W, W, 1, nullptr, 0, nullptr, 0, root_slots, 0, 0};
    uint32_t L = 1;
    for (uint32_t m = W; m >= 2; m /= 2, L++) {
        f.out = lev + level_offset(W, L, 1, kSlot);
        CDA_TRY(check(launch_level(&f, 1, m, 1, s), "nmt level"));
        f.in = f.out;
        f.tree_stride = m / 2;
        f.node_stride = 1;
    }
    const BefpBuildArgs a{E, leaf, lev, root_slots, dah, W, D, (uint32_t)axis, index, out, out + flags_b,
                          out + flags_b + shares_b};
    hipLaunchKernelGGL(befp_build_kernel, dim3((W + kBefpWaves - 1) / kBefpWaves), dim3(64 * kBefpWaves), 0, s, a);
    CDA_TRY(launched("fraud proof shares"));
    std::vector<uint8_t> host(out_b);
    CDA_TRY(d2h(host.data(), out, out_b, s, "D2H fraud proof"));
    CDA_TRY(sync(s));
    uint32_t n = 0;
    for (uint32_t p = 0; p < W; p++) {
        if (!host[p]) continue;
        positions[n] = p;
        std::memcpy(shares + (size_t)n * kShare, host.data() + flags_b + (size_t)p * kShare, kShare);
        std::memcpy(nmt_nodes + (size_t)n * D * kNode, host.data() + flags_b + shares_b + (size_t)p * D * kNode,
                    (size_t)D * kNode);
        n++;
    }
    *n_out = n;
    return CDA_OK;
}

int Engine::befp_verify(const cda_befp_batch* b, uint8_t* verdict, uint8_t* rebuilt_roots) {
    const std::string bad = befp_batch_check(b);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    const uint32_t P = b->n_proofs;
    if (P == 0) return CDA_OK;
    if (!verdict) return fail(CDA_ERR_INVALID, "null verdict buffer");
    const uint32_t k = b->k, W = 2 * k, D = ceil_log2(W), m = b->share_off[P];
    const size_t dah_b = (size_t)W * kNode;
    // the DAH root proof p's share i is proven against, and the root of the accused vector itself
    auto dah_root = [&](uint32_t p, uint32_t axis, uint32_t i) {
        return (axis == 0 ? b->row_roots : b->col_roots) + (size_t)p * dah_b + (size_t)i * kNode;
    };
    std::vector<uint8_t> v(P, 0);
    for (uint32_t p = 0; p < P; p++)
        if (b->share_off[p + 1] - b->share_off[p] < k) v[p] = 1;   // step 1
    // ---- step 2: every share under the root its proof names.  Everything a prover could lie about is derived
    // from (axis, index, position, proof axis): the cell, hence the leaf namespace; the tree; the leaf position.
    std::vector<uint8_t> sv(m, 0);
    if (m) {
        std::vector<uint8_t> ns((size_t)m * kNs), roots((size_t)m * kNode);
        std::vector<uint32_t> seg_off(m + 1), node_off(m + 1);
        std::vector<int32_t> st(m), en(m);
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t axis = b->axes[p], idx = b->indexes[p];
            for (uint32_t i = b->share_off[p]; i < b->share_off[p + 1]; i++) {
                const uint32_t pos = b->positions[i], pax = b->proof_axes ? b->proof_axes[i] : 1u - axis;
                const uint32_t row = axis == 0 ? idx : pos, col = axis == 0 ? pos : idx;
                if (row < k && col < k) std::memcpy(&ns[(size_t)i * kNs], b->shares + (size_t)i * kShare, kNs);
                else std::memset(&ns[(size_t)i * kNs], 0xFF, kNs);
                const uint32_t tree = pax == axis ? idx : pos, leaf = pax == axis ? pos : idx;
                st[i] = (int32_t)leaf;
                en[i] = (int32_t)leaf + 1;
                std::memcpy(&roots[(size_t)i * kNode], dah_root(p, pax, tree), kNode);
            }
        }
        for (uint32_t i = 0; i <= m; i++) {
            seg_off[i] = i;
            node_off[i] = i * D;
        }
        cda_share_proof_batch sb{};
        sb.n_proofs = m;
        sb.ns_len = kNs;
        sb.share_len = kShare;
        sb.namespaces = ns.data();
        sb.seg_off = seg_off.data();
        sb.nmt_start = st.data();
        sb.nmt_end = en.data();
        sb.node_off = node_off.data();
        sb.nodes = b->nmt_nodes;
        sb.n_nodes = m * D;
        sb.row_roots = roots.data();
        sb.shares = b->shares;
        sb.n_shares = m;
        CDA_TRY(share_proofs_verify(&sb, sv.data()));   // synchronises: the host selects the survivors
    }
    std::vector<uint32_t> alive;   // proofs that reach step 3
    for (uint32_t p = 0; p < P; p++) {
        if (v[p]) continue;
        for (uint32_t i = b->share_off[p]; i < b->share_off[p + 1] && !v[p]; i++)
            if (sv[i]) v[p] = 2;
        if (!v[p]) alive.push_back(p);
    }
    if (rebuilt_roots) std::memset(rebuilt_roots, 0, (size_t)P * kNode);
    const uint32_t n = (uint32_t)alive.size();
    if (n == 0) {
        std::memcpy(verdict, v.data(), P);
        return CDA_OK;
    }
    // ---- step 3: the survivors' vectors as rows of an [n][W] grid
    hipStream_t s = stream_;
    rp_host_used_ = 0;   // the stream is idle: earlier copies out of the pinned staging are done
    std::vector<uint32_t> dest(m, 0xFFFFFFFFu), cw, tree_axis(n);
    std::vector<uint8_t> want((size_t)n * kNode);
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t p = alive[j];
        for (uint32_t i = b->share_off[p]; i < b->share_off[p + 1]; i++) dest[i] = j * W + b->positions[i];
        if (b->share_off[p + 1] - b->share_off[p] < W) {   // Codec.Decode: a complete vector comes back as it is
            cw.push_back(0);
            cw.push_back(j);
        }
        tree_axis[j] = b->indexes[p];
        std::memcpy(&want[(size_t)j * kNode], dah_root(p, b->axes[p], b->indexes[p]), kNode);
    }
    const size_t dest_b = pad16((size_t)m * 4), want_b = pad16((size_t)n * kNode), verd_b = pad16(n),
                 res_b = verd_b + (size_t)n * kNode;
    CDA_TRY(ensure(bf_in_, dest_b + want_b + res_b, "hipMalloc"));
    const size_t grid_b = (size_t)n * W * kShare;
    CDA_TRY(ensure(bf_grid_, grid_b + (size_t)n * W, "hipMalloc"));
    uint8_t* in = bf_in_.as<uint8_t>();
    uint8_t* grid = bf_grid_.as<uint8_t>();
    uint8_t* present = grid + grid_b;
    uint8_t* d_verdict = in + dest_b + want_b;
    uint8_t* d_rebuilt = d_verdict + verd_b;
    CDA_TRY(h2d(in, dest.data(), (size_t)m * 4, s, "H2D fraud proof shares"));
    CDA_TRY(h2d(in + dest_b, want.data(), (size_t)n * kNode, s, "H2D fraud proof roots"));
    CDA_TRY(fill(present, 0, (size_t)n * W, s, "hipMemsetAsync"));
    hipLaunchKernelGGL(befp_scatter_kernel, dim3((m + kBefpWaves - 1) / kBefpWaves), dim3(64 * kBefpWaves), 0, s,
                       vp_shares_dev_, reinterpret_cast<const uint32_t*>(in), m, grid, present);
    CDA_TRY(launched("fraud proof scatter"));
    CDA_TRY(decode_codewords(grid, present, k, kShare, cw, s));
    // Codec.Encode of every data half over its parity half; the RS descriptors hold 32-bit offsets
    const uint32_t max_cw = (uint32_t)(0xFFFFFFFFull / ((uint64_t)W * kShare));
    for (uint32_t j0 = 0; j0 < n; j0 += max_cw) {
        const uint32_t cnt = n - j0 < max_cw ? n - j0 : max_cw;
        RsJob job{};
        job.src = grid + (size_t)j0 * W * kShare;
        job.dst = grid + (size_t)j0 * W * kShare;
        job.n_seg = 1;
        job.seg[0] = RsSeg{cnt, 0, W * (uint32_t)kShare, (uint32_t)kShare, k * (uint32_t)kShare,
                           W * (uint32_t)kShare, (uint32_t)kShare};
        CDA_TRY(check(launch_rs(job, k, 1, gf16(k), s), "fraud proof re-encode"));
    }
    uint32_t* d_err = nullptr;
    uint64_t root_off = 0;
    CDA_TRY(build_trees_device(grid, kShare, W, n, k, tree_axis.data(), &d_err, s, &root_off));
    hipLaunchKernelGGL(befp_compare_kernel, dim3((n + kBefpWaves - 1) / kBefpWaves), dim3(64 * kBefpWaves), 0, s,
                       tr_levels_.as<uint8_t>() + root_off, d_err, in + dest_b, n, d_verdict, d_rebuilt);
    CDA_TRY(launched("fraud proof compare"));
    std::vector<uint8_t> res(res_b);
    CDA_TRY(d2h(res.data(), d_verdict, res_b, s, "D2H fraud proof verdicts"));
    CDA_TRY(sync(s));
    for (uint32_t j = 0; j < n; j++) {
        v[alive[j]] = res[j];
        if (rebuilt_roots) std::memcpy(rebuilt_roots + (size_t)alive[j] * kNode, &res[verd_b + (size_t)j * kNode], kNode);
    }
    std::memcpy(verdict, v.data(), P);
    return CDA_OK;
}

// Axis halves against the DAH (celestia-node's shwap Row.Verify, EXT; restated in tests/axis_halves_ref.py):
// half i holds cells sides[i] * k .. + k - 1 of vector (axes[i], indexes[i]) of square squares[i].  The halves
// are ordered by side into an [n][2k][512] grid, every codeword is completed -- a left half by the encoder, a
// right half by its mirror (launch_rs_recover: the data from the parity alone) -- the vectors are hashed as
// erasured trees with one push-order word each (tree.hip) and the roots compared with the DAHs' by the fraud
// proofs' compare kernel.  verdict[i] = 0 valid, 2 nmt would refuse a push (checked first), 1 the root differs.
int Engine::axis_halves_verify(uint32_t k, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t n_squares,
                               const uint32_t* squares, const uint8_t* axes, const uint32_t* indexes,
                               const uint8_t* sides, uint32_t n, const uint8_t* shares, uint8_t* verdict,
                               uint8_t* vectors) {
    CDA_TRY(check_width(k));
    if (n == 0) return CDA_OK;
    if (!row_roots || !axes || !indexes || !sides || !shares || !verdict) return fail(CDA_ERR_INVALID, "null buffer");
    const std::string bad = axis_halves_check(k, n_squares, squares, axes, indexes, sides, n);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    if (!col_roots)
        for (uint32_t i = 0; i < n; i++)
            if (axes[i] == 1)
                return fail(CDA_ERR_INVALID, "half " + std::to_string(i) + ": axis 1 (column) needs col_roots, which is NULL");
    const uint32_t W = 2 * k;
    const size_t half_b = (size_t)k * kShare, vec_b = 2 * half_b, dah_b = (size_t)W * kNode;
    // grid row of half i: the left halves first, each side in the caller's order
    uint32_t n_left = 0;
    for (uint32_t i = 0; i < n; i++) n_left += sides[i] == 0;
    std::vector<uint32_t> pos(n), tree_axis(n);
    std::vector<uint8_t> want((size_t)n * kNode);
    for (uint32_t i = 0, l = 0, r = n_left; i < n; i++) {
        const uint32_t j = pos[i] = sides[i] ? r++ : l++;
        tree_axis[j] = indexes[i];
        const uint8_t* dah = (axes[i] ? col_roots : row_roots) + (squares ? squares[i] : 0u) * dah_b;
        std::memcpy(&want[(size_t)j * kNode], dah + (size_t)indexes[i] * kNode, kNode);
    }
    hipStream_t s = stream_;
    const size_t want_b = pad16((size_t)n * kNode), verd_b = pad16(n);
    CDA_TRY(ensure(bf_in_, want_b + verd_b + (size_t)n * kNode, "hipMalloc"));
    CDA_TRY(ensure(bf_grid_, (size_t)n * vec_b, "hipMalloc"));
    uint8_t* in = bf_in_.as<uint8_t>();
    uint8_t* grid = bf_grid_.as<uint8_t>();
    uint8_t* d_verdict = in + want_b;
    uint8_t* d_rebuilt = d_verdict + verd_b;
    CDA_TRY(h2d(in, want.data(), (size_t)n * kNode, s, "H2D axis half roots"));
    // a run of halves of one side lies in consecutive grid rows: one strided copy per run, each way
    auto runs = [&](auto&& f) -> int {
        for (uint32_t i = 0; i < n;) {
            uint32_t e = i + 1;
            while (e < n && sides[e] == sides[i]) e++;
            CDA_TRY(f(i, e - i));
            i = e;
        }
        return CDA_OK;
    };
    CDA_TRY(runs([&](uint32_t i, uint32_t cnt) {
        return check(hipMemcpy2DAsync(grid + (size_t)pos[i] * vec_b + sides[i] * half_b, vec_b,
                                      shares + (size_t)i * half_b, half_b, half_b, cnt, hipMemcpyHostToDevice, s),
                     "H2D axis halves");
    }));
    // the RS descriptors hold 32-bit offsets: chunks of codewords below 4 GiB
    const uint32_t max_cw = (uint32_t)(0xFFFFFFFFull / vec_b);
    for (uint32_t side = 0; side < 2; side++) {
        const uint32_t j_end = side ? n : n_left;
        for (uint32_t j0 = side ? n_left : 0; j0 < j_end; j0 += max_cw) {
            const uint32_t cnt = j_end - j0 < max_cw ? j_end - j0 : max_cw;
            RsJob job{};
            job.src = job.dst = grid + (size_t)j0 * vec_b;
            job.n_seg = 1;
            const uint32_t data = 0, parity = (uint32_t)half_b, sh = (uint32_t)kShare;
            if (side == 0) {
                job.seg[0] = RsSeg{cnt, data, (uint32_t)vec_b, sh, parity, (uint32_t)vec_b, sh};
                CDA_TRY(check(launch_rs(job, k, 1, gf16(k), s), "axis halves encode"));
            } else {
                job.seg[0] = RsSeg{cnt, parity, (uint32_t)vec_b, sh, data, (uint32_t)vec_b, sh};
                CDA_TRY(check(launch_rs_recover(job, k, 1, gf16(k), s), "axis halves recover"));
            }
        }
    }
    uint32_t* d_err = nullptr;
    uint64_t root_off = 0;
    CDA_TRY(build_trees_device(grid, kShare, W, n, k, tree_axis.data(), &d_err, s, &root_off));
    hipLaunchKernelGGL(befp_compare_kernel, dim3((n + kBefpWaves - 1) / kBefpWaves), dim3(64 * kBefpWaves), 0, s,
                       tr_levels_.as<uint8_t>() + root_off, d_err, in, n, d_verdict, d_rebuilt);
    CDA_TRY(launched("axis halves compare"));
    std::vector<uint8_t> same(n);   // the compare kernel's 3: equal and in order
    std::vector<uint32_t> err(n);
    CDA_TRY(d2h(same.data(), d_verdict, n, s, "D2H axis half verdicts"));
    CDA_TRY(d2h(err.data(), d_err, (size_t)n * 4, s, "D2H axis half push order"));
    if (vectors)
        CDA_TRY(runs([&](uint32_t i, uint32_t cnt) {
            return d2h(vectors + (size_t)i * vec_b, grid + (size_t)pos[i] * vec_b, (size_t)cnt * vec_b, s,
                       "D2H axis vectors");
        }));
    CDA_TRY(sync(s));
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t j = pos[i];
        verdict[i] = err[j] != push_order::kOrdered ? 2 : same[j] == 3 ? 0 : 1;
    }
    return CDA_OK;
}

}  // namespace cda
