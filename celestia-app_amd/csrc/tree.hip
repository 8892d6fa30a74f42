// tree.hip -- standalone erasured NMT trees and generic RFC-6962 roots.
//
// Reference behaviour (paths under /root/reference):
//   * pkg/wrapper/nmt_wrapper.go:55-140: NewErasuredNamespacedMerkleTree,
//     Push (leaf namespace = data[0:29] when isQuadrantZero, else
//     ParitySharesNamespace), Root, ProveRange -- used outside
//     ComputeExtendedDataSquare by pkg/proof/proof.go:157-189,
//     pkg/inclusion/nmt_caching.go:96-109 and test/util/malicious/tree.go:46-70.
//   * nmt v0.22.0 (EXT; hasher rules copied in-tree at
//     test/util/malicious/hasher.go:186-310): computeRoot splits n leaves at
//     the largest power of two < n (RFC-6962).  Pairing adjacent nodes level by
//     level and promoting an odd last node unchanged builds the same tree, so
//     every level is one launch for all trees whatever n is.
//   * go-square/merkle HashFromByteSlices (RFC-6962, same split rule) over
//     arbitrary byte slices: (*DataAvailabilityHeader).Hash,
//     pkg/da/data_availability_header.go:92-108, for any root count / size.
//
// The square-shaped case (512-B cells, power-of-two leaf count, consecutive
// axis indexes) runs on the tuned leaf/level kernels of nmt.hip; these generic
// kernels take any cell length and leaf count (byte-addressed message build).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "leaf_dev.h"
#include "sha_bytes_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

// One leaf per (tree, push): slot = ns || ns || sha256(0x00 || ns || cell).
// err[t] = min push position whose namespace is below the previous one.
__global__ __launch_bounds__(256) void gen_leaf_kernel(const uint8_t* __restrict__ cells, uint32_t cell_len,
                                                      uint32_t n_cells, uint32_t n_trees, uint32_t square_size,
                                                      const uint32_t* __restrict__ axis, uint8_t* __restrict__ slots,
                                                      uint32_t* __restrict__ err) {
    const uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (uint64_t)n_trees * n_cells) return;
    const uint32_t t = (uint32_t)(id / n_cells), i = (uint32_t)(id % n_cells);
    const uint32_t ax = axis[t];
    const uint8_t* cell = cells + id * cell_len;
    const bool parity = !(i < square_size && ax < square_size);   // isQuadrantZero
    uint32_t ns[8];
    load_ns_bytes(cell, parity, ns);
    uint8_t nsb[kNs];
#pragma unroll
    for (int j = 0; j < kNs; j++) nsb[j] = (uint8_t)(ns[j / 4] >> (24 - 8 * (j % 4)));
    uint32_t d[8];
    sha_cat(0x00, nsb, kNs, cell, cell_len, d);
    uint32_t out[kSlotWords];
    leaf_node_words(ns, d, out);
    store_slot(slots + id * kSlot, out);
    if (i > 0) {
        uint32_t prev[8];
        load_ns_bytes(cell - cell_len, !((i - 1) < square_size && ax < square_size), prev);
        if (ns_less(ns, prev)) atomicMin(err + t, i);
    }
}

// One level of every tree: parent p of tree t = HashNode(2p, 2p+1), or the
// odd last node promoted unchanged (RFC-6962 split, see the header).
__global__ __launch_bounds__(256) void gen_level_kernel(const uint8_t* __restrict__ in, uint32_t n_in,
                                                       uint8_t* __restrict__ out, uint32_t n_trees, uint64_t in_tree,
                                                       uint64_t out_tree) {
    const uint32_t n_out = (n_in + 1) / 2;
    const uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (uint64_t)n_trees * n_out) return;
    const uint32_t t = (uint32_t)(id / n_out), p = (uint32_t)(id % n_out);
    const uint8_t* l = in + t * in_tree + (uint64_t)(2 * p) * kSlot;
    uint8_t* o = out + t * out_tree + (uint64_t)p * kSlot;
    if (2 * p + 1 >= n_in) {
        const uint4* s = reinterpret_cast<const uint4*>(l);
        uint4* d = reinterpret_cast<uint4*>(o);
#pragma unroll
        for (int q = 0; q < 6; q++) d[q] = s[q];
        return;
    }
    uint32_t L[kSlotWords], R[kSlotWords], ow[kSlotWords];
    load_slot_be(l, L);
    load_slot_be(l + kSlot, R);
    hash_node_u<false>(L, R, ow, false);
    store_slot(o, ow);
}

// RFC-6962 leaf digests of arbitrary byte items: sha256(0x00 || item).
__global__ __launch_bounds__(256) void gen_rfc_leaf_kernel(const uint8_t* __restrict__ items,
                                                          const uint64_t* __restrict__ off, uint32_t n,
                                                          uint32_t* __restrict__ dig) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t d[8];
    sha_cat(0x00, items + off[i], off[i + 1] - off[i], nullptr, 0, d);
#pragma unroll
    for (int j = 0; j < 8; j++) dig[(size_t)i * 8 + j] = d[j];
}

// RFC-6962 inner levels of one tree of n digests in a single workgroup
// (pairs hashed, an odd last digest promoted); dig is overwritten.
__global__ __launch_bounds__(256) void gen_rfc_levels_kernel(uint32_t* __restrict__ dig, uint32_t n,
                                                            uint8_t* __restrict__ root) {
    for (uint32_t m = n; m > 1; m = (m + 1) / 2) {
        const uint32_t half = m / 2;
        // parents are written in place over slots 0..half-1 after all reads
        // of this level: first hash into registers, then barrier, then store
        for (uint32_t base = 0; base < half; base += blockDim.x) {
            const uint32_t p = base + threadIdx.x;
            uint32_t h[8];
            if (p < half) {
                uint32_t A[8], B[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { A[j] = dig[(2 * p) * 8 + j]; B[j] = dig[(2 * p + 1) * 8 + j]; }
                rfc_inner_plain(A, B, h);
            }
            __syncthreads();
            if (p < half) {
#pragma unroll
                for (int j = 0; j < 8; j++) dig[p * 8 + j] = h[j];
            }
            __syncthreads();
        }
        if (m & 1) {   // promote the odd last digest to slot half
            if (threadIdx.x < 8) dig[half * 8 + threadIdx.x] = dig[(m - 1) * 8 + threadIdx.x];
            __syncthreads();
        }
    }
    if (threadIdx.x < 8) reinterpret_cast<uint32_t*>(root)[threadIdx.x] = bswap32(dig[threadIdx.x]);
}

// Copy n 96-B slots at byte offsets src_off[i] of `base` into packed 90-B nodes.
__global__ __launch_bounds__(64) void gen_gather_nodes_kernel(const uint8_t* __restrict__ base,
                                                             const uint64_t* __restrict__ src_off, uint32_t n,
                                                             uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    for (uint32_t b = threadIdx.x; b < (uint32_t)kNode; b += blockDim.x) out[(size_t)i * kNode + b] = base[src_off[i] + b];
}

// Pack tree roots (slot 0 of the last level of tree t) into 90-B roots.
__global__ __launch_bounds__(96) void gen_pack_roots_kernel(const uint8_t* __restrict__ top, uint64_t tree_stride,
                                                           uint32_t n_trees, uint8_t* __restrict__ roots) {
    const uint32_t t = blockIdx.x;
    if (t < n_trees && threadIdx.x < (uint32_t)kNode)
        roots[(size_t)t * kNode + threadIdx.x] = top[t * tree_stride + threadIdx.x];
}

}  // namespace

// All levels of n_trees erasured trees over host cells into tr_ (device):
// level L of tree t at tr_ + off[L] + t * count[L] * 96.  err words per tree.
int Engine::build_trees(const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t n_trees,
                        uint32_t square_size, const uint32_t* axis, std::vector<uint64_t>* level_off,
                        std::vector<uint32_t>* err_out) {
    hipStream_t s = stream_;
    const std::vector<uint32_t> cnt = level_counts(n_cells);
    level_off->assign(cnt.size(), 0);
    uint64_t total = 0;
    for (size_t L = 0; L < cnt.size(); L++) {
        (*level_off)[L] = total;
        total += (uint64_t)cnt[L] * n_trees * kSlot;
    }
    const uint64_t cells_b = (uint64_t)n_trees * n_cells * cell_len;
    CDA_TRY(ensure(tr_cells_, cells_b + 16, "hipMalloc tree cells"));
    CDA_TRY(h2d(tr_cells_.ptr, cells, cells_b, s, "H2D"));
    uint32_t* d_err = nullptr;
    CDA_TRY(build_trees_device(tr_cells_.as<uint8_t>(), cell_len, n_cells, n_trees, square_size, axis, &d_err, s));
    err_out->assign(n_trees, 0);
    CDA_TRY(d2h(err_out->data(), d_err, (size_t)n_trees * 4, s, "D2H"));
    return CDA_OK;
}

// The same trees over cells that already lie in device memory (befp.hip: the rebuilt vectors): every level into
// tr_levels_ at build_trees' offsets, *d_err = one push-order word per tree (the bare push position of the first
// violation, ~0 = ordered), in tr_axis_; *root_off (optional) = bytes into tr_levels_ of the root slots, one per
// tree.  Enqueue only.
int Engine::build_trees_device(const uint8_t* d_cells, uint32_t cell_len, uint32_t n_cells, uint32_t n_trees,
                               uint32_t square_size, const uint32_t* axis, uint32_t** d_err_out, hipStream_t s,
                               uint64_t* root_off) {
    const std::vector<uint32_t> cnt = level_counts(n_cells);
    std::vector<uint64_t> off(cnt.size(), 0);
    uint64_t total = 0;
    for (size_t L = 0; L < cnt.size(); L++) {
        off[L] = total;
        total += (uint64_t)cnt[L] * n_trees * kSlot;
    }
    CDA_TRY(ensure(tr_levels_, total, "hipMalloc tree levels"));
    CDA_TRY(ensure(tr_axis_, (size_t)n_trees * 8, "hipMalloc tree axes"));
    uint32_t* d_axis = tr_axis_.as<uint32_t>();
    uint32_t* d_err = d_axis + n_trees;
    *d_err_out = d_err;
    if (root_off) *root_off = off.back();
    CDA_TRY(h2d(d_axis, axis, (size_t)n_trees * 4, s, "H2D"));
    CDA_TRY(fill(d_err, 0xFF, (size_t)n_trees * 4, s, "hipMemsetAsync"));
    uint8_t* lv = tr_levels_.as<uint8_t>();
    const uint64_t n_leaves = (uint64_t)n_trees * n_cells;
    hipLaunchKernelGGL(gen_leaf_kernel, dim3((uint32_t)((n_leaves + 255) / 256)), dim3(256), 0, s, d_cells, cell_len,
                       n_cells, n_trees, square_size, d_axis, lv, d_err);
    CDA_TRY(launched("tree leaves"));
    for (size_t L = 1; L < cnt.size(); L++) {
        const uint64_t work = (uint64_t)n_trees * cnt[L];
        hipLaunchKernelGGL(gen_level_kernel, dim3((uint32_t)((work + 255) / 256)), dim3(256), 0, s,
                           lv + off[L - 1], cnt[L - 1], lv + off[L], n_trees, (uint64_t)cnt[L - 1] * kSlot,
                           (uint64_t)cnt[L] * kSlot);
        CDA_TRY(launched("tree level"));
    }
    return CDA_OK;
}

int Engine::tree_order_error(const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                             const uint32_t* axis, const std::vector<uint32_t>& err, int32_t* status) {
    // (these trees' words are the bare push position of the first violation, ~0 = ordered)
    push_order::fill_status(err.data(), err.size(), status);
    for (size_t t = 0; t < err.size(); t++) {
        if (err[t] == push_order::kOrdered) continue;
        const uint32_t i = err[t];
        auto ns = [&](uint32_t pos) -> const uint8_t* {   // NULL: a parity cell
            const bool par = !(pos < square_size && axis[t] < square_size);
            return par ? nullptr : cells + ((uint64_t)t * n_cells + pos) * cell_len;
        };
        po_axis = 0;
        po_index = axis[t];
        po_pos = i;
        return fail_push_order(ns(i - 1), ns(i));
    }
    return CDA_OK;
}

int Engine::nmt_axis_roots(const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t n_trees,
                           uint32_t square_size, const uint32_t* axis, uint8_t* roots, int32_t* status) {
    if (n_cells == 0) {   // no pushes: NmtHasher.EmptyRoot = 0^29 || 0^29 || sha256("")
        for (uint32_t t = 0; t < n_trees; t++) {
            memset(roots + (size_t)t * kNode, 0, 2 * kNs);
            memcpy(roots + (size_t)t * kNode + 2 * kNs, kSha256Empty, 32);
            if (status) status[t] = CDA_OK;
        }
        return CDA_OK;
    }
    hipStream_t s = stream_;
    bool consecutive = true;
    for (uint32_t t = 1; t < n_trees; t++) consecutive = consecutive && axis[t] == axis[0] + t;
    if (cell_len == (uint32_t)kShare && n_cells >= 2 && is_pow2(n_cells) && consecutive && axis[0] + n_trees <= 4096 &&
        n_cells < 4096) {
        // square-shaped: the tuned leaf / level kernels of nmt.hip
        const uint64_t cells_b = (uint64_t)n_trees * n_cells * kShare, slots = (uint64_t)n_trees * n_cells * kSlot;
        CDA_TRY(ensure(tr_cells_, cells_b, "hipMalloc tree cells"));
        CDA_TRY(ensure(tr_levels_, 2 * slots, "hipMalloc tree levels"));
        CDA_TRY(ensure(tr_axis_, (size_t)n_trees * kNode + 64, "hipMalloc tree roots"));
        uint8_t* d_roots = tr_axis_.as<uint8_t>();
        uint32_t* d_err = reinterpret_cast<uint32_t*>(d_roots + (((size_t)n_trees * kNode + 15) & ~(size_t)15));
        uint8_t* leaf = tr_levels_.as<uint8_t>();
        uint8_t* lvl = leaf + slots;
        CDA_TRY(h2d(tr_cells_.ptr, cells, cells_b, s, "H2D"));
        CDA_TRY(fill(d_err, 0xFF, 4, s, "hipMemsetAsync"));
        const CellGrid g{tr_cells_.as<uint8_t>(), 0, n_trees, n_cells, n_cells, axis[0], 0, square_size};
        CDA_TRY(check(launch_leaves(g, 1, leaf, d_err, true, false, s), "leaf hashing"));
        Forest f{leaf, 0, n_trees, n_cells, 1, nullptr, 0, d_roots, 0, nullptr, 0, 0};
        const uint64_t off0[1] = {0};
        CDA_TRY(run_forests(&f, 1, n_cells, 1, lvl, leaf, 0, off0, s));
        uint32_t err = 0;
        CDA_TRY(d2h(roots, d_roots, (size_t)n_trees * kNode, s, "D2H"));
        CDA_TRY(read_push_order(d_err, 1, &err, s));
        // err = min over the batch's violations: a single word cannot tell
        // which other trees broke push order, so a batch with any violation
        // is re-run on the generic kernels, which keep one word per tree
        // (rare: an honest square never gets here)
        if (err == push_order::kOrdered) {
            if (status)
                for (uint32_t t = 0; t < n_trees; t++) status[t] = CDA_OK;
            return CDA_OK;
        }
    }
    std::vector<uint64_t> off;
    std::vector<uint32_t> err;
    CDA_TRY(build_trees(cells, cell_len, n_cells, n_trees, square_size, axis, &off, &err));
    CDA_TRY(ensure(tr_roots_, (size_t)n_trees * kNode, "hipMalloc tree roots"));
    hipLaunchKernelGGL(gen_pack_roots_kernel, dim3(n_trees), dim3(96), 0, s, tr_levels_.as<uint8_t>() + off.back(),
                       (uint64_t)kSlot, n_trees, tr_roots_.as<uint8_t>());
    CDA_TRY(launched("pack roots"));
    CDA_TRY(d2h(roots, tr_roots_.ptr, (size_t)n_trees * kNode, s, "D2H"));
    CDA_TRY(sync(s));
    return tree_order_error(cells, cell_len, n_cells, square_size, axis, err, status);
}

int Engine::nmt_prove_range(const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                            uint32_t axis, uint32_t start, uint32_t end, uint8_t* nodes, uint32_t* n_nodes,
                            uint8_t* root) {
    if (start >= end || end > n_cells) return fail(CDA_ERR_INVALID, "invalid proof range");
    hipStream_t s = stream_;
    std::vector<uint64_t> off;
    std::vector<uint32_t> err;
    CDA_TRY(build_trees(cells, cell_len, n_cells, 1, square_size, &axis, &off, &err));
    std::vector<std::pair<uint32_t, uint32_t>> ids;
    prove_nodes(0, n_cells, start, end, ids);
    const std::vector<uint32_t> cnt = level_counts(n_cells);
    std::vector<uint64_t> src(ids.size() + 1);
    for (size_t i = 0; i < ids.size(); i++) src[i] = off[ids[i].first] + (uint64_t)ids[i].second * kSlot;
    src[ids.size()] = off.back();   // the root
    const uint32_t n = (uint32_t)src.size();
    CDA_TRY(ensure(tr_roots_, (size_t)n * (kNode + 8) + 64, "hipMalloc proof nodes"));
    uint64_t* d_src = tr_roots_.as<uint64_t>();
    uint8_t* d_out = tr_roots_.as<uint8_t>() + (size_t)n * 8;
    CDA_TRY(h2d(d_src, src.data(), (size_t)n * 8, s, "H2D"));
    hipLaunchKernelGGL(gen_gather_nodes_kernel, dim3(n), dim3(64), 0, s, tr_levels_.as<uint8_t>(), d_src, n, d_out);
    CDA_TRY(launched("gather nodes"));
    std::vector<uint8_t> host((size_t)n * kNode);
    CDA_TRY(d2h(host.data(), d_out, host.size(), s, "D2H"));
    CDA_TRY(sync(s));
    CDA_TRY(tree_order_error(cells, cell_len, n_cells, square_size, &axis, err, nullptr));
    if (nodes) memcpy(nodes, host.data(), (size_t)(n - 1) * kNode);
    if (n_nodes) *n_nodes = n - 1;
    if (root) memcpy(root, host.data() + (size_t)(n - 1) * kNode, kNode);
    return CDA_OK;
}

int Engine::merkle_root(const uint8_t* items, const uint64_t* off, uint32_t n, uint8_t* out) {
    hipStream_t s = stream_;
    const uint64_t bytes = off[n] - off[0];
    std::vector<uint64_t> rel(n + 1);
    for (uint32_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    CDA_TRY(ensure(tr_cells_, bytes + 16, "hipMalloc merkle items"));
    CDA_TRY(ensure(tr_levels_, (size_t)n * 32, "hipMalloc merkle digests"));
    CDA_TRY(ensure(tr_axis_, (size_t)(n + 1) * 8 + 64, "hipMalloc merkle offsets"));
    uint64_t* d_off = tr_axis_.as<uint64_t>();
    uint8_t* d_root = reinterpret_cast<uint8_t*>(d_off + n + 1);
    if (bytes) CDA_TRY(h2d(tr_cells_.ptr, items + off[0], bytes, s, "H2D"));
    CDA_TRY(h2d(d_off, rel.data(), (size_t)(n + 1) * 8, s, "H2D"));
    hipLaunchKernelGGL(gen_rfc_leaf_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tr_cells_.as<uint8_t>(), d_off, n,
                       tr_levels_.as<uint32_t>());
    CDA_TRY(launched("merkle leaves"));
    hipLaunchKernelGGL(gen_rfc_levels_kernel, dim3(1), dim3(256), 0, s, tr_levels_.as<uint32_t>(), n, d_root);
    CDA_TRY(launched("merkle levels"));
    CDA_TRY(d2h(out, d_root, 32, s, "D2H"));
    return sync(s);
}

}  // namespace cda
