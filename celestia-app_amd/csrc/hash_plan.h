// hash_plan.h -- the launch schedule of the hashing half of cda_extend_dah*
// (leaves, NMT levels, tree top, data root) as pure host functions of
// (k, n, knob values).  No HIP include: engine.hip and nmt.hip call these
// functions for every decision they take, and tools/hash_plan_host_test.cpp
// prints the same decisions for tests/test_hash_schedules.py (g++ -I csrc,
// like tree_index.h and split_layout.h).
//
// The knob values are read where they always were (knobs.h: the test build
// only) and passed in; the defaults below are the product constants.  A
// threshold changed here changes which kernels a batch runs: the coverage
// test of tests/test_hash_schedules.py then names the (k, n) row its SWEEP
// table needs.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

namespace cda {

// nmt.hip's launch constants (the kernels are written against them).
constexpr uint32_t kTopThreads = 128;   // parents per workgroup: tpw = 256 / n_in trees x n_in / 2
constexpr uint32_t kPairMaxParents = 128;
constexpr uint32_t kPairMaxParentsSmall = 256;
constexpr uint32_t kPairSmallSquares = 8;   // launches of <= this many squares
constexpr uint32_t kPlanSlot = 96;          // device node slot (bytes): sha256_dev.h kSlot
constexpr uint32_t kPlanMaxHashParts = 4;   // Engine::kMaxHashParts

// Values of the A/B knobs the schedule depends on.
struct HashKnobs {
    int top_fuse = -1;               // CDA_TOP_FUSE: -1 auto, 0 off, N = nodes per tree
    int top_wide = 2;                // CDA_TOP_WIDE
    int subtree_min = 8;             // CDA_SUBTREE
    uint64_t subtree_lanes = 0;      // CDA_SUBTREE_LANES (0 = by tree size)
    int hash_split = -1;             // CDA_HASH_SPLIT (-1 auto)
    uint64_t leaf_pair_max = 32768;  // CDA_LEAF_PAIR_MAX
    bool pair = true;                // CDA_TOP_PAIR
    bool dr_helpers = true;          // CDA_DR_HELPERS
    bool top_helpers = true;         // CDA_TOP_HELPERS
    bool top_rfc = true;             // CDA_TOP_RFC
    uint32_t hash_wg_cap = 0;        // CDA_HASH_WG_PER_CU x CUs (0 = a workgroup per block)
    int rs8_one = -1;                // CDA_RS8_ONE (-1 auto)
    bool rs8_byteform = false;       // CDA_RS8_BYTEFORM
};

// Nodes per tree at which the NMT levels switch from one wide launch per level
// to tree_top_kernel (0 = never): the first level whose parents, over all 2W
// trees of the n squares, fill less than one wave per SIMD of the chip
// (1024 SIMDs x 64 lanes) -- lane pairs from there -- and then up to
// top_wide (CDA_TOP_WIDE) levels more, while the lane pairs of the level
// below the first fit in two waves per SIMD: the first of them runs a thread
// per parent inside the tree top (*wide), which saves their per-level
// launches (drain tail + boundary each).  CDA_TOP_FUSE=0 disables, =N forces
// N (not wide).
inline uint32_t top_fuse_nodes(uint32_t W, uint32_t n, int top_fuse, int top_wide, bool pair_sha, bool* wide) {
    if (wide) *wide = false;
    if (top_fuse >= 0) return (uint32_t)top_fuse <= W && top_fuse <= 256 ? (uint32_t)top_fuse : 0;
    for (uint32_t m = W; m >= 2; m /= 2) {
        if ((uint64_t)n * 2 * W * (m / 2) >= 65536) continue;
        if (m > 256) return 0;
        uint32_t t = m;
        // the wide first level runs lane pairs above it: none without pairs
        // (a one-thread-per-parent top holds at most 256 nodes)
        const int widen = pair_sha ? top_wide : 0;
        for (int e = 0; e < widen && 2 * t <= W && 2 * t <= 512 && 2 * t >= 8 &&
                        2 * (uint64_t)n * 2 * W * (t / 2) <= 131072;
             e++)
            t *= 2;
        if (wide) *wide = t > m;
        return t;
    }
    return 0;
}

// run_forests' fused subtree launch: the node count `sub` its lanes stop at,
// or 0 for per-level launches only.  A lane per (n_in / sub)-leaf subtree, sub
// the smallest node count >= stop at which the launch holds `want` lanes
// (default 524288, or 262144 for trees of >= 1024 leaves); subtrees keep >=
// max(subtree_min, 4) leaves; a batch too small to reach the target still
// takes the fused launch when it holds 131072 lanes.  Roots and per-lane
// stacks need n_trees * sub * log2(n_in / sub) slots of each forest's output
// region (`room` bytes), and the kernel's 64-tree tiles whole forests.
inline uint32_t subtree_sub(uint32_t n_in, uint32_t stop, uint32_t n, const uint32_t* n_trees, uint32_t n_forest,
                            uint64_t room, int subtree_min, uint64_t subtree_lanes) {
    if (!(subtree_min > 0 && stop >= 1 && n_in % stop == 0)) return 0;
    uint64_t per_node = 0;   // lanes per subtree root per tree
    for (uint32_t i = 0; i < n_forest; i++) per_node += (uint64_t)n * n_trees[i];
    uint32_t sub = stop;
    const uint64_t want = subtree_lanes ? subtree_lanes : n_in >= 1024 ? 262144u : 524288u;
    // launch_subtrees needs subtrees of >= 4 leaves: a smaller CDA_SUBTREE
    // setting means per-level launches, not a failing launch
    const uint32_t min_leaves = (uint32_t)std::max(subtree_min, 4);
    while (sub < n_in && 2 * (uint64_t)sub * min_leaves <= n_in && per_node * sub < want) sub *= 2;
    bool fits = per_node * sub >= std::min<uint64_t>(want, 131072) && sub < n_in && n_in / sub >= min_leaves;
    const uint32_t slog = fits ? (uint32_t)__builtin_ctz(n_in / sub) : 0;
    for (uint32_t i = 0; i < n_forest && fits; i++) {
        const uint64_t need = (uint64_t)n_trees[i] * sub * slog * kPlanSlot;
        fits = need <= room && n_trees[i] % 64 == 0;
    }
    return fits ? sub : 0;
}

// enqueue_dah's hash split: parts of the batch that hash on their own streams
// (auto: two below 64 squares of k <= 128, one otherwise; one while profiling).
inline uint32_t hash_parts(uint32_t k, uint32_t n, int hash_split, bool profiling = false) {
    const uint32_t want = hash_split >= 0 ? (uint32_t)hash_split : (n < 64 && k <= 128 ? 2u : 1u);
    const uint32_t parts = std::min<uint32_t>(std::min<uint32_t>(want, n), kPlanMaxHashParts);
    return parts > 1 && !profiling ? parts : 1;
}
// part p: squares [p n / parts, (p + 1) n / parts)
inline uint32_t hash_part_begin(uint32_t p, uint32_t n, uint32_t parts) { return p * n / parts; }

// dah_finish's tree top for a part of m squares whose levels ran down to
// `from` nodes per tree: the part's own top_fuse_nodes, clamped to `from`.
struct TopChoice {
    uint32_t top;
    bool wide;
};
inline TopChoice finish_top(uint32_t W, uint32_t m, uint32_t from, int top_fuse, int top_wide, bool pair_sha) {
    bool wide = false;
    uint32_t top = from > 1 ? top_fuse_nodes(W, m, top_fuse, top_wide, pair_sha, &wide) : 0;
    if (top > from) {
        top = from;
        wide = false;
    }
    return TopChoice{top, wide};
}

// launch_leaves: the lane-pair leaf kernel up to leaf_pair_max cells per launch.
inline bool leaves_pair(uint64_t cells, uint64_t leaf_pair_max, bool pair_sha) {
    return cells > 0 && cells <= leaf_pair_max && pair_sha;
}

// Workgroups of a leaf / level launch over `nblocks` virtual blocks: all of
// them, or `cap` persistent ones (CDA_HASH_WG_PER_CU x the device's CUs).
inline uint32_t hash_grid_for(uint32_t nblocks, uint32_t cap) { return cap && nblocks > cap ? cap : nblocks; }

// launch_tree_top.
struct TopLaunch {
    bool valid;
    bool wide;      // first level a thread per parent
    uint32_t tpw;   // trees per workgroup
    uint32_t lv;    // RFC-6962 levels inside the workgroups
    uint32_t n_dig; // digests per square left for the data root
    bool pair;      // tree_top_kernel<true>
    uint32_t grid_x;
    bool ragged;    // the last workgroup holds fewer than tpw trees
};
inline TopLaunch tree_top_launch(uint32_t n_in, uint32_t n, uint32_t trees, uint32_t n_items, bool has_dig, bool wide,
                                 bool pair_sha, bool rfc_in_top) {
    TopLaunch t{};
    wide = wide && pair_sha;
    t.wide = wide;
    if (n_in < (wide ? 8u : 2u) || n_in > (wide ? 4 : 2) * kTopThreads || (n_in & (n_in - 1))) return t;
    t.valid = true;
    const uint32_t tpw = (wide ? 4 : 2) * kTopThreads / n_in;   // trees per workgroup
    // RFC-6962 levels inside the workgroups: while every workgroup holds tpw
    // of the n_items (a power of two) roots and at least 2 digests per square
    // remain for data_root_digest_kernel
    uint32_t lv = 0;
    if (has_dig && trees == n_items && (n_items & (n_items - 1)) == 0 && tpw <= n_items)
        while ((2u << lv) <= tpw && (n_items >> (lv + 1)) >= 2) lv++;
    if (!rfc_in_top) lv = 0;   // CDA_TOP_RFC=0: leaf digests only (A/B knob)
    t.tpw = tpw;
    t.lv = lv;
    t.n_dig = n_items >> lv;
    // lane pairs while they still fit in a wave per SIMD (1024 SIMDs); wide:
    // the caller's choice (a thread per parent in the first level)
    const uint64_t parents = (uint64_t)n * trees * (n_in / 2);
    t.pair = wide || (pair_sha && 2 * parents <= 65536);
    t.grid_x = (trees + tpw - 1) / tpw;
    t.ragged = trees % tpw != 0;
    return t;
}

// launch_data_root_digests.
struct DataRootLaunch {
    uint32_t pmax;     // the largest lane-pair level
    uint32_t threads;
    uint32_t mode;     // 0 a thread per parent, 1 lane pairs, 2 lane pairs + schedule helpers
    uint64_t lds;
};
inline uint32_t data_root_mode_for(bool pair_sha, bool dr_helpers) { return pair_sha ? (dr_helpers ? 2u : 1u) : 0u; }
inline DataRootLaunch data_root_launch(uint32_t n_items, uint32_t n, uint32_t mode) {
    DataRootLaunch d{};
    d.lds = (uint64_t)(n_items / 2 + n_items / 4) * 32;
    // a thread per first-level parent (<= 512: more would cap the kernel at
    // 128 VGPRs and spill the helpers' registers), and room for the lane pairs
    const uint32_t pmax = n <= kPairSmallSquares ? kPairMaxParentsSmall : kPairMaxParents;
    uint32_t threads = std::min<uint32_t>(n_items / 2, 512);
    threads = std::max<uint32_t>(threads, std::min<uint32_t>(n_items, 2 * pmax));
    threads = std::max<uint32_t>((threads + 63) / 64 * 64, 64);
    d.pmax = pmax;
    d.threads = threads;
    d.mode = mode;
    return d;
}

// The k = 128 RS launches (rs_gf8.hip / rs_gf8_bs.hip): the bitsliced encoder
// unless a segment is not a multiple of its 4-codeword workgroup or
// CDA_RS8_BYTEFORM=1; one codeword per workgroup for a job that cannot fill
// the chip with two (fewer than 2 per CU), CDA_RS8_ONE=0/1 forces either.
inline bool rs8_bitsliced(uint32_t k, bool byteform, uint32_t ncw0, uint32_t ncw1) {
    return k == 128 && !byteform && ncw0 % 4 == 0 && ncw1 % 4 == 0;
}
inline bool rs8_one_per_wg(uint32_t ncw, uint32_t n, int one_env) {
    return one_env >= 0 ? one_env != 0 : (uint64_t)ncw * n < 2u * 256u;
}

// ---------------------------------------------------------------------------
// The launches of one part, in order, as enqueue_dah issues them (dah_chunk
// then dah_finish on the part's stream).
// ---------------------------------------------------------------------------
enum class PlanKernel : uint8_t {
    kRs8,           // k = 128 RS launch (whole batch, before the parts): sub = 1 bitsliced, pair = one per workgroup
    kLeafPair,      // leaf_pair_kernel
    kLeaf,          // leaf_kernel
    kSubtree,       // subtree_kernel: n_in -> sub nodes per tree
    kLevel,         // level_kernel: n_in -> n_in / 2
    kTreeTop,       // tree_top_kernel<pair>: n_in -> roots
    kRfcLeaf,       // rfc_leaf_kernel over the root slots (no tree top)
    kDataRoot,      // data_root_digest_kernel over n_dig digests
};

struct PlanLaunch {
    PlanKernel kernel;
    uint32_t n_in;      // nodes per tree the launch reads (leaves: W)
    uint32_t sub;       // subtree: nodes per tree it leaves; tree top: tpw
    bool wide;
    uint32_t lv;
    uint32_t n_dig;
    bool pair;
    bool ragged;
    uint32_t pmax;
    uint32_t mode;      // data root: data_root_mode; tree top: 1 with schedule helpers
    uint32_t threads;   // data root
    bool persistent;    // leaf / level: fewer workgroups than blocks (hash_grid)
    uint64_t scratch;   // subtree: bytes of its output region a forest needs
};

struct PartPlan {
    uint32_t i0, m;         // squares [i0, i0 + m) of the batch
    uint32_t stop;          // nodes per tree the whole batch's wide levels stop at
    uint64_t subtree_room;  // bytes of a forest's output region
    uint32_t count;
    PlanLaunch launch[24];
};

inline void plan_forests(PartPlan& P, uint32_t W, uint32_t n_in, uint32_t m, uint32_t stop, bool subtrees,
                         const HashKnobs& K) {
    const uint32_t n_trees[2] = {W, W};
    uint32_t m0 = n_in;
    if (subtrees) {
        const uint32_t sub = subtree_sub(n_in, stop, m, n_trees, 2, P.subtree_room, K.subtree_min, K.subtree_lanes);
        if (sub) {
            PlanLaunch L{};
            L.kernel = PlanKernel::kSubtree;
            L.n_in = n_in;
            L.sub = sub;
            L.scratch = (uint64_t)W * sub * (uint32_t)__builtin_ctz(n_in / sub) * kPlanSlot;
            P.launch[P.count++] = L;
            m0 = sub;
        }
    }
    for (uint32_t l = m0; l >= 2 && l > stop; l /= 2) {
        PlanLaunch L{};
        L.kernel = PlanKernel::kLevel;
        L.n_in = l;
        const uint32_t nbx = (W * (l / 2) + 255) / 256, nblocks = nbx * m * 2;
        L.persistent = hash_grid_for(nblocks, K.hash_wg_cap) != nblocks;
        P.launch[P.count++] = L;
    }
}

// Part p (of hash_parts(k, n)) of a batch of n squares of width k.
inline PartPlan part_plan(uint32_t k, uint32_t n, uint32_t p, const HashKnobs& K) {
    const uint32_t W = 2 * k;
    const uint32_t parts = hash_parts(k, n, K.hash_split);
    PartPlan P{};
    P.i0 = hash_part_begin(p, n, parts);
    P.m = hash_part_begin(p + 1, n, parts) - P.i0;
    P.subtree_room = (uint64_t)W * W * kPlanSlot / 2;
    const uint32_t m = P.m;
    const uint32_t top_all = top_fuse_nodes(W, n, K.top_fuse, K.top_wide, K.pair, nullptr);
    const uint32_t stop = top_all ? top_all : 1;
    P.stop = stop;
    if (k == 128) {   // the batch's two RS launches: Q0 (rows and columns of Q0: 2k codewords), Q3 (k)
        for (uint32_t ncw : {2 * k, k}) {
            PlanLaunch L{};
            L.kernel = PlanKernel::kRs8;
            L.n_in = ncw;
            L.sub = rs8_bitsliced(k, K.rs8_byteform, k, ncw == k ? 0 : k) ? 1 : 0;
            L.pair = L.sub && rs8_one_per_wg(ncw, n, K.rs8_one);
            P.launch[P.count++] = L;
        }
    }
    // dah_chunk: leaves, then the levels down to the batch's stop
    {
        PlanLaunch L{};
        const uint64_t cells = (uint64_t)W * W * m;
        L.pair = leaves_pair(cells, K.leaf_pair_max, K.pair);
        L.kernel = L.pair ? PlanKernel::kLeafPair : PlanKernel::kLeaf;
        L.n_in = W;
        const uint32_t nblocks = (W * W + 255) / 256 * m;
        L.persistent = !L.pair && hash_grid_for(nblocks, K.hash_wg_cap) != nblocks;
        P.launch[P.count++] = L;
    }
    if (W > stop) plan_forests(P, W, W, m, stop, true, K);
    // dah_finish: the part's own top, the levels down to it, the data root
    const uint32_t from = stop;
    const TopChoice tc = finish_top(W, m, from, K.top_fuse, K.top_wide, K.pair);
    uint32_t n_dig = 2 * W;
    if (from > 1) {
        const uint32_t fstop = tc.top ? tc.top : 1;
        if (from > fstop) plan_forests(P, W, from, m, fstop, false, K);
        if (tc.top) {
            const TopLaunch t = tree_top_launch(tc.top, m, 2 * W, 2 * W, true, tc.wide, K.pair, K.top_rfc);
            PlanLaunch L{};
            L.kernel = PlanKernel::kTreeTop;
            L.n_in = tc.top;
            L.sub = t.tpw;
            L.wide = t.wide;
            L.lv = t.lv;
            L.n_dig = t.n_dig;
            L.pair = t.pair;
            L.ragged = t.ragged;
            L.mode = t.pair && K.top_helpers ? 1 : 0;
            P.launch[P.count++] = L;
            n_dig = t.n_dig;
        }
    }
    if (!tc.top) {
        PlanLaunch L{};
        L.kernel = PlanKernel::kRfcLeaf;
        L.n_in = 1;
        P.launch[P.count++] = L;
    }
    {
        const DataRootLaunch d = data_root_launch(n_dig, m, data_root_mode_for(K.pair, K.dr_helpers));
        PlanLaunch L{};
        L.kernel = PlanKernel::kDataRoot;
        L.n_in = 1;
        L.n_dig = n_dig;
        L.pmax = d.pmax;
        L.mode = d.mode;
        L.threads = d.threads;
        P.launch[P.count++] = L;
    }
    return P;
}

}  // namespace cda
