// proof.hip -- device-resident extended squares: NMT share-inclusion proofs
// and blob commitments from cached row-tree nodes.
//
// Reference: pkg/proof/proof.go:77-206 (NewShareInclusionProofFromEDS,
// CreateShareToRowRootProofs -> nmt ProveRange, merkle.ProofsFromByteSlices
// over rowRoots || colRoots) and pkg/inclusion/{nmt_caching.go,
// get_commit.go, paths.go} (EDSSubTreeRootCacher: every inner node of every
// row tree kept so GetCommitment can walk to the subtree roots).
//
// The reference re-hashes whole rows on the CPU for every proof.  Here the
// square is extended once and EVERYTHING the proofs read stays in HBM:
//   leaf slots      [W][W][96]            (level 0 of every row tree)
//   row levels      level L: [W][W >> L][96]
//   column levels   level L >= 1: [W columns][W >> L][96] (sample.hip: column-axis proofs)
//   RFC levels      data-root tree over the 2W roots: level l: [2W >> l][32]
// Share-range proofs and samples are then served by one launch each, whose
// kernels do the index arithmetic themselves (share_proofs.hip: the one
// producer of share-range proofs, for one range or many; sample.hip).  What is
// left here: building the square, reading it back, and the subtree roots and
// blob commitments, which are index arithmetic on the host plus one gather
// launch.
#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/cda.h"
#include "engine.h"
#include "out_regions.h"
#include "resident_proof_dev.h"
#include "sha256_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

// All RFC-6962 levels of the data-root tree (n leaf digests, n a power of two)
// in one workgroup: level 0 = the leaf digests, level l has n >> l entries.
// One workgroup per square (blockIdx.x): square y's levels at lv + y * lv_sq
// words, its root at root + 32 y.  kFromSlots (sets of squares, square_set.hip):
// the workgroup first hashes level 0 itself from the square's n root slots at
// slots + y * slots_sq bytes, so a whole set's trees are one launch; otherwise
// level 0 is there already (launch_rfc_leaves).  A level is read back from
// global memory by other threads of the workgroup after the barrier.
template <bool kFromSlots>
__global__ __launch_bounds__(kFromSlots ? 256 : 1024) void rfc_levels_kernel(
    uint32_t* __restrict__ lv, uint64_t lv_sq, uint32_t n, uint8_t* __restrict__ root,
    const uint8_t* __restrict__ slots, uint64_t slots_sq) {
    const uint64_t sq = blockIdx.x;
    uint32_t* src = lv + sq * lv_sq;
    root += sq * 32;
    if constexpr (kFromSlots) {
        const uint8_t* in = slots + sq * slots_sq;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            uint32_t I[kSlotWords], D[8];
            load_slot_be(in + (uint64_t)i * kSlot, I);
            rfc_leaf_u<false>(I, D, false);
#pragma unroll
            for (int j = 0; j < 8; j++) src[8 * i + j] = D[j];
        }
        __syncthreads();
    }
    for (uint32_t m = n / 2; m >= 1; m >>= 1) {
        uint32_t* dst = src + 2 * m * 8;
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) {
            uint32_t A[8], B[8], D[8];
#pragma unroll
            for (int j = 0; j < 8; j++) { A[j] = src[16 * i + j]; B[j] = src[16 * i + 8 + j]; }
            rfc_inner_plain(A, B, D);
#pragma unroll
            for (int j = 0; j < 8; j++) dst[8 * i + j] = D[j];
        }
        __syncthreads();
        src = dst;
    }
    if (threadIdx.x < 8) reinterpret_cast<uint32_t*>(root)[threadIdx.x] = bswap32(src[threadIdx.x]);
}

// Copies of (src, len) pieces into one output buffer (8-byte aligned): one wavefront per piece, source and
// destination at any byte offset.  A lane owns one aligned 8-byte window of the output per pass: it reads the
// three aligned source words that hold the window's bytes (only those that hold a byte of the piece, so nothing
// is read outside the aligned words of [src, src + len)), realigns them with v_alignbyte and stores the window
// whole when it lies inside the piece, byte by byte at the piece's two ends.  Every output byte is written by
// exactly one lane and no window is read back: a neighbouring piece owns the rest of an edge window.
__global__ __launch_bounds__(256) void gather_kernel(const GatherPiece* __restrict__ pieces, uint32_t n_pieces,
                                                     uint8_t* __restrict__ out) {
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_pieces) return;
    const GatherPiece p = pieces[g];
    const uint32_t lane = threadIdx.x & 63;
    const int32_t len = (int32_t)p.len, lead = (int32_t)(p.dst & 7);
    for (int32_t rel = 8 * (int32_t)lane - lead; rel < len; rel += 8 * 64) {   // the window holds piece bytes [rel, rel + 8)
        const int32_t first = rel < 0 ? -rel : 0, last = min(8, len - rel);     // its valid bytes [first, last)
        const uintptr_t s = reinterpret_cast<uintptr_t>(p.src) + rel;           // rel < 0: only bytes >= first are used
        const uint32_t sh = (uint32_t)(s & 3);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s - sh);
        // source word j holds window bytes [4j - sh, 4j - sh + 4)
        uint32_t x[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int32_t lo = 4 * j - (int32_t)sh;
            x[j] = (lo < last && lo + 4 > first) ? q[j] : 0u;
        }
        const uint32_t w0 = __builtin_amdgcn_alignbyte(x[1], x[0], sh), w1 = __builtin_amdgcn_alignbyte(x[2], x[1], sh);
        uint8_t* win = out + (p.dst - lead) + (rel + lead);
        if (first == 0 && last == 8) {
            *reinterpret_cast<uint2*>(win) = make_uint2(w0, w1);
        } else {
            const uint64_t w = (uint64_t)w1 << 32 | w0;
            for (int32_t b = first; b < last; b++) win[b] = (uint8_t)(w >> (8 * b));
        }
    }
}

}  // namespace

hipError_t launch_rfc_levels_set(const uint8_t* root_slots, uint64_t slots_sq, uint32_t n_items, uint32_t n_squares,
                                 uint32_t* rfc, uint64_t rfc_sq_words, uint8_t* data_roots, hipStream_t s) {
    hipLaunchKernelGGL(rfc_levels_kernel<true>, dim3(n_squares), dim3(256), 0, s, rfc, rfc_sq_words, n_items,
                       data_roots, root_slots, slots_sq);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// ResidentSquare
// ---------------------------------------------------------------------------
ResidentSquare::~ResidentSquare() {
    if (borrowed)   // the set's arenas outlive the member: only the per-call buffers are its own
        for (DevBuf* b : {&eds, &levels, &col_levels, &roots_slots, &rfc, &rows, &cols, &root, &err}) *b = DevBuf{};
    for (DevBuf* b : {&eds, &levels, &col_levels, &roots_slots, &rfc, &rows, &cols, &root, &err, &scratch, &pieces})
        b->release();
}

uint64_t ResidentSquare::level_offset(uint32_t L) const {   // bytes into `levels`
    return cda::level_offset(2 * k, L, 0, kSlot);
}

uint64_t ResidentSquare::col_level_offset(uint32_t L) const {   // bytes into `col_levels`, L >= 1
    return cda::level_offset(2 * k, L, 1, kSlot);
}

ResidentView ResidentSquare::view() const {
    return ResidentView{eds.as<uint8_t>(), levels.as<uint8_t>(), col_levels.as<uint8_t>(), roots_slots.as<uint8_t>(),
                        rfc.as<uint32_t>(), k, log_w};
}

int Engine::square_create(const uint8_t* ods, uint32_t k, ResidentSquare* sq) {
    CDA_TRY(check_width(k));
    const uint32_t W = 2 * k, logW = ceil_log2(W);
    sq->k = k;
    sq->log_w = logW;
    const size_t ods_b = (size_t)k * k * kShare, eds_b = (size_t)W * W * kShare;
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->eds, eds_b, "hipMalloc"));
    CDA_TRY(ensure(sq->levels, sq->level_offset(logW + 1), "hipMalloc"));
    CDA_TRY(ensure(sq->col_levels, sq->col_level_offset(logW + 1), "hipMalloc"));
    CDA_TRY(ensure(sq->roots_slots, (size_t)2 * W * kSlot, "hipMalloc"));
    CDA_TRY(ensure(sq->rfc, (size_t)2 * (2 * W) * 32, "hipMalloc"));
    CDA_TRY(ensure(sq->rows, (size_t)W * kNode, "hipMalloc"));
    CDA_TRY(ensure(sq->cols, (size_t)W * kNode, "hipMalloc"));
    CDA_TRY(ensure(sq->root, 32, "hipMalloc"));
    CDA_TRY(ensure(sq->err, 4, "hipMalloc"));
    CDA_TRY(ensure(h_ods_, ods_b, "hipMalloc"));
    CDA_TRY(h2d(h_ods_.ptr, ods, ods_b, s, "H2D"));
    CDA_TRY(enqueue_extend(h_ods_.as<uint8_t>(), k, 1, sq->eds.as<uint8_t>(), s));
    CDA_TRY(fill(sq->err.ptr, 0xFF, 4, s, "hipMemsetAsync"));
    uint8_t* lv = sq->levels.as<uint8_t>();
    const CellGrid g{sq->eds.as<uint8_t>(), 0, W, W, W, 0, 0, k};
    CDA_TRY(check(launch_leaves(g, 1, lv, sq->err.as<uint32_t>(), true, true, s), "leaf hashing"));
    // both forests: every level retained (the columns' for the column-axis sample proofs, sample.hip)
    Forest f[2]{};
    f[0] = Forest{lv, 0, W, W, 1, nullptr, 0, sq->rows.as<uint8_t>(), 0, sq->roots_slots.as<uint8_t>(), 0, 0};
    f[1] = Forest{lv, 0, W, 1, W, nullptr, 0, sq->cols.as<uint8_t>(), 0, sq->roots_slots.as<uint8_t>(), 0, W};
    uint32_t L = 1;
    for (uint32_t m = W; m >= 2; m /= 2, L++) {
        f[0].out = lv + sq->level_offset(L);
        f[1].out = sq->col_levels.as<uint8_t>() + sq->col_level_offset(L);
        CDA_TRY(check(launch_level(f, 2, m, 1, s), "nmt level"));
        for (int i = 0; i < 2; i++) {
            f[i].in = f[i].out;
            f[i].tree_stride = m / 2;
            f[i].node_stride = 1;
        }
    }
    // data root with every RFC-6962 level kept: leaf digests, then one workgroup
    CDA_TRY(check(launch_rfc_leaves(sq->roots_slots.as<uint8_t>(), 2 * W, sq->rfc.as<uint32_t>(), s), "rfc leaves"));
    hipLaunchKernelGGL(rfc_levels_kernel<false>, dim3(1), dim3(1024), 0, s, sq->rfc.as<uint32_t>(), uint64_t{0}, 2 * W,
                       sq->root.as<uint8_t>(), static_cast<const uint8_t*>(nullptr), uint64_t{0});
    CDA_TRY(launched("rfc levels"));
    CDA_TRY(read_push_order(sq->err.ptr, 1, &sq->push_err, s));
    return push_order_error(&sq->push_err, 1, ods, k, false);
}

int Engine::square_read(ResidentSquare* sq, ResidentSquare::Part part, uint8_t* out) {
    const uint64_t W = 2ull * sq->k;
    const DevBuf* b = part == ResidentSquare::kRowRoots  ? &sq->rows
                      : part == ResidentSquare::kColRoots ? &sq->cols
                      : part == ResidentSquare::kDataRoot ? &sq->root
                                                          : &sq->eds;
    const size_t len = part == ResidentSquare::kDataRoot ? 32 : part == ResidentSquare::kEds ? W * W * kShare : W * kNode;
    CDA_TRY(d2h(out, b->ptr, len, stream_, "D2H"));
    return sync(stream_);
}

int Engine::square_gather(ResidentSquare* sq, const std::vector<GatherPiece>& pieces, uint8_t* out, size_t out_len) {
    CDA_TRY(square_gather_device(sq, pieces, out_len));
    hipStream_t s = stream_;
    CDA_TRY(d2h(out, sq->scratch.ptr, out_len, s, "D2H"));
    return sync(s);
}

int Engine::square_gather_device(ResidentSquare* sq, const std::vector<GatherPiece>& pieces, size_t out_len,
                                 bool wait) {
    hipStream_t s = stream_;
    CDA_TRY(ensure(sq->scratch, out_len ? out_len : 1, "hipMalloc"));
    if (pieces.empty()) return CDA_OK;
    CDA_TRY(ensure(sq->pieces, pieces.size() * sizeof(GatherPiece), "hipMalloc"));
    CDA_TRY(h2d(sq->pieces.ptr, pieces.data(), pieces.size() * sizeof(GatherPiece), s, "H2D pieces"));
    hipLaunchKernelGGL(gather_kernel, dim3(((uint32_t)pieces.size() + 3) / 4), dim3(256), 0, s,
                       sq->pieces.as<GatherPiece>(), (uint32_t)pieces.size(), sq->scratch.as<uint8_t>());
    CDA_TRY(launched("gather"));
    // `pieces` is pageable: make sure the copy has left it before returning (wait = false: the caller
    // synchronises the stream itself before it lets go of `pieces`)
    return wait ? sync(s) : CDA_OK;
}

// The first bad coordinate of a batch of axis halves ("" if none): the text names the half and the field.
// n_squares: the members of the set or the DAHs of the verifier (squares == NULL: one square, nothing to check).
std::string axis_halves_check(uint32_t k, uint32_t n_squares, const uint32_t* squares, const uint8_t* axes,
                              const uint32_t* indexes, const uint8_t* sides, uint32_t n) {
    const uint32_t W = 2 * k;
    for (uint32_t i = 0; i < n; i++) {
        const std::string at = "half " + std::to_string(i) + ": ";
        if (squares && squares[i] >= n_squares)
            return at + "square " + std::to_string(squares[i]) + " is not below the " + std::to_string(n_squares) +
                   " squares";
        if (axes[i] > 1) return at + "axis " + std::to_string(axes[i]) + " is neither 0 (row) nor 1 (column)";
        if (indexes[i] >= W)
            return at + "index " + std::to_string(indexes[i]) + " is not below the EDS width " + std::to_string(W);
        if (sides[i] > 1) return at + "side " + std::to_string(sides[i]) + " is neither 0 (left) nor 1 (right)";
    }
    return "";
}

// Axis halves of one resident square (sq) or of the members squares[i] of a set (sq == NULL): half i is the k
// cells side * k .. side * k + k - 1 of row or column `index`, k * 512 bytes of the output.  A row half is one
// contiguous piece of the EDS, a column half k pieces of one share; one gather launch, one copy back.  The
// piece table rides behind the output in the scratch buffer.
int Engine::axis_halves(ResidentSquare* sq, ResidentSquareSet* set, const uint32_t* squares, const uint8_t* axes,
                        const uint32_t* indexes, const uint8_t* sides, uint32_t n, uint8_t* shares) {
    if (n == 0) return CDA_OK;
    if ((set && !sq && !squares) || !axes || !indexes || !sides || !shares) return fail(CDA_ERR_INVALID, "null buffer");
    const uint32_t k = sq ? sq->k : set->k, W = 2 * k;
    const std::string bad = axis_halves_check(k, sq ? 0 : set->n, sq ? nullptr : squares, axes, indexes, sides, n);
    if (!bad.empty()) return fail(CDA_ERR_INVALID, bad);
    const uint64_t half_b = (uint64_t)k * kShare;
    std::vector<GatherPiece> pieces;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* eds = sq ? sq->eds.as<uint8_t>() : set->eds.as<uint8_t>() + (uint64_t)squares[i] * set->eds_sq;
        const uint64_t first = (uint64_t)sides[i] * k, dst = i * half_b;
        if (axes[i] == 0) {
            pieces.push_back(GatherPiece{eds + ((uint64_t)indexes[i] * W + first) * kShare, dst, (uint32_t)half_b});
        } else {
            for (uint32_t j = 0; j < k; j++)
                pieces.push_back(GatherPiece{eds + ((first + j) * W + indexes[i]) * kShare, dst + (uint64_t)j * kShare,
                                             (uint32_t)kShare});
        }
    }
    const size_t out_b = (size_t)(n * half_b), table_b = pieces.size() * sizeof(GatherPiece);
    DevBuf& scratch = sq ? sq->scratch : set->scratch;
    hipStream_t s = stream_;
    CDA_TRY(ensure(scratch, out_b + table_b, "hipMalloc"));
    uint8_t* scr = scratch.as<uint8_t>();
    GatherPiece* table = reinterpret_cast<GatherPiece*>(scr + out_b);   // out_b is a multiple of 512
    CDA_TRY(h2d(table, pieces.data(), table_b, s, "H2D pieces"));
    hipLaunchKernelGGL(gather_kernel, dim3(((uint32_t)pieces.size() + 3) / 4), dim3(256), 0, s, table,
                       (uint32_t)pieces.size(), scr);
    CDA_TRY(launched("axis halves"));
    CDA_TRY(d2h(shares, scr, out_b, s, "D2H axis halves"));
    return sync(s);   // `pieces` is pageable and the output is the caller's: complete before returning
}

int Engine::regions_out(const OutRegions& out, const uint8_t* scratch, bool one_copy, hipStream_t s,
                        const char* what) {
    if (!one_copy) {
        for (const OutRegions::Region& r : out.copies()) CDA_TRY(d2h(r.host, scratch + r.off, r.bytes, s, what));
        return sync(s);
    }
    const OutRegions::Span span = out.span();
    std::vector<uint8_t> buf(span.bytes);
    if (span.bytes) CDA_TRY(d2h(buf.data(), scratch + span.off, span.bytes, s, what));
    CDA_TRY(sync(s));
    for (const OutRegions::Region& r : out.copies()) std::memcpy(r.host, buf.data() + (r.off - span.off), r.bytes);
    return CDA_OK;
}

// ---------------------------------------------------------------------------
// EDSSubTreeRootCacher.getSubTreeRoot (pkg/inclusion/nmt_caching.go:111-124,
// walk :51-78): the node of row tree `row` reached from its root by `walk`
// (0 = WalkLeft, 1 = WalkRight).  The cache holds inner nodes only, so a walk
// may end on a leaf but not continue below one.
// ---------------------------------------------------------------------------
int Engine::square_subtree_root(ResidentSquare* sq, uint32_t row, const uint8_t* walk, uint32_t walk_len,
                                uint8_t* out) {
    const uint32_t W = 2 * sq->k, logW = sq->log_w;
    if (row >= W)
        return fail(CDA_ERR_INVALID,
                    "row exceeds range of cache: max " + std::to_string(W) + " got " + std::to_string(row));
    const uint32_t d = std::min(walk_len, logW);
    uint32_t pos = 0;
    for (uint32_t i = 0; i < d; i++) pos = 2 * pos + (walk[i] ? 1u : 0u);
    const uint32_t L = logW - d;
    // the levels below the root are kept per row tree; the root itself is the row root
    const uint8_t* src = L == logW ? sq->rows.as<uint8_t>() + (uint64_t)row * kNode
                                   : sq->levels.as<uint8_t>() + sq->level_offset(L) +
                                         ((uint64_t)row * (W >> L) + pos) * kSlot;
    const GatherPiece piece{src, 0, kNode};
    CDA_TRY(square_gather(sq, {piece}, out, kNode));
    if (walk_len > logW) {   // walk(leaf, rest): the leaf is not in the cache -- Go's %v of its bytes
        std::string msg = "did not find sub tree root: [";
        for (uint32_t i = 0; i < kNode; i++) msg += (i ? " " : "") + std::to_string(out[i]);
        return fail(CDA_ERR_INVALID, msg + "]");
    }
    return CDA_OK;
}

// ---------------------------------------------------------------------------
// GetCommitment from the cached row trees (pkg/inclusion/get_commit.go,
// paths.go): subtree roots of the blob's rows, RFC-6962 over them.
// ---------------------------------------------------------------------------
namespace {

struct Coord {
    int depth, position;
};

// paths.go calculateSubTreeRootCoordinates (restated: climb from the leftmost
// leaf while the node is a left child above minDepth and its range fits).
std::vector<Coord> subtree_coords(int maxDepth, int minDepth, int start, int end) {
    std::vector<Coord> coords;
    int leafCursor = start;
    Coord node{maxDepth, start}, lastNode = node;
    int lastLeaf = leafCursor, range = 1;
    auto reset = [&]() {
        lastNode = node;
        lastLeaf = leafCursor;
        node = Coord{maxDepth, leafCursor};
        range = 1;
    };
    for (;;) {
        if (leafCursor + 1 == end) {
            coords.push_back(node);
            return coords;
        } else if (leafCursor + 1 > end) {
            coords.push_back(lastNode);
            leafCursor = lastLeaf + 1;
            reset();
        } else if (!(node.position % 2 == 0 && node.depth > minDepth)) {
            coords.push_back(node);
            leafCursor++;
            reset();
        } else {
            lastLeaf = leafCursor;
            lastNode = node;
            leafCursor += range;
            range *= 2;
            node = Coord{node.depth - 1, node.position / 2};
        }
    }
}

}  // namespace

int Engine::square_blob_commitments(ResidentSquare* sq, const uint32_t* starts, const uint32_t* lens, uint32_t n,
                                    uint32_t threshold, uint8_t* out) {
    if (n == 0) return CDA_OK;
    if (threshold == 0) return fail(CDA_ERR_INVALID, "subtree root threshold must be positive");
    const uint32_t k = sq->k, W = 2 * k;
    const int maxDepth = (int)ceil_log2(k);
    std::vector<GatherPiece> pieces;
    std::vector<uint32_t> bt{0};
    uint32_t max_n = 0;
    for (uint32_t b = 0; b < n; b++) {
        const uint64_t len = lens[b];
        if (len == 0 || starts[b] + len > (uint64_t)k * k)
            return fail(CDA_ERR_INVALID, "cannot get commitment for blob that doesn't fit in square");
        const uint32_t w = square::subtree_width((uint32_t)len, threshold);
        const uint64_t start = (starts[b] + w - 1) / w * w;   // inclusion.NextShareIndex
        if (start + len > (uint64_t)k * k)
            return fail(CDA_ERR_INVALID, "cannot get commitment for blob that doesn't fit in square");
        const uint32_t startRow = (uint32_t)(start / k), endRow = (uint32_t)((start + len - 1) / k);
        const int nsi = (int)(start % k), nei = (int)(start + len - (uint64_t)endRow * k);
        const int minDepth = maxDepth - (int)ceil_log2(w);
        uint32_t cnt = 0;
        for (uint32_t r = startRow; r <= endRow; r++) {
            const int s0 = r == startRow ? nsi : 0, e0 = r == endRow ? nei : (int)k;
            for (const Coord& c : subtree_coords(maxDepth, minDepth, s0, e0)) {
                // depth d of the ODS half of the row tree = level maxDepth - d of the full row tree
                const uint32_t L = (uint32_t)(maxDepth - c.depth);
                const uint64_t src = sq->level_offset(L) + ((uint64_t)r * (W >> L) + (uint32_t)c.position) * kSlot;
                pieces.push_back(GatherPiece{sq->levels.as<uint8_t>() + src, (uint64_t)pieces.size() * kSlot, kSlot});
                cnt++;
            }
        }
        bt.push_back(bt.back() + cnt);
        max_n = std::max(max_n, cnt);
    }
    const uint32_t n_slots = bt.back();
    CDA_TRY(square_gather_device(sq, pieces, (size_t)n_slots * kSlot));
    hipStream_t s = stream_;
    CDA_TRY(ensure(cm_roots_, (size_t)n_slots * 32 + 32, "hipMalloc"));
    CDA_TRY(ensure(cm_plan_, bt.size() * 4, "hipMalloc"));
    CDA_TRY(ensure(cm_out_, (size_t)n * 32, "hipMalloc"));
    CDA_TRY(h2d(cm_plan_.ptr, bt.data(), bt.size() * 4, s, "H2D"));
    CDA_TRY(check(launch_slot_merkle_roots(sq->scratch.as<uint8_t>(), cm_plan_.as<uint32_t>(), n, n_slots, max_n,
            cm_roots_.as<uint32_t>(), cm_out_.as<uint8_t>(), s), "commitment roots"));
    CDA_TRY(d2h(out, cm_out_.ptr, (size_t)n * 32, s, "D2H"));
    return sync(s);
}

}  // namespace cda
