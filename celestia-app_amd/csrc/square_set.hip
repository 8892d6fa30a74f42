// square_set.hip -- sets of resident squares: what Engine::square_create
// (proof.hip) keeps for one square, built for n squares of one width in one
// submission, from a batch of ODSs or of EDSs that lies on the host or already
// in HBM (the output of cda_extend_dah_device, replay, cda_repair_batch_device).
//
// Layout.  One arena per part -- EDS, row levels, column levels, root slots,
// RFC-6962 levels, packed row roots, packed column roots, data roots,
// push-order words -- and square y of an arena at base + y * stride, the stride
// being the size square_create gives the buffer of the same name.  A member
// (ResidentSquareSet::lend) is a ResidentSquare whose buffers point into the
// arenas, so every kernel that serves a single square serves a member as it
// is.  All offsets are 64-bit: the EDS arena of 130 k = 128 squares is past
// 4 GiB.
//
// Build.  RS extension (ODS sources only), leaf hashing and every tree level
// are the batch launches the DAH path uses, with n squares per launch and the
// arenas' strides as the per-square strides.  launch_leaves writes the squares'
// leaf slots back to back, while a square's leaf level lies at the head of its
// stride of the row-level arena, so the leaves go to a staging buffer and one
// strided device copy puts them in place.  The new kernel is the data-root
// tree (proof.hip rfc_levels_kernel<true>, launch_rfc_levels_set): a workgroup
// per square hashes the 2W root slots to leaf digests and keeps every RFC-6962
// level; the single square's form takes its digests from a launch of their own,
// and launch_data_root_slots keeps no level.
#include <string>

#include "../../include/cda.h"
#include "engine.h"
#include "sha256_dev.h"
#include "tree_index.h"

namespace cda {

namespace {

DevBuf view(const DevBuf& arena, uint64_t off, uint64_t bytes) {
    DevBuf b;
    b.ptr = arena.as<uint8_t>() + off;
    b.bytes = bytes;
    return b;
}

}  // namespace

ResidentSquareSet::~ResidentSquareSet() {
    for (DevBuf* b : {&eds, &levels, &col_levels, &roots_slots, &rfc, &rows, &cols, &roots, &err, &scratch}) b->release();
}

void ResidentSquareSet::lend(uint32_t i, ResidentSquare* sq) const {
    sq->k = k;
    sq->log_w = log_w;
    sq->push_err = push_err[i];
    sq->borrowed = true;
    sq->eds = view(eds, i * eds_sq, eds_sq);
    sq->levels = view(levels, i * levels_sq, levels_sq);
    sq->col_levels = view(col_levels, i * col_levels_sq, col_levels_sq);
    sq->roots_slots = view(roots_slots, i * roots_slots_sq, roots_slots_sq);
    sq->rfc = view(rfc, i * rfc_sq, rfc_sq);
    sq->rows = view(rows, i * axis_roots_sq, axis_roots_sq);
    sq->cols = view(cols, i * axis_roots_sq, axis_roots_sq);
    sq->root = view(roots, (uint64_t)i * 32, 32);
    sq->err = view(err, (uint64_t)i * 4, 4);
}

int Engine::square_set_create(const uint8_t* src, const uint8_t* d_src, int kind, uint32_t k, uint32_t n,
                              ResidentSquareSet* set, hipStream_t s) {
    set_device_batch(0);   // the last batch's words are gone once this call touches them
    const uint32_t W = 2 * k, logW = ceil_log2(W);
    const bool from_ods = kind == CDA_SET_FROM_ODS;
    set->k = k;
    set->log_w = logW;
    set->n = n;
    set->eds_sq = (uint64_t)W * W * kShare;
    set->levels_sq = level_offset(W, logW + 1, 0, kSlot);
    set->col_levels_sq = level_offset(W, logW + 1, 1, kSlot);
    set->roots_slots_sq = (uint64_t)2 * W * kSlot;
    set->rfc_sq = (uint64_t)2 * (2 * W) * 32;
    set->axis_roots_sq = (uint64_t)W * kNode;
    // the arenas live as long as the set: plain allocations, not the call stream's pool
    CDA_TRY(check(set->eds.ensure_fixed(n * set->eds_sq), "hipMalloc"));
    CDA_TRY(check(set->levels.ensure_fixed(n * set->levels_sq), "hipMalloc"));
    CDA_TRY(check(set->col_levels.ensure_fixed(n * set->col_levels_sq), "hipMalloc"));
    CDA_TRY(check(set->roots_slots.ensure_fixed(n * set->roots_slots_sq), "hipMalloc"));
    CDA_TRY(check(set->rfc.ensure_fixed(n * set->rfc_sq), "hipMalloc"));
    CDA_TRY(check(set->rows.ensure_fixed(n * set->axis_roots_sq), "hipMalloc"));
    CDA_TRY(check(set->cols.ensure_fixed(n * set->axis_roots_sq), "hipMalloc"));
    CDA_TRY(check(set->roots.ensure_fixed((uint64_t)n * 32), "hipMalloc"));
    CDA_TRY(check(set->err.ensure_fixed((uint64_t)n * 4), "hipMalloc"));
    uint8_t* eds = set->eds.as<uint8_t>();
    uint32_t* err = set->err.as<uint32_t>();
    // build scratch, back to the call stream's pool when the call's work is done: the uploaded ODS batch and
    // the contiguous leaf slots
    DevBuf up, leaf;
    struct Release {
        DevBuf &a, &b;
        ~Release() { a.release(), b.release(); }
    } release{up, leaf};
    const uint64_t src_b = from_ods ? (uint64_t)n * k * k * kShare : n * set->eds_sq;
    if (from_ods) {
        if (src) {
            CDA_TRY(ensure(up, src_b, "hipMalloc"));
            CDA_TRY(h2d(up.ptr, src, src_b, s, "H2D"));
            d_src = up.as<uint8_t>();
        }
        CDA_TRY(enqueue_extend(d_src, k, n, eds, s));
    } else if (src) {
        CDA_TRY(h2d(eds, src, src_b, s, "H2D"));
    } else {
        CDA_TRY(check(hipMemcpyAsync(eds, d_src, src_b, hipMemcpyDeviceToDevice, s), "copy"));
    }
    CDA_TRY(fill(err, 0xFF, (size_t)n * 4, s, "hipMemsetAsync"));
    const uint64_t leaf_sq = (uint64_t)W * W * kSlot;
    CDA_TRY(ensure(leaf, n * leaf_sq, "hipMalloc"));
    const CellGrid g{eds, set->eds_sq, W, W, W, 0, 0, k};
    CDA_TRY(check(launch_leaves(g, n, leaf.as<uint8_t>(), err, true, true, s), "leaf hashing"));
    uint8_t* lv = set->levels.as<uint8_t>();
    CDA_TRY(check(hipMemcpy2DAsync(lv, set->levels_sq, leaf.ptr, leaf_sq, leaf_sq, n, hipMemcpyDeviceToDevice, s),
                  "leaf slots"));
    // both forests of every square, every level retained, as square_create builds them for one
    Forest f[2]{};
    f[0] = Forest{lv, set->levels_sq, W, W, 1, nullptr, 0, set->rows.as<uint8_t>(), set->axis_roots_sq,
                  set->roots_slots.as<uint8_t>(), set->roots_slots_sq, 0};
    f[1] = Forest{lv, set->levels_sq, W, 1, W, nullptr, 0, set->cols.as<uint8_t>(), set->axis_roots_sq,
                  set->roots_slots.as<uint8_t>(), set->roots_slots_sq, W};
    uint32_t L = 1;
    for (uint32_t m = W; m >= 2; m /= 2, L++) {
        f[0].out = lv + level_offset(W, L, 0, kSlot);
        f[0].out_sq = set->levels_sq;
        f[1].out = set->col_levels.as<uint8_t>() + level_offset(W, L, 1, kSlot);
        f[1].out_sq = set->col_levels_sq;
        CDA_TRY(check(launch_level(f, 2, m, n, s), "nmt level"));
        for (int i = 0; i < 2; i++) {
            f[i].in = f[i].out;
            f[i].in_sq = f[i].out_sq;
            f[i].tree_stride = m / 2;
            f[i].node_stride = 1;
        }
    }
    CDA_TRY(check(launch_rfc_levels_set(set->roots_slots.as<uint8_t>(), set->roots_slots_sq, 2 * W, n,
                                        set->rfc.as<uint32_t>(), set->rfc_sq / 4, set->roots.as<uint8_t>(), s),
                  "rfc levels of a set"));
    // the words also as the context's last device batch (cda_push_order_detail_at)
    uint32_t* batch_words = err_words(n);
    if (!batch_words) return fail(CDA_ERR_OOM, "hipMalloc err words");
    CDA_TRY(check(hipMemcpyAsync(batch_words, err, (size_t)n * 4, hipMemcpyDeviceToDevice, s), "copy"));
    // complete on return, waiting for this call's own work only: an event, not the caller's whole stream
    set->push_err.assign(n, push_order::kOrdered);
    CDA_TRY(d2h(set->push_err.data(), err, (size_t)n * 4, s, "D2H"));
    hipEvent_t done = nullptr;
    CDA_TRY(check(hipEventCreateWithFlags(&done, hipEventDisableTiming), "hipEventCreate"));
    hipError_t e = hipEventRecord(done, s);
    if (e == hipSuccess) e = hipEventSynchronize(done);
    (void)hipEventDestroy(done);
    CDA_TRY(check(e, "hipEventSynchronize (set build)"));
    set_device_batch(n);
    // the reference's text for the first unordered square, from the two cells where they now lie
    for (uint32_t i = 0; i < n; i++) {
        const push_order::Violation v = push_order::decode(set->push_err[i]);
        if (v.axis < 0) continue;
        po_axis = v.axis;
        po_index = v.index;
        po_pos = v.pos;
        uint8_t ns[2][32];
        for (uint32_t j = 0; j < 2; j++) {
            const uint32_t pos = v.pos - 1 + j, r = v.axis == 0 ? v.index : pos, c = v.axis == 0 ? pos : v.index;
            CDA_TRY(d2h(ns[j], eds + i * set->eds_sq + ((uint64_t)r * W + c) * kShare, 32, s, "D2H"));
        }
        CDA_TRY(sync(s));
        return fail_push_order(ns[0], ns[1]);
    }
    return CDA_OK;
}

int Engine::square_set_dah(ResidentSquareSet* set, uint8_t* rows, uint8_t* cols, uint8_t* roots, int32_t* status) {
    hipStream_t s = stream_;
    const size_t axis_b = (size_t)set->n * set->axis_roots_sq;
    if (rows) CDA_TRY(d2h(rows, set->rows.ptr, axis_b, s, "D2H"));
    if (cols) CDA_TRY(d2h(cols, set->cols.ptr, axis_b, s, "D2H"));
    if (roots) CDA_TRY(d2h(roots, set->roots.ptr, (size_t)set->n * 32, s, "D2H"));
    if (status)
        for (uint32_t i = 0; i < set->n; i++)
            status[i] = set->push_err[i] == push_order::kOrdered ? CDA_OK : CDA_ERR_PUSH_ORDER;
    return sync(s);
}

}  // namespace cda
