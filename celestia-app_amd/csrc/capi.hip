// capi.hip -- extern "C" entry points of libcda.so (declared in include/cda.h).
// Each function validates arguments the way the reference does, locks the
// context and forwards to cda::Engine.  No C++ exception or abort crosses the
// ABI.
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <utility>

#include "../../include/cda.h"
#include "engine.h"
#include "commitment_proofs_plan.h"
#include "share_proofs_plan.h"
#include "split_layout.h"

struct cda_ctx {
    cda::Engine eng;
    explicit cda_ctx(int dev) : eng(dev) {}
};

struct cda_square {
    cda_ctx* ctx;
    cda::ResidentSquare sq;
    cda_square_set* owner = nullptr;   // a member of a set: borrowed, ends with the set
};

struct cda_square_set {
    cda_ctx* ctx;
    cda::ResidentSquareSet set;
    std::vector<std::unique_ptr<cda_square>> members;   // one per square, views into the set's arenas
};

namespace {

// pkg/da/data_availability_header.go SquareSize + IsPowerOfTwo; a power of
// two that is not a square (8 shares) passes ExtendShares' check and fails in
// rsmt2d's newDataSquare instead
bool square_width(uint32_t n_shares, uint32_t* k) {
    if (n_shares == 0 || (n_shares & (n_shares - 1))) return false;
    uint32_t w = 1;
    while ((uint64_t)w * w < n_shares) w <<= 1;
    if ((uint64_t)w * w != n_shares) return false;
    *k = w;
    return true;
}

// The last call's error text and push-order details, per calling thread.  The
// context's own copy is overwritten by the next call on it (from any thread),
// so cda_last_error / cda_push_order_detail read this snapshot instead.
struct ThreadError {
    std::string msg;
    int32_t axis = -1;
    uint32_t index = 0, pos = 0;
};
thread_local ThreadError tl_err;

// A context may be driven from any OS thread (Go moves goroutines between
// threads): its device becomes current for the call and the caller's device
// is restored afterwards.
struct DeviceScope {
    int prev = -1, want;
    explicit DeviceScope(int d) : want(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != d) (void)hipSetDevice(d);
    }
    ~DeviceScope() {
        if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
    }
};

// Lock the context, make its device current, order the call's GPU work after
// the previous call's (Engine::order_begin / order_end on the stream the call
// enqueues on: `stream`, or the context's private stream for host-buffer
// calls), run f and publish the error to the calling thread.
template <class F>
int guarded_on(cda_ctx* ctx, const hipStream_t* stream, F&& f) {
    if (!ctx) {
        tl_err.msg = "null context";
        return CDA_ERR_INVALID;
    }
    cda::Engine& e = ctx->eng;
    std::lock_guard<std::mutex> g(e.mutex());
    DeviceScope dev(e.device());
    e.clear_error();
    const hipStream_t s = stream ? *stream : e.stream();
    int rc;
    try {
        rc = e.order_begin(s);
        if (rc == CDA_OK) rc = f(e);
    } catch (const std::bad_alloc&) {
        rc = e.fail(CDA_ERR_OOM, "host allocation failed");
    } catch (...) {
        rc = e.fail(CDA_ERR_DEVICE, "unexpected exception");
    }
    // A failed call may have returned before joining its side streams (hash
    // split parts, RS chunks, the host pipeline's copies): wait for them here,
    // so nothing the call queued can still read a buffer that the next call
    // frees in stream order, or a host buffer the caller frees on return.
    // (Push-order results are complete answers, not failures.)
    if (rc != CDA_OK && rc != CDA_ERR_PUSH_ORDER) {
        const std::string msg = e.last_error();
        (void)e.drain_streams();
        e.fail(rc, msg);   // keep the call's own error text
    }
    e.order_end(s);
    tl_err.msg = e.last_error();
    if (rc == CDA_ERR_PUSH_ORDER) {
        tl_err.axis = e.po_axis;
        tl_err.index = e.po_index;
        tl_err.pos = e.po_pos;
    }
    return rc;
}

template <class F>
int guarded(cda_ctx* ctx, F&& f) {
    return guarded_on(ctx, nullptr, std::forward<F>(f));
}

// Device entry points enqueue on the caller's stream (NULL = HIP's default).
template <class F>
int guarded_stream(cda_ctx* ctx, void* stream, F&& f) {
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return guarded_on(ctx, &s, [&](cda::Engine& e) { return f(e, s); });
}

// The error of a share count square_width rejects: ExtendShares' own
// (data_availability_header.go:67-69), or rsmt2d's for a power of two that is
// not a square (newDataSquare, EXT v0.14.0).
int not_pow2(cda::Engine& e, uint32_t n) {
    if (n && !(n & (n - 1))) return e.fail(CDA_ERR_INVALID, "number of chunks must be a square number");
    char buf[96];
    snprintf(buf, sizeof buf, "number of shares is not a power of 2: got %u", n);
    return e.fail(CDA_ERR_NOT_POW2, buf);
}

// The widest square the library extends (Engine::check_width).  The host
// entry points say so before they stage a byte of a wider one.
int too_wide(cda::Engine& e) { return e.fail(CDA_ERR_INVALID, "square width must be a power of two <= 1024"); }

int plan_square(const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs, uint32_t max_square_size,
                uint32_t threshold, int mode, cda::square::Plan* p, std::string* err) {
    if (mode != CDA_SQUARE_CONSTRUCT && mode != CDA_SQUARE_BUILD) {
        *err = "unknown square construction mode";
        return -1;
    }
    for (uint32_t i = 0; i < n_txs; i++)
        if (tx_off[i + 1] < tx_off[i]) {
            *err = "tx offsets must be non-decreasing";
            return -1;
        }
    return cda::square::plan(txs, tx_off, n_txs, max_square_size, threshold,
                             mode == CDA_SQUARE_BUILD ? cda::square::kBuild : cda::square::kConstruct, p, err);
}

// The plan's kept transaction indexes into the caller's optional outputs.
void copy_kept(const cda::square::Plan& p, uint32_t* kept, uint32_t* n_kept) {
    if (!kept) return;
    memcpy(kept, p.kept.data(), p.kept.size() * 4);
    if (n_kept) *n_kept = (uint32_t)p.kept.size();
}

// A host-only entry point (no device work), usable without a context:
// run(&err) returns a CDA_* code and the error text.
template <class F>
int host_only(cda_ctx* ctx, F&& run) {
    if (!ctx) {
        tl_err.msg.clear();
        try {
            return run(&tl_err.msg);
        } catch (const std::bad_alloc&) {
            tl_err.msg = "host allocation failed";
            return CDA_ERR_OOM;
        }
    }
    return guarded(ctx, [&](cda::Engine& e) -> int {
        std::string err;
        const int rc = run(&err);
        return rc ? e.fail(rc, err) : CDA_OK;
    });
}

}  // namespace

extern "C" {

const char* cda_version(void) { return cda::kTestBuild ? "cda 0.1.0 gfx950 test-build" : "cda 0.1.0 gfx950"; }

int cda_ctx_create(int device, cda_ctx** out) {
    if (!out) return CDA_ERR_INVALID;
    *out = nullptr;
    cda_ctx* c = new (std::nothrow) cda_ctx(device);
    if (!c) return CDA_ERR_OOM;
    int rc = c->eng.init();
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return CDA_OK;
}

int cda_ctx_destroy(cda_ctx* ctx) {
    delete ctx;
    return CDA_OK;
}

const char* cda_last_error(cda_ctx* ctx) {
    (void)ctx;   // per calling thread: the message of this thread's last call (include/cda.h)
    return tl_err.msg.c_str();
}

int cda_extend_shares(cda_ctx* ctx, const uint8_t* ods, uint32_t n_shares, uint8_t* eds) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        uint32_t k;
        if (!square_width(n_shares, &k)) return not_pow2(e, n_shares);
        if (k > 1024) return too_wide(e);
        if (!ods || !eds) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_extend(ods, k, eds);
    });
}

int cda_dah_from_eds(cda_ctx* ctx, const uint8_t* eds, uint32_t w, uint8_t* row_roots, uint8_t* col_roots,
                     uint8_t* data_root) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (w < 2 || (w & (w - 1))) return e.fail(CDA_ERR_INVALID, "EDS width must be a power of two >= 2");
        if (w > 2048) return too_wide(e);
        if (!eds || !row_roots || !col_roots || !data_root) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_dah(eds, w / 2, row_roots, col_roots, data_root);
    });
}

int cda_extend_dah(cda_ctx* ctx, const uint8_t* ods, uint32_t n_shares, uint8_t* eds, uint8_t* row_roots,
                   uint8_t* col_roots, uint8_t* data_root) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        uint32_t k;
        if (!square_width(n_shares, &k)) return not_pow2(e, n_shares);
        if (k > 1024) return too_wide(e);
        if (!ods || !row_roots || !col_roots || !data_root) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_extend_dah(ods, k, 1, eds, row_roots, col_roots, data_root, nullptr);
    });
}

int cda_extend_dah_batch(cda_ctx* ctx, const uint8_t* ods, uint32_t k, uint32_t n, uint8_t* eds, uint8_t* row_roots,
                         uint8_t* col_roots, uint8_t* data_roots, int32_t* status) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (k == 0 || (k & (k - 1))) return not_pow2(e, k * k);
        if (k > 1024) return too_wide(e);
        if (n == 0) return CDA_OK;
        if (!ods || !row_roots || !col_roots || !data_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_extend_dah(ods, k, n, eds, row_roots, col_roots, data_roots, status);
    });
}

int cda_extend_dah_batch_ex(cda_ctx* ctx, const uint8_t* ods, uint32_t k, uint32_t n, uint8_t* eds, int eds_mode,
                            uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots, int32_t* status) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (k == 0 || (k & (k - 1))) return not_pow2(e, k * k);
        if (k > 1024) return too_wide(e);
        if (eds_mode != CDA_EDS_FULL && eds_mode != CDA_EDS_SKIP_Q0 && eds_mode != CDA_EDS_PARITY)
            return e.fail(CDA_ERR_INVALID, "unknown eds_mode");
        if (n == 0) return CDA_OK;
        if (!ods || !row_roots || !col_roots || !data_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_extend_dah(ods, k, n, eds, row_roots, col_roots, data_roots, status, eds_mode);
    });
}

int cda_extend_dah_device(cda_ctx* ctx, const void* d_ods, uint32_t k, uint32_t n, void* d_eds, void* d_row_roots,
                          void* d_col_roots, void* d_data_roots, int32_t* d_status, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (k == 0 || (k & (k - 1))) return not_pow2(e, k * k);
        if (n == 0) return CDA_OK;
        if (!d_ods || !d_eds || !d_row_roots || !d_col_roots || !d_data_roots)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        uint32_t* err = e.err_words(n);
        if (!err) return e.fail(CDA_ERR_OOM, "hipMalloc err words");
        const int rc = e.enqueue_extend_dah(static_cast<const uint8_t*>(d_ods), k, n, static_cast<uint8_t*>(d_eds),
                                            static_cast<uint8_t*>(d_row_roots), static_cast<uint8_t*>(d_col_roots),
                                            static_cast<uint8_t*>(d_data_roots), err, d_status, s);
        e.set_device_batch(rc == CDA_OK ? n : 0);
        return rc;
    });
}

int cda_reserve(cda_ctx* ctx, uint32_t k, uint32_t n) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (k == 0 || (k & (k - 1))) return not_pow2(e, k * k);
        if (k > 1024) return too_wide(e);
        return e.reserve(k, n);
    });
}

int cda_extend_dah_inplace_device(cda_ctx* ctx, uint32_t k, uint32_t n, void* d_eds, void* d_row_roots,
                                  void* d_col_roots, void* d_data_roots, int32_t* d_status, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (k == 0 || (k & (k - 1))) return not_pow2(e, k * k);
        if (n == 0) return CDA_OK;
        if (!d_eds || !d_row_roots || !d_col_roots || !d_data_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        uint32_t* err = e.err_words(n);
        if (!err) return e.fail(CDA_ERR_OOM, "hipMalloc err words");
        const int rc = e.enqueue_extend_dah(nullptr, k, n, static_cast<uint8_t*>(d_eds),
                                            static_cast<uint8_t*>(d_row_roots), static_cast<uint8_t*>(d_col_roots),
                                            static_cast<uint8_t*>(d_data_roots), err, d_status, s);
        e.set_device_batch(rc == CDA_OK ? n : 0);
        return rc;
    });
}

int cda_rs_encode(cda_ctx* ctx, const uint8_t* data, uint32_t n_shards, uint32_t shard_len, uint32_t n_codewords,
                  uint8_t* parity) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n_codewords == 0) return CDA_OK;
        if (!data || !parity) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_rs(data, n_shards, shard_len, n_codewords, parity);
    });
}

int cda_data_root(cda_ctx* ctx, const uint8_t* row_roots, const uint8_t* col_roots, uint32_t w, uint8_t* data_root) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!data_root) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (w == 0) {  // merkle.HashFromByteSlices(nil) = sha256("")
            memcpy(data_root, cda::kSha256Empty, 32);
            return CDA_OK;
        }
        if (w & (w - 1)) return e.fail(CDA_ERR_UNSUPPORTED, "root count must be a power of two");
        if (w > 2048) return e.fail(CDA_ERR_UNSUPPORTED, "more than 2048 roots per axis");
        if (!row_roots || !col_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_data_root(row_roots, col_roots, w, data_root);
    });
}

int cda_push_order_detail(cda_ctx* ctx, int32_t* axis, uint32_t* index, uint32_t* position) {
    if (!ctx) return CDA_ERR_INVALID;
    if (axis) *axis = tl_err.axis;
    if (index) *index = tl_err.index;
    if (position) *position = tl_err.pos;
    return CDA_OK;
}

int cda_push_order_detail_at(cda_ctx* ctx, uint32_t square, int32_t* axis, uint32_t* index, uint32_t* position) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!axis || !index || !position) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.device_push_order_detail(square, axis, index, position);
    });
}

int cda_split_rows(cda_ctx* ctx, const void* d_ods_rows, uint32_t k, uint32_t n_rows, uint32_t row0,
                   void* d_row_block, uint32_t* d_err, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (!d_ods_rows || !d_row_block || !d_err) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.enqueue_split_rows(static_cast<const uint8_t*>(d_ods_rows), k, n_rows, row0,
                                    static_cast<uint8_t*>(d_row_block), d_err, s);
    });
}

int cda_split_cols(cda_ctx* ctx, void* d_col_block, uint32_t k, uint32_t n_cols, uint32_t col0,
                   void* d_col_root_slots, void* d_row_subtree_slots, uint32_t* d_err, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (!d_col_block || !d_col_root_slots || !d_row_subtree_slots || !d_err)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.enqueue_split_cols(static_cast<uint8_t*>(d_col_block), k, n_cols, col0,
                                    static_cast<uint8_t*>(d_col_root_slots), static_cast<uint8_t*>(d_row_subtree_slots),
                                    d_err, s);
    });
}

int cda_split_combine(cda_ctx* ctx, const void* d_row_subtree_slots, uint32_t parts, uint32_t k,
                      const void* d_col_root_slots, void* d_row_roots, void* d_col_roots, void* d_data_root,
                      void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (!d_row_subtree_slots || !d_col_root_slots || !d_row_roots || !d_col_roots || !d_data_root)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.enqueue_split_combine(static_cast<const uint8_t*>(d_row_subtree_slots), parts, k,
                                       static_cast<const uint8_t*>(d_col_root_slots),
                                       static_cast<uint8_t*>(d_row_roots), static_cast<uint8_t*>(d_col_roots),
                                       static_cast<uint8_t*>(d_data_root), s);
    });
}

int cda_square_tx_share_range(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                              uint32_t max_square_size, uint32_t threshold, uint32_t tx_index, uint32_t* start,
                              uint32_t* end, int* is_pfb) {
    // Host-only (no device work): usable without a context.
    auto run = [&](std::string* err) -> int {
        if (!start || !end || (n_txs && (!txs || !tx_off))) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::square::Plan p;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, CDA_SQUARE_CONSTRUCT, &p, err))
            return CDA_ERR_SQUARE;
        if (tx_index >= p.unit_start.size()) {
            char b[64];
            snprintf(b, sizeof b, "txIndex %u out of range", tx_index);
            *err = b;
            return CDA_ERR_INVALID;
        }
        *start = p.unit_start[tx_index];
        *end = p.unit_end[tx_index];
        if (is_pfb) *is_pfb = tx_index >= p.n_normal;
        return CDA_OK;
    };
    return host_only(ctx, run);
}

int cda_square_tx_share_ranges(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                               uint32_t max_square_size, uint32_t threshold, const uint32_t* tx_indexes, uint32_t n,
                               uint32_t* starts, uint32_t* ends, uint8_t* is_pfb) {
    // Host-only (no device work): usable without a context.
    auto run = [&](std::string* err) -> int {
        if ((n && (!tx_indexes || !starts || !ends)) || (n_txs && (!txs || !tx_off))) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::square::Plan p;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, CDA_SQUARE_CONSTRUCT, &p, err))
            return CDA_ERR_SQUARE;
        for (uint32_t i = 0; i < n; i++)
            if (tx_indexes[i] >= p.unit_start.size()) {
                char b[64];
                snprintf(b, sizeof b, "txIndex %u out of range", tx_indexes[i]);
                *err = b;
                return CDA_ERR_INVALID;
            }
        for (uint32_t i = 0; i < n; i++) {
            starts[i] = p.unit_start[tx_indexes[i]];
            ends[i] = p.unit_end[tx_indexes[i]];
            if (is_pfb) is_pfb[i] = tx_indexes[i] >= p.n_normal;
        }
        return CDA_OK;
    };
    return host_only(ctx, run);
}

int cda_square_layout(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                      uint32_t max_square_size, uint32_t threshold, int mode, uint32_t* square_size, uint32_t* kept,
                      uint32_t* n_kept, uint32_t* share_indexes, uint32_t share_index_cap, uint32_t* n_share_indexes) {
    // Host-only (no device work): usable without a context.
    auto run = [&](std::string* err) -> int {
        if (!square_size || (n_txs && (!txs || !tx_off))) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::square::Plan p;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, mode, &p, err)) return CDA_ERR_SQUARE;
        *square_size = p.square_size;
        copy_kept(p, kept, n_kept);
        if (n_share_indexes) *n_share_indexes = (uint32_t)p.share_indexes.size();
        if (share_indexes) {
            if (p.share_indexes.size() > share_index_cap) {
                *err = "share_indexes capacity too small";
                return CDA_ERR_INVALID;
            }
            memcpy(share_indexes, p.share_indexes.data(), p.share_indexes.size() * 4);
        }
        return CDA_OK;
    };
    return host_only(ctx, run);
}

int cda_square_construct(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                         uint32_t max_square_size, uint32_t threshold, int mode, uint8_t* ods, size_t ods_capacity,
                         uint32_t* square_size, uint32_t* kept, uint32_t* n_kept) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!ods || !square_size || (n_txs && (!txs || !tx_off))) return e.fail(CDA_ERR_INVALID, "null buffer");
        cda::square::Plan p;
        std::string err;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, mode, &p, &err))
            return e.fail(CDA_ERR_SQUARE, err);
        *square_size = p.square_size;
        copy_kept(p, kept, n_kept);
        if ((size_t)p.square_size * p.square_size * CDA_SHARE_SIZE > ods_capacity)
            return e.fail(CDA_ERR_INVALID, "ods capacity too small for the square");
        return e.host_square(p, txs, n_txs ? tx_off[n_txs] : 0, ods);
    });
}

int cda_construct_extend_dah(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                             uint32_t max_square_size, uint32_t threshold, int mode, uint8_t* eds, size_t eds_capacity,
                             uint8_t* row_roots, uint8_t* col_roots, size_t roots_capacity, uint8_t* data_root,
                             uint32_t* square_size, uint32_t* kept, uint32_t* n_kept) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!row_roots || !col_roots || !data_root || !square_size || (n_txs && (!txs || !tx_off)))
            return e.fail(CDA_ERR_INVALID, "null buffer");
        cda::square::Plan p;
        std::string err;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, mode, &p, &err))
            return e.fail(CDA_ERR_SQUARE, err);
        *square_size = p.square_size;
        copy_kept(p, kept, n_kept);
        const size_t w = 2 * (size_t)p.square_size;
        if (w * CDA_NMT_ROOT_SIZE > roots_capacity) return e.fail(CDA_ERR_INVALID, "roots capacity too small");
        if (eds && w * w * CDA_SHARE_SIZE > eds_capacity) return e.fail(CDA_ERR_INVALID, "eds capacity too small");
        return e.host_construct_extend_dah(p, txs, n_txs ? tx_off[n_txs] : 0, eds, row_roots, col_roots, data_root);
    });
}

int cda_square_construct_device(cda_ctx* ctx, const uint8_t* txs, const uint64_t* tx_off, uint32_t n_txs,
                                const void* d_txs, uint32_t max_square_size, uint32_t threshold, int mode,
                                void* d_ods, size_t ods_capacity, uint32_t* square_size, uint32_t* kept,
                                uint32_t* n_kept, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (!d_ods || !square_size || (n_txs && (!txs || !tx_off || !d_txs)))
            return e.fail(CDA_ERR_INVALID, "null buffer");
        cda::square::Plan p;
        std::string err;
        if (plan_square(txs, tx_off, n_txs, max_square_size, threshold, mode, &p, &err))
            return e.fail(CDA_ERR_SQUARE, err);
        *square_size = p.square_size;
        copy_kept(p, kept, n_kept);
        if ((size_t)p.square_size * p.square_size * CDA_SHARE_SIZE > ods_capacity)
            return e.fail(CDA_ERR_INVALID, "ods capacity too small for the square");
        return e.enqueue_square(p, static_cast<const uint8_t*>(d_txs), static_cast<uint8_t*>(d_ods), s);
    });
}

int cda_blob_commitments(cda_ctx* ctx, const uint8_t* namespaces, const uint8_t* data, const uint64_t* data_off,
                         const uint8_t* share_versions, uint32_t n, uint32_t threshold, uint8_t* commitments) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n == 0) return CDA_OK;
        if (!namespaces || !data_off || !commitments || (data_off[n] > data_off[0] && !data))
            return e.fail(CDA_ERR_INVALID, "null buffer");
        cda::square::CommitPlan& p = e.commit_plan();
        std::string err;
        if (cda::square::plan_commitments(namespaces, data_off, share_versions, n, threshold, &p, &err))
            return e.fail(CDA_ERR_SQUARE, err);
        return e.host_commitments(p, n, data, (size_t)data_off[n], commitments);
    });
}

int cda_blob_commitments_device(cda_ctx* ctx, const uint8_t* namespaces, const uint64_t* data_off,
                                const uint8_t* share_versions, uint32_t n, uint32_t threshold, const void* d_data,
                                void* d_commitments, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (n == 0) return CDA_OK;
        if (!namespaces || !data_off || !d_commitments || (data_off[n] > data_off[0] && !d_data))
            return e.fail(CDA_ERR_INVALID, "null buffer");
        cda::square::CommitPlan& p = e.commit_plan();
        std::string err;
        if (cda::square::plan_commitments(namespaces, data_off, share_versions, n, threshold, &p, &err))
            return e.fail(CDA_ERR_SQUARE, err);
        return e.enqueue_commitments(p, n, static_cast<const uint8_t*>(d_data), static_cast<uint8_t*>(d_commitments),
                                     s);
    });
}

int cda_square_create(cda_ctx* ctx, const uint8_t* ods, uint32_t n_shares, cda_square** out) {
    if (!out) return CDA_ERR_INVALID;
    *out = nullptr;
    return guarded(ctx, [&](cda::Engine& e) -> int {
        uint32_t k;
        if (!square_width(n_shares, &k)) return not_pow2(e, n_shares);
        if (!ods) return e.fail(CDA_ERR_INVALID, "null buffer");
        cda_square* h = new cda_square{ctx, {}};
        const int rc = e.square_create(ods, k, &h->sq);
        if (rc != CDA_OK && rc != CDA_ERR_PUSH_ORDER) {
            delete h;
            return rc;
        }
        *out = h;   // a push-order failure still leaves the EDS (as ExtendShares does)
        return rc;
    });
}

int cda_square_destroy(cda_square* sq) {
    if (!sq) return CDA_OK;
    if (sq->owner)
        return guarded(sq->ctx, [&](cda::Engine& e) -> int {
            return e.fail(CDA_ERR_INVALID, "the square is a member of a cda_square_set and ends with it: "
                                           "call cda_square_set_destroy on the set");
        });
    std::lock_guard<std::mutex> g(sq->ctx->eng.mutex());
    DeviceScope dev(sq->ctx->eng.device());
    // no queued work of the context reads the square any more: the square's
    // calls end with the context's end event, and waiting for that (not every
    // context stream) leaves unrelated in-flight batch work alone
    (void)sq->ctx->eng.wait_last_call();
    delete sq;
    return CDA_OK;
}

int cda_square_dah(cda_square* sq, uint32_t* k, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_root,
                   uint8_t* eds) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (k) *k = sq->sq.k;
        if (row_roots) CDA_TRY(e.square_read(&sq->sq, cda::ResidentSquare::kRowRoots, row_roots));
        if (col_roots) CDA_TRY(e.square_read(&sq->sq, cda::ResidentSquare::kColRoots, col_roots));
        if (data_root) CDA_TRY(e.square_read(&sq->sq, cda::ResidentSquare::kDataRoot, data_root));
        if (eds) CDA_TRY(e.square_read(&sq->sq, cda::ResidentSquare::kEds, eds));
        return CDA_OK;
    });
}

int cda_square_share_proof(cda_square* sq, uint32_t start, uint32_t end, uint8_t* shares, uint32_t* start_row,
                           uint32_t* end_row, int32_t* nmt_start, int32_t* nmt_end, uint32_t* nmt_count,
                           uint8_t* nmt_nodes, uint8_t* row_roots, uint8_t* row_leaf_hash, uint8_t* row_aunts) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!nmt_start || !nmt_end || !nmt_count || !start_row || !end_row)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        *start_row = *end_row = 0;   // what a failed call leaves in them
        const cda_share_proofs_out o{.nmt_start = nmt_start, .nmt_end = nmt_end, .nodes = nmt_nodes,
                                     .row_roots = row_roots, .rfc_leaf_hash = row_leaf_hash, .aunts = row_aunts,
                                     .shares = shares, .start_row = start_row, .end_row = end_row};
        return e.square_share_proof(&sq->sq, start, end, o, nmt_count);
    });
}

int cda_square_blob_commitments(cda_square* sq, const uint32_t* starts, const uint32_t* share_lens, uint32_t n,
                                uint32_t threshold, uint8_t* commitments) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (n && (!starts || !share_lens || !commitments)) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_blob_commitments(&sq->sq, starts, share_lens, n, threshold, commitments);
    });
}

int cda_square_subtree_root(cda_square* sq, uint32_t row, const uint8_t* walk, uint32_t walk_len, uint8_t* root) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!root || (walk_len && !walk)) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_subtree_root(&sq->sq, row, walk, walk_len, root);
    });
}

int cda_square_sample_proofs(cda_square* sq, const uint32_t* rows, const uint32_t* cols, const uint8_t* axes,
                             uint32_t n, uint8_t* shares, uint8_t* namespaces, uint8_t* nmt_nodes,
                             uint8_t* axis_roots, uint8_t* leaf_hash, uint8_t* aunts) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        const cda::Engine::SampleOut o{shares, namespaces, nmt_nodes, axis_roots, leaf_hash, aunts};
        return e.square_sample_proofs(&sq->sq, rows, cols, axes, n, o);
    });
}

// Both create calls: src on the host or d_src on the device.
static int square_set_create(cda_ctx* ctx, const uint8_t* src, const void* d_src, int kind, uint32_t k, uint32_t n,
                             void* stream, bool device, cda_square_set** out) {
    if (!out) return CDA_ERR_INVALID;
    *out = nullptr;
    auto run = [&](cda::Engine& e, hipStream_t s) -> int {
        if (kind != CDA_SET_FROM_ODS && kind != CDA_SET_FROM_EDS)
            return e.fail(CDA_ERR_INVALID, "unknown source kind of a square set");
        if (!cda::is_pow2(k) || k > 1024)
            return e.fail(CDA_ERR_INVALID, "square width must be a power of two <= 1024");
        if (n == 0) return e.fail(CDA_ERR_INVALID, "a square set holds at least one square");
        if (n > CDA_SET_MAX_SQUARES) return e.fail(CDA_ERR_INVALID, "a square set holds at most 65535 squares");
        if (device ? !d_src : !src) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (device && (reinterpret_cast<uintptr_t>(d_src) & 15))
            return e.fail(CDA_ERR_INVALID, "device_src must be 16-byte aligned");
        std::unique_ptr<cda_square_set> h(new cda_square_set{ctx, {}, {}});
        const int rc = e.square_set_create(src, static_cast<const uint8_t*>(d_src), kind, k, n, &h->set, s);
        if (rc != CDA_OK && rc != CDA_ERR_PUSH_ORDER) return rc;
        h->members.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            h->members.emplace_back(new cda_square{ctx, {}, h.get()});
            h->set.lend(i, &h->members.back()->sq);
        }
        *out = h.release();   // unordered squares stay in the set with their blind roots
        return rc;
    };
    if (device) return guarded_stream(ctx, stream, run);
    return guarded(ctx, [&](cda::Engine& e) -> int { return run(e, e.stream()); });
}

int cda_square_set_create(cda_ctx* ctx, const uint8_t* src, int kind, uint32_t k, uint32_t n, cda_square_set** out) {
    return square_set_create(ctx, src, nullptr, kind, k, n, nullptr, false, out);
}

int cda_square_set_create_device(cda_ctx* ctx, const void* device_src, int kind, uint32_t k, uint32_t n, void* stream,
                                 cda_square_set** out) {
    return square_set_create(ctx, nullptr, device_src, kind, k, n, stream, true, out);
}

int cda_square_set_destroy(cda_square_set* set) {
    if (!set) return CDA_OK;
    std::lock_guard<std::mutex> g(set->ctx->eng.mutex());
    DeviceScope dev(set->ctx->eng.device());
    // as cda_square_destroy: every call on the set or a member ended with the context's end event
    (void)set->ctx->eng.wait_last_call();
    delete set;   // the members first (their own scratch), then the arenas
    return CDA_OK;
}

int cda_square_set_info(cda_square_set* set, uint32_t* k, uint32_t* n) {
    if (!set) return CDA_ERR_INVALID;
    if (k) *k = set->set.k;
    if (n) *n = set->set.n;
    return CDA_OK;
}

int cda_square_set_at(cda_square_set* set, uint32_t i, cda_square** member) {
    if (!set || !member) return CDA_ERR_INVALID;
    *member = nullptr;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        if (i >= set->set.n)
            return e.fail(CDA_ERR_INVALID, "square " + std::to_string(i) + " is not below the set's " +
                                               std::to_string(set->set.n) + " squares");
        *member = set->members[i].get();
        return CDA_OK;
    });
}

int cda_square_set_dah(cda_square_set* set, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots,
                       int32_t* status) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        return e.square_set_dah(&set->set, row_roots, col_roots, data_roots, status);
    });
}

int cda_square_set_sample_proofs(cda_square_set* set, const uint32_t* squares, const uint32_t* rows,
                                 const uint32_t* cols, const uint8_t* axes, uint32_t n, uint8_t* shares,
                                 uint8_t* namespaces, uint8_t* nmt_nodes, uint8_t* axis_roots, uint8_t* leaf_hash,
                                 uint8_t* aunts) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        const cda::Engine::SampleOut o{shares, namespaces, nmt_nodes, axis_roots, leaf_hash, aunts};
        return e.square_set_sample_proofs(&set->set, squares, rows, cols, axes, n, o);
    });
}

int cda_square_set_namespace_plan(cda_square_set* set, const uint32_t* squares, const uint8_t* namespaces, uint32_t n,
                                  cda_namespace_plan_t* out) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_set_namespace_plan(&set->set, squares, namespaces, n, out);
    });
}

int cda_square_set_namespace_proofs(cda_square_set* set, const uint32_t* squares, const uint8_t* namespaces,
                                    uint32_t n, const cda_namespace_proofs_out* out) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_set_namespace_proofs(&set->set, squares, namespaces, n, *out);
    });
}

int cda_square_set_share_proofs(cda_square_set* set, const uint32_t* squares, const uint32_t* starts,
                                const uint32_t* ends, uint32_t n, const cda_share_proofs_out* out) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_set_share_proofs(&set->set, squares, starts, ends, n, *out);
    });
}

int cda_square_share_proofs_plan(uint32_t k, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                                 cda_share_proofs_plan_t* out) {
    // Host-only (no device work), no context.
    return host_only(nullptr, [&](std::string* err) -> int {
        if (!out) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::ShareProofsPlan p;
        *err = cda::share_proofs_plan(k, starts, ends, n, &p);
        if (!err->empty()) return CDA_ERR_INVALID;
        *out = cda_share_proofs_plan_t{p.n_segments, p.n_nodes, p.n_aunts, p.aunts_per_segment, p.n_shares};
        return CDA_OK;
    });
}

int cda_square_share_proofs(cda_square* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                            const cda_share_proofs_out* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_share_proofs(&sq->sq, starts, ends, n, *out);
    });
}

int cda_square_commitment_proofs_plan(uint32_t k, const uint32_t* starts, const uint32_t* share_lens, uint32_t n,
                                      uint32_t threshold, cda_commitment_proofs_plan_t* out) {
    // Host-only (no device work), no context.
    return host_only(nullptr, [&](std::string* err) -> int {
        if (!out) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::CommitmentProofsPlan p;
        *err = cda::commitment_proofs_plan(k, starts, share_lens, n, threshold, &p);
        if (!err->empty()) return CDA_ERR_INVALID;
        *out = cda_commitment_proofs_plan_t{p.n_segments, p.n_roots, p.n_nodes, p.n_aunts, p.aunts_per_segment};
        return CDA_OK;
    });
}

int cda_square_commitment_proofs(cda_square* sq, const uint32_t* starts, const uint32_t* share_lens, uint32_t n,
                                 uint32_t threshold, const cda_commitment_proofs_out* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_commitment_proofs(&sq->sq, starts, share_lens, n, threshold, *out);
    });
}

int cda_commitment_proofs_verify(cda_ctx* ctx, const cda_commitment_proof_batch* b, uint8_t* verdict) {
    return guarded(ctx, [&](cda::Engine& e) -> int { return e.commitment_proofs_verify(b, verdict); });
}

int cda_square_namespace_plan(cda_square* sq, const uint8_t* namespaces, uint32_t n, cda_namespace_plan_t* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_namespace_plan(&sq->sq, namespaces, n, out);
    });
}

int cda_square_namespace_proofs(cda_square* sq, const uint8_t* namespaces, uint32_t n,
                                const cda_namespace_proofs_out* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_namespace_proofs(&sq->sq, namespaces, n, *out);
    });
}

int cda_shares_parse_plan(const uint8_t* shares, uint64_t n_shares, cda_parse_plan_t* out) {
    // Host-only (no device work), no context.
    return host_only(nullptr, [&](std::string* err) -> int {
        if (!out) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        return cda::shares_parse(shares, n_shares, out, nullptr, err);
    });
}

int cda_shares_parse(const uint8_t* shares, uint64_t n_shares, const cda_parse_out* out) {
    return host_only(nullptr, [&](std::string* err) -> int {
        if (!out) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        return cda::shares_parse(shares, n_shares, nullptr, out, err);
    });
}

int cda_square_parse_plan(cda_square* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n_ranges,
                          cda_parse_plan_t* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_parse(&sq->sq, starts, ends, n_ranges, out, nullptr);
    });
}

int cda_square_parse(cda_square* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n_ranges,
                     const cda_parse_out* out) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.square_parse(&sq->sq, starts, ends, n_ranges, nullptr, out);
    });
}

int cda_namespace_proofs_verify(cda_ctx* ctx, uint32_t k, const uint8_t* row_roots,
                                const cda_namespace_proof_batch* b, uint8_t* verdict) {
    return guarded(ctx, [&](cda::Engine& e) -> int { return e.namespace_proofs_verify(k, row_roots, b, verdict); });
}

int cda_namespace_proofs_verify_set(cda_ctx* ctx, uint32_t k, const uint8_t* row_roots, uint32_t n_squares,
                                    const uint32_t* squares, const cda_namespace_proof_batch* b, uint8_t* verdict) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (b && b->n_queries && !squares) return e.fail(CDA_ERR_INVALID, "null squares");
        return e.namespace_proofs_verify_set(k, row_roots, n_squares, squares, b, verdict);
    });
}

int cda_sample_proofs_verify(cda_ctx* ctx, uint32_t k, uint32_t n, const uint8_t* data_roots, const uint32_t* rows,
                             const uint32_t* cols, const uint8_t* axes, const uint8_t* shares,
                             const uint8_t* nmt_nodes, const uint8_t* axis_roots, const uint8_t* leaf_hash,
                             const uint8_t* aunts, uint8_t* verdict) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        return e.sample_proofs_verify(k, n, data_roots, rows, cols, axes, shares, nmt_nodes, axis_roots, leaf_hash,
                                      aunts, verdict);
    });
}

int cda_repair(cda_ctx* ctx, uint8_t* eds, const uint8_t* present, uint32_t w, const uint8_t* row_roots,
               const uint8_t* col_roots, int32_t* byz_axis, uint32_t* byz_index) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!eds || !present || !row_roots || !col_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (byz_axis) *byz_axis = -1;
        return e.host_repair(eds, present, w, row_roots, col_roots, byz_axis, byz_index);
    });
}

int cda_repair_device(cda_ctx* ctx, void* d_eds, const uint8_t* present, uint32_t w, const uint8_t* row_roots,
                      const uint8_t* col_roots, int32_t* byz_axis, uint32_t* byz_index) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!d_eds || !present || !row_roots || !col_roots) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (byz_axis) *byz_axis = -1;
        return e.device_repair(static_cast<uint8_t*>(d_eds), present, w, row_roots, col_roots, byz_axis, byz_index);
    });
}

int cda_repair_batch_device(cda_ctx* ctx, void* d_eds, const uint8_t* present, uint32_t w, uint32_t n,
                            const uint8_t* row_roots, const uint8_t* col_roots, int32_t* status, int32_t* byz_axis,
                            uint32_t* byz_index) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n == 0) return CDA_OK;
        if (!d_eds || !present || !row_roots || !col_roots || !status) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.device_repair_batch(static_cast<uint8_t*>(d_eds), present, w, n, row_roots, col_roots, status,
                                     byz_axis, byz_index);
    });
}

int cda_repair_batch(cda_ctx* ctx, uint8_t* eds, const uint8_t* present, uint32_t w, uint32_t n,
                     const uint8_t* row_roots, const uint8_t* col_roots, int32_t* status, int32_t* byz_axis,
                     uint32_t* byz_index) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n == 0) return CDA_OK;
        if (!eds || !present || !row_roots || !col_roots || !status) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_repair_batch(eds, present, w, n, row_roots, col_roots, status, byz_axis, byz_index);
    });
}

int cda_repair_batch_plan(const uint8_t* present, uint32_t w, uint32_t n, uint32_t* n_segments, uint32_t* seg_off,
                          uint32_t* seg_sweep, uint32_t* entries, uint8_t* solved) {
    // Host-only (no device work), no context.
    return host_only(nullptr, [&](std::string* err) -> int {
        if (w < 2 || (w & (w - 1)) || w > 1024) {
            *err = "EDS width must be a power of two in [2, 1024]";
            return CDA_ERR_INVALID;
        }
        if (n && !present) {
            *err = "null buffer";
            return CDA_ERR_INVALID;
        }
        cda::RepairPlan p;
        cda::repair_plan(present, n, w, &p);
        if (n_segments) *n_segments = p.n_segments();
        if (seg_off) memcpy(seg_off, p.seg_off.data(), p.seg_off.size() * 4);
        if (seg_sweep && p.n_segments()) memcpy(seg_sweep, p.seg_sweep.data(), p.seg_sweep.size() * 4);
        if (entries && !p.entries.empty()) memcpy(entries, p.entries.data(), p.entries.size() * sizeof(cda::RepairEntry));
        if (solved && n) memcpy(solved, p.solved.data(), n);
        return CDA_OK;
    });
}

int cda_rs_decode(cda_ctx* ctx, uint8_t* shards, const uint8_t* present, uint32_t n_shards, uint32_t shard_len,
                  uint32_t n_codewords) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n_codewords == 0) return CDA_OK;
        if (!shards || !present) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_rs_decode(shards, present, n_shards, shard_len, n_codewords);
    });
}

int cda_befp_build(cda_ctx* ctx, const uint8_t* eds, uint32_t w, int axis, uint32_t index, const uint8_t* row_roots,
                   const uint8_t* col_roots, uint32_t* n_out, uint32_t* positions, uint8_t* shares,
                   uint8_t* nmt_nodes) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!eds || !row_roots || !col_roots || !n_out || !positions || !shares || !nmt_nodes)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.befp_build(eds, nullptr, w, axis, index, row_roots, col_roots, n_out, positions, shares, nmt_nodes);
    });
}

int cda_befp_build_device(cda_ctx* ctx, const void* d_eds, uint32_t w, int axis, uint32_t index,
                          const uint8_t* row_roots, const uint8_t* col_roots, uint32_t* n_out, uint32_t* positions,
                          uint8_t* shares, uint8_t* nmt_nodes) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!d_eds || !row_roots || !col_roots || !n_out || !positions || !shares || !nmt_nodes)
            return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.befp_build(nullptr, static_cast<const uint8_t*>(d_eds), w, axis, index, row_roots, col_roots, n_out,
                            positions, shares, nmt_nodes);
    });
}

int cda_befp_batch_check(const cda_befp_batch* b) {
    // Host-only (no device work), no context.
    return host_only(nullptr, [&](std::string* err) -> int {
        *err = cda::befp_batch_check(b);
        return err->empty() ? CDA_OK : CDA_ERR_INVALID;
    });
}

int cda_befp_verify(cda_ctx* ctx, const cda_befp_batch* b, uint8_t* verdict, uint8_t* rebuilt_roots) {
    return guarded(ctx, [&](cda::Engine& e) -> int { return e.befp_verify(b, verdict, rebuilt_roots); });
}

int cda_square_axis_halves(cda_square* sq, const uint8_t* axes, const uint32_t* indexes, const uint8_t* sides,
                           uint32_t n, uint8_t* shares) {
    if (!sq) return CDA_ERR_INVALID;
    return guarded(sq->ctx, [&](cda::Engine& e) -> int {
        return e.axis_halves(&sq->sq, nullptr, nullptr, axes, indexes, sides, n, shares);
    });
}

int cda_square_set_axis_halves(cda_square_set* set, const uint32_t* squares, const uint8_t* axes,
                               const uint32_t* indexes, const uint8_t* sides, uint32_t n, uint8_t* shares) {
    if (!set) return CDA_ERR_INVALID;
    return guarded(set->ctx, [&](cda::Engine& e) -> int {
        return e.axis_halves(nullptr, &set->set, squares, axes, indexes, sides, n, shares);
    });
}

int cda_axis_halves_verify(cda_ctx* ctx, uint32_t k, const uint8_t* row_roots, const uint8_t* col_roots,
                           uint32_t n_squares, const uint32_t* squares, const uint8_t* axes, const uint32_t* indexes,
                           const uint8_t* sides, uint32_t n, const uint8_t* shares, uint8_t* verdict,
                           uint8_t* vectors) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        return e.axis_halves_verify(k, row_roots, col_roots, n_squares, squares, axes, indexes, sides, n, shares,
                                    verdict, vectors);
    });
}

int cda_rs_recover_data(cda_ctx* ctx, const uint8_t* parity, uint32_t n_shards, uint32_t shard_len,
                        uint32_t n_codewords, uint8_t* data) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n_codewords == 0) return CDA_OK;
        if (!parity || !data) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.host_rs_recover(parity, n_shards, shard_len, n_codewords, data);
    });
}

int cda_nmt_axis_roots(cda_ctx* ctx, const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t n_trees,
                       uint32_t square_size, const uint32_t* axis_index, uint8_t* roots, int32_t* status) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (n_trees == 0) return CDA_OK;
        if (square_size == 0) return e.fail(CDA_ERR_INVALID, "cannot create a ErasuredNamespacedMerkleTree of squareSize == 0");
        if (!roots || !axis_index || (n_cells && !cells)) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (cell_len < CDA_NAMESPACE_SIZE) return e.fail(CDA_ERR_INVALID, "data is too short to contain namespace ID");
        for (uint32_t t = 0; t < n_trees; t++) {
            // wrapper Push (pkg/wrapper/nmt_wrapper.go:94-96)
            if ((uint64_t)axis_index[t] + 1 > 2ull * square_size || (uint64_t)n_cells > 2ull * square_size) {
                char buf[160];
                snprintf(buf, sizeof buf, "pushed past predetermined square size: boundary at %llu index at %u %u",
                         2ull * square_size, axis_index[t], n_cells > 2 * square_size ? 2 * square_size : n_cells - 1);
                return e.fail(CDA_ERR_INVALID, buf);
            }
        }
        return e.nmt_axis_roots(cells, cell_len, n_cells, n_trees, square_size, axis_index, roots, status);
    });
}

int cda_nmt_axis_root(cda_ctx* ctx, const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                      uint32_t axis_index, uint8_t* root) {
    return cda_nmt_axis_roots(ctx, cells, cell_len, n_cells, 1, square_size, &axis_index, root, nullptr);
}

int cda_nmt_prove_range(cda_ctx* ctx, const uint8_t* cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                        uint32_t axis_index, uint32_t start, uint32_t end, uint8_t* nodes, uint32_t* n_nodes,
                        uint8_t* root) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (square_size == 0) return e.fail(CDA_ERR_INVALID, "cannot create a ErasuredNamespacedMerkleTree of squareSize == 0");
        if (!cells || !n_nodes) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (cell_len < CDA_NAMESPACE_SIZE) return e.fail(CDA_ERR_INVALID, "data is too short to contain namespace ID");
        if ((uint64_t)axis_index + 1 > 2ull * square_size || (uint64_t)n_cells > 2ull * square_size)
            return e.fail(CDA_ERR_INVALID, "pushed past predetermined square size");
        return e.nmt_prove_range(cells, cell_len, n_cells, square_size, axis_index, start, end, nodes, n_nodes, root);
    });
}

int cda_merkle_root(cda_ctx* ctx, const uint8_t* items, const uint64_t* off, uint32_t n, uint8_t* out) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!out) return e.fail(CDA_ERR_INVALID, "null buffer");
        if (n == 0) {   // merkle.HashFromByteSlices(nil) = sha256("")
            memcpy(out, cda::kSha256Empty, 32);
            return CDA_OK;
        }
        if (!off || (off[n] > off[0] && !items)) return e.fail(CDA_ERR_INVALID, "null buffer");
        for (uint32_t i = 0; i < n; i++)
            if (off[i + 1] < off[i]) return e.fail(CDA_ERR_INVALID, "item offsets must be non-decreasing");
        return e.merkle_root(items, off, n, out);
    });
}

int cda_share_proofs_verify(cda_ctx* ctx, const cda_share_proof_batch* b, uint8_t* verdict) {
    return guarded(ctx, [&](cda::Engine& e) -> int { return e.share_proofs_verify(b, verdict); });
}

int cda_comm_unique_id(uint8_t* id) {
    if (!id) return CDA_ERR_INVALID;
    tl_err.msg.clear();
    int rc = cda::comm_unique_id(id);
    if (rc) tl_err.msg = "ncclGetUniqueId failed";
    return rc;
}

int cda_comm_init(cda_ctx* ctx, int rank, int world, const uint8_t* id) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!id) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.comm_init(rank, world, id);
    });
}

int cda_comm_destroy(cda_ctx* ctx) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        e.comm_destroy();
        return CDA_OK;
    });
}

int cda_comm_size(cda_ctx* ctx, int* rank, int* world) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        if (!rank || !world) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.comm_size(rank, world);
    });
}

int cda_comm_abort(cda_ctx* ctx) {
    // no context lock: a watchdog thread may call this while another thread
    // is blocked inside a collective on the same context
    if (!ctx) return CDA_ERR_INVALID;
    DeviceScope dev(ctx->eng.device());
    return ctx->eng.comm_abort();
}

int cda_split_rows_send(cda_ctx* ctx, const void* d_ods_rows, uint32_t k, uint32_t n_rows, uint32_t row0,
                        uint32_t parts, void* d_send, uint32_t* d_err, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        if (!d_ods_rows || !d_send || !d_err) return e.fail(CDA_ERR_INVALID, "null buffer");
        return e.enqueue_split_rows_send(static_cast<const uint8_t*>(d_ods_rows), k, n_rows, row0, parts,
                                         static_cast<uint8_t*>(d_send), d_err, s);
    });
}

int cda_extend_dah_split(cda_ctx* ctx, const void* d_ods_rows, uint32_t k, void* d_col_block, void* d_row_roots,
                         void* d_col_roots, void* d_data_root, uint32_t* d_err, void* stream) {
    return guarded_stream(ctx, stream, [&](cda::Engine& e, hipStream_t s) -> int {
        // per-rank buffer checks happen inside, after this rank has taken part
        // in every collective (an early return here would leave the peers
        // blocked in the all-to-all)
        return e.split_extend_dah(static_cast<const uint8_t*>(d_ods_rows), k, static_cast<uint8_t*>(d_col_block),
                                  static_cast<uint8_t*>(d_row_roots), static_cast<uint8_t*>(d_col_roots),
                                  static_cast<uint8_t*>(d_data_root), d_err, s);
    });
}

int cda_split_layout(uint32_t k, uint32_t world, cda_split_layout_t* out) {
    if (!out) return CDA_ERR_INVALID;
    const cda::SplitLayout L(k, world ? world : 1);
    if (!world || !L.valid() || world > 2 * k) return CDA_ERR_INVALID;
    *out = cda_split_layout_t{L.k, L.G, L.W, L.R, L.C, L.piece(), L.send_bytes(), L.col_block_bytes(),
                              L.col_slots_off(), L.row_sub_off(), L.gather_sub_off(0), L.gather_col_off(0),
                              L.err_off(), L.slots_bytes()};
    return CDA_OK;
}

int cda_split_offsets(uint32_t k, uint32_t world, int what, uint32_t n, const uint32_t* a, const uint32_t* b,
                      uint64_t* off) {
    if (!world || !off || (n && !a)) return CDA_ERR_INVALID;
    const cda::SplitLayout L(k, world);
    if (!L.valid()) return CDA_ERR_INVALID;
    // (a, b) ranges per kind; b must be given where the kind reads it
    uint32_t amax, bmax = 1;
    switch (what) {
        case CDA_SPLIT_SEND: amax = L.R; bmax = L.W; break;
        case CDA_SPLIT_BLOCK: amax = L.W; bmax = L.C; break;
        case CDA_SPLIT_COMBINE: amax = L.G; bmax = L.W; break;
        case CDA_SPLIT_SEND_PIECE: case CDA_SPLIT_RECV_PIECE: case CDA_SPLIT_GATHER_SUB: case CDA_SPLIT_GATHER_COL:
            amax = L.G; break;
        default: return CDA_ERR_INVALID;
    }
    if (n && bmax > 1 && !b) return CDA_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (a[i] >= amax || (bmax > 1 && b[i] >= bmax)) return CDA_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t x = a[i], y = bmax > 1 ? b[i] : 0;
        switch (what) {
            case CDA_SPLIT_SEND: off[i] = L.send_off(x, y); break;
            case CDA_SPLIT_SEND_PIECE: off[i] = L.send_piece_off(x); break;
            case CDA_SPLIT_RECV_PIECE: off[i] = L.recv_piece_off(x); break;
            case CDA_SPLIT_BLOCK: off[i] = L.block_off(x, y); break;
            case CDA_SPLIT_GATHER_SUB: off[i] = L.gather_sub_off(x); break;
            case CDA_SPLIT_GATHER_COL: off[i] = L.gather_col_off(x); break;
            case CDA_SPLIT_COMBINE: off[i] = L.combine_slot(x, y); break;
            default: return CDA_ERR_INVALID;
        }
    }
    return CDA_OK;
}

int cda_extend_dah_multi(cda_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* ods, uint32_t k, uint32_t n,
                         uint8_t* eds, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots, int32_t* status) {
    tl_err.msg.clear();
    if (!ctxs || n_ctx == 0) {
        tl_err.msg = "no contexts";
        return CDA_ERR_INVALID;
    }
    if (n == 0) return CDA_OK;
    const uint32_t W = 2 * k;
    const size_t ods_sq = (size_t)k * k * CDA_SHARE_SIZE, eds_sq = (size_t)W * W * CDA_SHARE_SIZE;
    const size_t roots_sq = (size_t)W * CDA_NMT_ROOT_SIZE;
    std::vector<int> rcs(n_ctx, CDA_OK);
    std::vector<std::string> msgs(n_ctx);
    std::vector<std::thread> th;
    uint32_t first = 0;
    try {
        for (uint32_t d = 0; d < n_ctx; d++) {
            // context d: squares [first, first + m), config 4's contiguous shard
            const uint32_t m = n / n_ctx + (d < n % n_ctx ? 1 : 0);
            if (m == 0) continue;
            th.emplace_back([=, &rcs, &msgs] {
                rcs[d] = cda_extend_dah_batch(ctxs[d], ods + first * ods_sq, k, m,
                                              eds ? eds + first * eds_sq : nullptr, row_roots + first * roots_sq,
                                              col_roots + first * roots_sq, data_roots + (size_t)first * 32,
                                              status ? status + first : nullptr);
                msgs[d] = tl_err.msg;   // the worker thread's error text
            });
            first += m;
        }
    } catch (...) {
        for (auto& t : th) t.join();
        tl_err.msg = "thread creation failed";
        return CDA_ERR_DEVICE;
    }
    for (auto& t : th) t.join();
    // the first device error wins over push-order (reported per square in status)
    int rc = CDA_OK;
    for (uint32_t d = 0; d < n_ctx; d++) {
        if (rcs[d] != CDA_OK && (rc == CDA_OK || rc == CDA_ERR_PUSH_ORDER) && rc != rcs[d]) {
            rc = rcs[d];
            tl_err.msg = msgs[d];
        }
    }
    return rc;
}

int cda_set_profiling(cda_ctx* ctx, int enable) {
    return guarded(ctx, [&](cda::Engine& e) -> int {
        e.set_profiling(enable != 0);
        return CDA_OK;
    });
}

int cda_stage_times(cda_ctx* ctx, double* ms, uint32_t* counts, int n_stages) {
    return guarded(ctx, [&](cda::Engine& e) -> int { return e.collect_stage_times(ms, counts, n_stages); });
}

}  // extern "C"
