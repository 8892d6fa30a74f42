/*
 * cda.h -- C ABI of libcda.so, the MI355X (gfx950) implementation of
 * celestia-app's block data-availability hot path:
 *
 *   ODS (k x k shares of 512 B) -> EDS (2k x 2k, Leopard RS) -> 4k NMT
 *   row/column roots -> DataAvailabilityHeader data root.
 *
 * Every entry point replaces one reference interface (paths relative to the
 * celestia-app v3 tree; EXT = third-party Go module pinned in go.mod):
 *
 *   cda_extend_shares      da.ExtendShares            pkg/da/data_availability_header.go:65-75
 *   cda_dah_from_eds       da.NewDataAvailabilityHeader pkg/da/data_availability_header.go:44-63
 *                          (+ rsmt2d (*EDS).RowRoots/ColRoots via
 *                          wrapper.NewConstructor, pkg/wrapper/nmt_wrapper.go:73-86)
 *   cda_extend_dah         ExtendShares + NewDataAvailabilityHeader in one
 *                          submission (app/prepare_proposal.go:61,71;
 *                          app/process_proposal.go:138,144)
 *   cda_extend_dah_batch   the same for n independent squares
 *   cda_rs_encode          rsmt2d Codec.Encode (appconsts.DefaultCodec,
 *                          pkg/appconsts/global_consts.go:92 -> LeoRSCodec)
 *   cda_data_root          (*DataAvailabilityHeader).Hash
 *                          pkg/da/data_availability_header.go:92-108
 *   cda_extend_dah_device  device-resident batch (inputs/outputs in HBM)
 *   cda_extend_dah_inplace_device
 *                          the same with the ODS already in Q0 of the EDS
 *                          (rsmt2d ImportExtendedDataSquare-style arena)
 *   cda_square_layout / cda_square_construct / cda_construct_extend_dah /
 *   cda_square_construct_device
 *                          go-square square.Construct / square.Build (EXT
 *                          v1.1.0, go.mod:9; app/process_proposal.go:122,
 *                          app/prepare_proposal.go:50, app/extend_block.go:16)
 *   cda_blob_commitments   go-square inclusion.CreateCommitment
 *                          (x/blob/types/blob_tx.go:98, payforblob.go:53)
 *   cda_repair             rsmt2d ExtendedDataSquare.Repair (EXT v0.14.0)
 *   cda_repair_batch / cda_repair_batch_device / cda_repair_batch_plan
 *                          Repair of many squares of one width in one
 *                          submission, every sweep planned on the host first
 *   cda_rs_decode          rsmt2d Codec.Decode (reedsolomon Reconstruct)
 *   cda_square_*           resident squares: proof.NewShareInclusionProofFromEDS
 *                          (pkg/proof/proof.go:77), inclusion.GetCommitment
 *                          (pkg/inclusion/get_commit.go:12)
 *   cda_square_sample_proofs / cda_sample_proofs_verify
 *                          data-availability sampling of a built EDS: any cell
 *                          (parity included) with nmt ProveRange(p, p+1) of its
 *                          row or column tree (rsmt2d / wrapper trees,
 *                          pkg/wrapper/nmt_wrapper.go:55-129) and the merkle proof
 *                          of that root in the DAH; batched, and the batch check
 *   cda_square_share_proofs / cda_square_share_proofs_plan
 *                          NewShareInclusionProofFromEDS for many ranges of one
 *                          square in one launch, as a cda_share_proof_batch
 *   cda_square_namespace_plan / cda_square_namespace_proofs / cda_namespace_proofs_verify
 *                          all shares of many namespaces of one square with nmt
 *                          ProveNamespace's proofs (EXT nmt v0.22.0; absence proofs
 *                          included), the rows chosen as GetSharesByNamespace chooses
 *                          them from the DAH, and Proof.VerifyNamespace of the answers
 *   cda_square_set_namespace_plan / cda_square_set_namespace_proofs /
 *   cda_square_set_share_proofs / cda_namespace_proofs_verify_set
 *                          the same queries across a set of resident squares (a range
 *                          of heights) in the launches of one square's call
 *   cda_shares_parse_plan / cda_shares_parse / cda_square_parse_plan / cda_square_parse
 *                          go-square shares.ParseShares / ParseTxs / ParseBlobs (EXT v1.1.0): a
 *                          square's shares back into its transactions, IndexWrappers and blobs,
 *                          on the host or from a resident square's Q0 on the device
 *   cda_nmt_axis_root(s) / cda_nmt_prove_range
 *                          wrapper.NewErasuredNamespacedMerkleTree + Push +
 *                          Root / ProveRange (pkg/wrapper/nmt_wrapper.go:55-129)
 *   cda_merkle_root        go-square/merkle HashFromByteSlices (DAH.Hash for
 *                          any root count, data_availability_header.go:92-108)
 *   cda_share_proofs_verify
 *                          ShareProof.Validate / VerifyProof and RowProof.Validate
 *                          (pkg/proof/share_proof.go:16-82, row_proof.go:13-51),
 *                          batched
 *   cda_comm_* / cda_extend_dah_split / cda_extend_dah_multi
 *                          multi-GPU configs 4 and 5 (app/process_proposal.go:138-152
 *                          block replay; one square over G GPUs)
 *
 * Conventions
 *   - All buffers are plain byte arrays; shares are row-major and contiguous
 *     (share (r, c) of a width-w square at offset (r*w + c)*512).  NMT roots
 *     are 90 bytes (min ns 29 || max ns 29 || sha256 32), packed.
 *   - Inputs are borrowed for the duration of the call; outputs are written to
 *     caller-owned buffers; the library keeps no pointer after return.
 *   - Return value: CDA_OK (0) or a negative CDA_ERR_* code.  The message of
 *     the calling thread's last call is available from cda_last_error(); it
 *     uses the reference's error text where one exists.  The library never
 *     aborts across the ABI.
 *   - A context owns one HIP device and stream; calls on one context are
 *     serialised by an internal mutex (rsmt2d calls Codec/Tree from many
 *     goroutines) and may come from any OS thread (the context's device is
 *     made current for the call).  Device entry points only enqueue on the
 *     caller's stream; their GPU work is ordered after the previous call's on
 *     the same context (any stream), because the context's scratch is shared.
 *     Use one context per device.
 *   - Alignment of device pointers.  A device pointer must be aligned to the
 *     widest access a kernel makes straight through it (host buffers need only
 *     their element type's alignment).  The library does not check this: a
 *     pointer below its alignment is the caller's error.  The values,
 *     repeated at each argument below:
 *       16  share buffers (d_ods, d_eds, d_ods_rows, d_row_block, d_col_block,
 *           d_send) and arrays of 96-byte node slots (d_col_root_slots,
 *           d_row_subtree_slots): 16-byte loads and stores;
 *        8  d_ods of cda_square_construct_device: the share writer stores 8
 *           bytes per lane;
 *        4  32-byte digests (d_data_roots, d_data_root, d_commitments), the
 *           status and push-order words (d_status, d_err), and the byte
 *           buffers d_txs / d_data (read as 4-byte words from the pointer);
 *        2  packed 90-byte roots (d_row_roots, d_col_roots): 2-byte stores.
 *     The layouts' strides (512, 96, 90, 32, 4) keep every element of a batch
 *     at the alignment of the first.
 */
#ifndef CDA_H
#define CDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDA_SHARE_SIZE 512     /* appconsts.ShareSize, pkg/appconsts/global_consts.go:29 */
#define CDA_NAMESPACE_SIZE 29  /* appconsts.NamespaceSize, global_consts.go:26 */
#define CDA_NMT_ROOT_SIZE 90   /* 2*NamespaceSize + sha256.Size */
#define CDA_HASH_SIZE 32

enum {
    CDA_OK = 0,
    CDA_ERR_NOT_POW2 = -1,      /* "number of shares is not a power of 2: got %d" (data_availability_header.go:68) */
    CDA_ERR_CHUNK_SIZE = -2,    /* rsmt2d LeoRSCodec.ValidateChunkSize: "chunkSize %v must be a multiple of 64 bytes" */
    CDA_ERR_PUSH_ORDER = -3,    /* nmt ErrInvalidPushOrder on a Q0 row/column (surfaces from RowRoots/ColRoots) */
    CDA_ERR_DEVICE = -4,        /* HIP runtime / kernel launch failure */
    CDA_ERR_OOM = -5,           /* device allocation failure */
    CDA_ERR_INVALID = -6,       /* bad argument (NULL pointer, k out of range, ...) */
    CDA_ERR_UNSUPPORTED = -7,   /* shard count the codec does not support */
    CDA_ERR_SQUARE = -8,        /* go-square square.Construct / Build error (message from cda_last_error) */
    CDA_ERR_BYZANTINE = -9,     /* rsmt2d ErrByzantineData ("byzantine row: %d" / "byzantine col: %d") */
    CDA_ERR_UNREPAIRABLE = -10, /* rsmt2d ErrUnrepairableDataSquare ("failed to solve data square") /
                                   reedsolomon ErrTooFewShards */
    CDA_ERR_COMM = -11          /* an RCCL call failed: the context's communicator was aborted and
                                   released; every rank must call cda_comm_init again */
};

typedef struct cda_ctx cda_ctx;

/* ---- Square widths --------------------------------------------------------------
 * The calls that extend, hash, prove and sample take squares of ODS width
 * k = 1 .. 1024 (a power of two; EDS width 2k <= 2048).  A wider square is
 * answered with CDA_ERR_INVALID, "square width must be a power of two <=
 * 1024", before a buffer is read or staged: cda_extend_shares,
 * cda_dah_from_eds, cda_extend_dah, cda_extend_dah_batch[_ex],
 * cda_extend_dah_device, cda_extend_dah_inplace_device, cda_reserve,
 * cda_square_create, cda_square_set_create[_device], cda_sample_proofs_verify,
 * cda_namespace_proofs_verify[_set], cda_axis_halves_verify.  The host plans name the width ("square
 * width 2048 is not a power of two <= 1024"), cda_split_rows / cda_split_cols
 * answer "bad row block" / "bad column block".  cda_rs_encode and
 * cda_rs_recover_data take up to 1024 data shards, cda_data_root up to 2048 roots per axis (CDA_ERR_UNSUPPORTED
 * above).
 * Repair and the fraud proofs stop at k = 512 (EDS width 1024): cda_repair*,
 * cda_repair_batch* and cda_befp_build* answer EDS width 2048 with
 * CDA_ERR_INVALID, "EDS width must be a power of two in [2, 1024]",
 * cda_befp_verify / cda_befp_batch_check a batch of k = 1024 with
 * CDA_ERR_INVALID, and cda_rs_decode 1024 data shards with
 * CDA_ERR_UNSUPPORTED, "shard count must be a power of two <= 512". */

/* Context lifecycle. device: HIP ordinal (-1 = current device). */
int cda_ctx_create(int device, cda_ctx **out);
int cda_ctx_destroy(cda_ctx *ctx);
/* Message of the calling thread's last call (never NULL; "" after success).
 * Thread-local, so a concurrent call on the same context from another thread
 * cannot change or free it; a cgo caller reads it in the same C call or under
 * runtime.LockOSThread. */
const char *cda_last_error(cda_ctx *ctx);
/* Library version string, e.g. "cda 0.1.0 gfx950". */
const char *cda_version(void);

/* da.ExtendShares: ods = k*k*512 bytes (k a power of two, k >= 1);
 * eds = (2k)^2*512 bytes. n_shares is len(s) (checked for power of two). */
int cda_extend_shares(cda_ctx *ctx, const uint8_t *ods, uint32_t n_shares, uint8_t *eds);

/* da.NewDataAvailabilityHeader on an existing EDS of width w = 2k:
 * row_roots, col_roots = w*90 bytes each; data_root = 32 bytes (DAH.Hash()).
 * Returns CDA_ERR_PUSH_ORDER if a Q0 row or column is not namespace ordered. */
int cda_dah_from_eds(cda_ctx *ctx, const uint8_t *eds, uint32_t w, uint8_t *row_roots, uint8_t *col_roots,
                     uint8_t *data_root);

/* ExtendShares + NewDataAvailabilityHeader in one device submission. eds may be
 * NULL when the caller only needs the roots. On CDA_ERR_PUSH_ORDER the EDS is
 * still written (ExtendShares succeeds; the error belongs to the DAH step), and
 * so are the roots and data root: those of the reference's fraud tooling,
 * NewDataAvailabilityHeader over test/util/malicious/tree.go's BlindTrees (no
 * order check; the hashing never depends on it).  The same holds per square in
 * the batch entry points. */
int cda_extend_dah(cda_ctx *ctx, const uint8_t *ods, uint32_t n_shares, uint8_t *eds, uint8_t *row_roots,
                   uint8_t *col_roots, uint8_t *data_root);

/* Batch of n squares of width k, contiguous: ods = n*k*k*512, eds = n*(2k)^2*512
 * (or NULL), row_roots/col_roots = n*2k*90, data_roots = n*32. status (may be
 * NULL) receives one CDA_OK / CDA_ERR_PUSH_ORDER per square; the call returns
 * CDA_ERR_PUSH_ORDER if any square failed. */
int cda_extend_dah_batch(cda_ctx *ctx, const uint8_t *ods, uint32_t k, uint32_t n, uint8_t *eds, uint8_t *row_roots,
                         uint8_t *col_roots, uint8_t *data_roots, int32_t *status);

/* cda_extend_dah_batch with a choice of what goes back into eds (NULL: roots
 * only, as before):
 *   CDA_EDS_FULL     eds = n*(2k)^2*512, the whole EDS (= cda_extend_dah_batch);
 *                    the library copies Q0 from ods on host threads;
 *   CDA_EDS_SKIP_Q0  the same buffer, Q0 left untouched: a cgo caller that
 *                    wraps the EDS with rsmt2d.ImportExtendedDataSquare points
 *                    the Q0 cells at its own shares (it holds them already),
 *                    which saves the host copy of Q0;
 *   CDA_EDS_PARITY   eds = n*3*k^2*512 packed parity: per square Q1 as k rows
 *                    of k shares ([k][k][512]), then EDS rows k..2k-1 whole
 *                    ([k][2k][512]); Q0 is the caller's ODS.  The device packs
 *                    each chunk and returns it in one linear copy.
 * Reference: pkg/da/data_availability_header.go:65-75 (ExtendShares returns
 * the EDS whose Q0 cells are the input shares). */
#define CDA_EDS_FULL 0
#define CDA_EDS_SKIP_Q0 1
#define CDA_EDS_PARITY 2
int cda_extend_dah_batch_ex(cda_ctx *ctx, const uint8_t *ods, uint32_t k, uint32_t n, uint8_t *eds, int eds_mode,
                            uint8_t *row_roots, uint8_t *col_roots, uint8_t *data_roots, int32_t *status);

/* Device-resident batch: every pointer is device memory on ctx's device;
 * stream is a hipStream_t; NULL is HIP's default (null) stream, the one a
 * PyTorch/Go caller enqueues on by default -- NOT the context's private
 * stream, so the call is ordered after the caller's own work. Asynchronous: the
 * call only enqueues work. Per-square push-order status is written to d_status
 * (n int32, device memory, may be NULL).
 * Alignment: d_ods, d_eds 16 bytes; d_row_roots, d_col_roots 2; d_data_roots
 * 4; d_status 4.  d_ods is read only; exactly n*(2k)^2*512, n*2k*90 (twice),
 * n*32 and n*4 bytes are written. */
int cda_extend_dah_device(cda_ctx *ctx, const void *d_ods, uint32_t k, uint32_t n, void *d_eds, void *d_row_roots,
                          void *d_col_roots, void *d_data_roots, int32_t *d_status, void *stream);

/* Size the context's scratch for device batches of up to n squares of width
 * k (synchronous).  Scratch buffers only grow; inside a call a growing buffer
 * is released and reallocated in stream order on the call's stream
 * (hipFreeAsync / hipMallocAsync: no device synchronisation), so device entry
 * points stay enqueue-only either way; cda_reserve just moves the allocations
 * out of the first calls. */
int cda_reserve(cda_ctx *ctx, uint32_t k, uint32_t n);

/* As cda_extend_dah_device, but the k*k ODS shares are already in place in
 * quadrant Q0 of d_eds (row r, column c at (r*2k + c)*512 of each square),
 * the layout rsmt2d's EDS has after ExtendShares.  The cgo caller flattens the
 * [][]byte shares straight into that arena (it must copy them into one flat
 * buffer anyway), so the kernels read Q0 where it lies and never copy it.
 * Outputs and semantics are identical to cda_extend_dah_device; Q0 of d_eds is
 * read only, the three parity quadrants are written.
 * Alignment: d_eds 16 bytes; d_row_roots, d_col_roots 2; d_data_roots 4;
 * d_status 4. */
int cda_extend_dah_inplace_device(cda_ctx *ctx, uint32_t k, uint32_t n, void *d_eds, void *d_row_roots,
                                  void *d_col_roots, void *d_data_roots, int32_t *d_status, void *stream);

/* rsmt2d Codec.Encode (Leopard, GF(2^8) for 2*n_shards <= 256, else GF(2^16)):
 * n_codewords codewords, each n_shards data shards of shard_len bytes,
 * contiguous; parity has the same shape.  n_shards <= 1024 ("more than 2048
 * shards", CDA_ERR_UNSUPPORTED, above); a count that is no power of two is
 * padded with zero shards up to the next one, as klauspost's encoder does. */
int cda_rs_encode(cda_ctx *ctx, const uint8_t *data, uint32_t n_shards, uint32_t shard_len, uint32_t n_codewords,
                  uint8_t *parity);

/* (*DataAvailabilityHeader).Hash: RFC-6962 root of row_roots || col_roots
 * (w roots of 90 bytes each, w a power of two <= 2048). w == 0 gives
 * sha256("") like Hash() on a nil DAH. */
int cda_data_root(cda_ctx *ctx, const uint8_t *row_roots, const uint8_t *col_roots, uint32_t w, uint8_t *data_root);

/* Details of the calling thread's last CDA_ERR_PUSH_ORDER: axis (0 row, 1
 * column), the axis index, and the leaf position whose push failed. */
int cda_push_order_detail(cda_ctx *ctx, int32_t *axis, uint32_t *index, uint32_t *position);
/* The same detail for square `square` of the context's last device batch
 * (cda_extend_dah_device / cda_extend_dah_inplace_device), whose d_status
 * carries only CDA_ERR_PUSH_ORDER: waits for that batch's GPU work, then
 * decodes the square's first violation (axis -1 when the square is ordered).
 * Valid until the next device batch on the context.  A block-replay caller
 * (app/process_proposal.go:138-147) builds the rejection text from it. */
int cda_push_order_detail_at(cda_ctx *ctx, uint32_t square, int32_t *axis, uint32_t *index, uint32_t *position);

/* Config 5: ONE square split across G ranks (one GPU each), row blocks +
 * column blocks.  k = ODS width, W = 2k, R = k/G rows and C = W/G columns per
 * rank.  All pointers are device memory; calls only enqueue on `stream`
 * (NULL = HIP's default stream, as for cda_extend_dah_device).
 * d_err is one uint32 per rank, initialised by the caller to 0xFFFFFFFF;
 * push-order violations atomically lower it (encoding: axis<<24 | index<<12 |
 * position, reduce with MIN across ranks).
 *  1. cda_split_rows: ODS rows [row0, row0+R) (R x k shares, row-major) ->
 *     row block (R x W shares: Q0 row | Q1 row), plus the Q0 row-order check.
 *  2. caller: all-to-all of the row blocks' column slices (RCCL) so rank g
 *     holds rows 0..k-1 of columns [g*C, g*C+C) as a W x C share block.
 *  3. cda_split_cols: column-encode the block (Q0->Q2 / Q1->Q3), hash each
 *     cell once, write the C column roots and, per EDS row, the NMT subtree
 *     node over this rank's C columns (96-B slots, W of them).
 *  4. caller: gather the subtree slots ([G][W][96]) and column root slots
 *     ([W][96], rank order) on one rank.
 *  5. cda_split_combine: top log2(G) levels of every row tree, pack roots,
 *     data root.
 * Alignment: d_ods_rows, d_row_block, d_col_block, d_send 16 bytes;
 * d_col_root_slots, d_row_subtree_slots 16; d_err 4 (exactly one word is
 * written); d_row_roots, d_col_roots 2; d_data_root 4. */
int cda_split_rows(cda_ctx *ctx, const void *d_ods_rows, uint32_t k, uint32_t n_rows, uint32_t row0,
                   void *d_row_block, uint32_t *d_err, void *stream);
int cda_split_cols(cda_ctx *ctx, void *d_col_block, uint32_t k, uint32_t n_cols, uint32_t col0,
                   void *d_col_root_slots, void *d_row_subtree_slots, uint32_t *d_err, void *stream);
int cda_split_combine(cda_ctx *ctx, const void *d_row_subtree_slots, uint32_t parts, uint32_t k,
                      const void *d_col_root_slots, void *d_row_roots, void *d_col_roots, void *d_data_root,
                      void *stream);

/* ---- Multi-GPU inside the library ---------------------------
 * Config 5 with the library's own RCCL collectives (no torch.distributed in the
 * host): rank 0 makes an id (cda_comm_unique_id, 128 bytes) and hands it to
 * every rank out of band; each rank's context joins (cda_comm_init, one context
 * per GPU, all ranks call it together); cda_extend_dah_split then runs the
 * whole split of ONE square on `stream`: rows into the all-to-all send layout,
 * a grouped ncclSend/ncclRecv all-to-all, column encode + hashing, a gather of
 * the subtree / column-root slots and a MIN reduce of the push-order word to
 * rank 0, which writes the roots and the data root.  Every rank must call it.
 *   d_ods_rows: this rank's R = k/G ODS rows (R*k shares, device);
 *   d_col_block: W x C shares (device, may be NULL = library scratch): the EDS
 *     columns [rank*C, rank*C + C) on return (row-major [W][C][512]);
 *   d_row_roots / d_col_roots (W*90) / d_data_root (32): rank 0 only;
 *   d_err: one device uint32, on rank 0 the MIN over ranks of the push-order
 *     words (0xFFFFFFFF = ordered; axis<<24 | index<<12 | position; 0 = a rank
 *     failed locally: rank 0 then returns CDA_ERR_DEVICE and writes no roots).
 * Alignment: d_ods_rows, d_col_block 16 bytes; d_row_roots, d_col_roots 2;
 * d_data_root 4; d_err 4. */
#define CDA_COMM_ID_BYTES 128
int cda_comm_unique_id(uint8_t id[CDA_COMM_ID_BYTES]);
int cda_comm_init(cda_ctx *ctx, int rank, int world, const uint8_t id[CDA_COMM_ID_BYTES]);
int cda_comm_destroy(cda_ctx *ctx);
/* The live communicator's rank and rank count as RCCL formed them
 * (ncclCommUserRank / ncclCommCount); CDA_ERR_INVALID without one. */
int cda_comm_size(cda_ctx *ctx, int *rank, int *world);
/* ncclCommAbort of the context's communicator (then released).  Takes no
 * context lock, so a host watchdog may call it from another thread while a
 * call on the context waits in a collective for a peer that failed.  Errors
 * of cda_extend_dah_split: checks that depend on k / the world size fail on
 * every rank before any collective; scratch is sized when k changes, followed
 * by one agreement all-reduce, so an allocation failure on any rank makes
 * every rank return CDA_ERR_OOM; a local failure after that keeps the rank in
 * the remaining collectives with its push-order word poisoned to 0 and returns
 * the rank's error; rank 0 reads the reduced word back and, when it is 0 (a
 * peer failed), returns CDA_ERR_DEVICE without writing roots; a failed RCCL
 * call closes its group, aborts the communicator and returns CDA_ERR_COMM, and
 * so does a call that cda_comm_abort released while it waited in a collective
 * (every RCCL post re-reads the communicator under a lock that the abort also
 * takes, so no call touches an aborted communicator). */
int cda_comm_abort(cda_ctx *ctx);
int cda_extend_dah_split(cda_ctx *ctx, const void *d_ods_rows, uint32_t k, void *d_col_block, void *d_row_roots,
                         void *d_col_roots, void *d_data_root, uint32_t *d_err, void *stream);
/* Step 1 of the split for a caller that runs its own all-to-all (e.g. over
 * torch.distributed): the row block of R ODS rows written straight in the send
 * layout [parts][R][C][512] (part h = columns [h*C, h*C + C)), so the received
 * pieces ARE rows 0..k-1 of the receiver's column block.
 * Alignment: d_ods_rows, d_send 16 bytes; d_err 4. */
int cda_split_rows_send(cda_ctx *ctx, const void *d_ods_rows, uint32_t k, uint32_t n_rows, uint32_t row0,
                        uint32_t parts, void *d_send, uint32_t *d_err, void *stream);
/* The split's buffer arithmetic (host only, no context; csrc/split_layout.h,
 * the same functions the group-rows kernel and cda_extend_dah_split use), so a
 * host can size its buffers and a test can replay the G > 1 exchange on the
 * CPU.  Byte sizes / offsets: the all-to-all piece of one rank pair, the send
 * buffer [G][R][C][512], the column block [W][C][512], and in the slot area
 * (96-B NMT node slots) the rank's C column roots, its W row subtree nodes,
 * (rank 0) the gathered [G][W] subtrees and [W] column roots, the push-order
 * word.  CDA_ERR_INVALID unless k and world are powers of two, world | k. */
typedef struct {
    uint32_t k, world, W, R, C;
    uint64_t piece_bytes, send_bytes, col_block_bytes;
    uint64_t col_slots_off, row_sub_off, gather_sub_off, gather_col_off, err_off, slots_bytes;
} cda_split_layout_t;
int cda_split_layout(uint32_t k, uint32_t world, cda_split_layout_t *out);
/* n offsets at once, off[i] for (a[i], b[i]) (b may be NULL when unused):
 *   CDA_SPLIT_SEND        send-buffer byte offset of row-block cell (r = a, col = b)
 *   CDA_SPLIT_SEND_PIECE  send-buffer byte offset of the piece for rank a
 *   CDA_SPLIT_RECV_PIECE  column-block byte offset where rank a's piece lands
 *   CDA_SPLIT_BLOCK       column-block byte offset of EDS row a, local column b
 *   CDA_SPLIT_GATHER_SUB  slot-area byte offset of rank a's W row subtrees (rank 0)
 *   CDA_SPLIT_GATHER_COL  slot-area byte offset of rank a's C column roots (rank 0)
 *   CDA_SPLIT_COMBINE     slot index, in the gathered subtrees, of rank a's node of row b
 * CDA_ERR_INVALID (nothing written) for an unknown kind, an index out of its
 * range (r < R, col < W, row < W, c < C, ranks < world) or b NULL where read. */
#define CDA_SPLIT_SEND 0
#define CDA_SPLIT_SEND_PIECE 1
#define CDA_SPLIT_RECV_PIECE 2
#define CDA_SPLIT_BLOCK 3
#define CDA_SPLIT_GATHER_SUB 4
#define CDA_SPLIT_GATHER_COL 5
#define CDA_SPLIT_COMBINE 6
int cda_split_offsets(uint32_t k, uint32_t world, int what, uint32_t n, const uint32_t *a, const uint32_t *b,
                      uint64_t *off);
/* Config 4 on one node: n independent squares (host buffers, as
 * cda_extend_dah_batch) split into contiguous shards over n_ctx contexts (one
 * per GPU) and run concurrently on host threads; no collective. */
int cda_extend_dah_multi(cda_ctx *const *ctxs, uint32_t n_ctx, const uint8_t *ods, uint32_t k, uint32_t n,
                         uint8_t *eds, uint8_t *row_roots, uint8_t *col_roots, uint8_t *data_roots, int32_t *status);

/* ---- Data-square construction ----------------------
 * go-square v1.1.0 square.Construct (mode CDA_SQUARE_CONSTRUCT; used by
 * ProcessProposal app/process_proposal.go:122-126 and ExtendBlock
 * app/extend_block.go:16-20) and square.Build (mode CDA_SQUARE_BUILD;
 * PrepareProposal app/prepare_proposal.go:50-53).  Construct fails on a tx
 * that does not fit or a normal tx after a blob tx; Build skips txs that do
 * not fit and returns the kept ones.
 *   txs, tx_off: the block's n_txs transactions concatenated; tx i is
 *     txs[tx_off[i] .. tx_off[i+1]) (tx_off has n_txs + 1 entries).
 *   max_square_size: appconsts.SquareSizeUpperBound / GovMaxSquareSize
 *     (power of two); threshold: appconsts.SubtreeRootThreshold (64).
 *   square_size: out, the ODS width k (dataSquare.Size()).
 *   kept (n_txs entries, may be NULL) / n_kept: indexes of the txs in the
 *     square in block order (normal txs, then blob txs) -- Build's txs result.
 * Errors: CDA_ERR_SQUARE with go-square's message (cda_last_error). */
#define CDA_SQUARE_CONSTRUCT 0
#define CDA_SQUARE_BUILD 1

/* Layout only, on the host (no device work; ctx may be NULL, then the error
 * message is cda_last_error(NULL) of the calling thread).  share_indexes
 * receives the start share of every blob, per PFB in square order and blob
 * order within the PFB (the IndexWrapper.share_indexes written to the square). */
int cda_square_layout(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                      uint32_t max_square_size, uint32_t threshold, int mode, uint32_t *square_size, uint32_t *kept,
                      uint32_t *n_kept, uint32_t *share_indexes, uint32_t share_index_cap, uint32_t *n_share_indexes);

/* go-square builder.FindTxShareRange for the square.Construct layout of txs
 * (pkg/proof/proof.go:22-49 NewTxInclusionProof): the shares [start, end) of
 * the square holding kept tx tx_index (normal txs, then blob txs as their
 * IndexWrapper in the PFB namespace; *is_pfb says which).  Equal txs report
 * the last copy's range (the splitters key ranges by tx hash).  Host only;
 * ctx may be NULL.  CDA_ERR_INVALID "txIndex %u out of range". */
int cda_square_tx_share_range(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                              uint32_t max_square_size, uint32_t threshold, uint32_t tx_index, uint32_t *start,
                              uint32_t *end, int *is_pfb);

/* cda_square_tx_share_range for n kept txs at once: the square is laid out once, then starts[i],
 * ends[i] and is_pfb[i] (n bytes, may be NULL) answer tx_indexes[i].  An index out of range fails
 * the call as above, nothing written.  Host only; ctx may be NULL. */
int cda_square_tx_share_ranges(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                               uint32_t max_square_size, uint32_t threshold, const uint32_t *tx_indexes, uint32_t n,
                               uint32_t *starts, uint32_t *ends, uint8_t *is_pfb);

/* The square's k*k shares (row-major) into ods (host, ods_capacity bytes;
 * max_square_size^2 * 512 always suffices).  Shares are written on the GPU. */
int cda_square_construct(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                         uint32_t max_square_size, uint32_t threshold, int mode, uint8_t *ods, size_t ods_capacity,
                         uint32_t *square_size, uint32_t *kept, uint32_t *n_kept);

/* Construct + ExtendShares + NewDataAvailabilityHeader in one submission (the
 * proposal paths' whole DA step); the ODS never leaves HBM.  eds may be NULL;
 * row_roots / col_roots hold roots_capacity bytes each (2 * max_square_size *
 * 90 always suffices); data_root = 32 bytes. */
int cda_construct_extend_dah(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                             uint32_t max_square_size, uint32_t threshold, int mode, uint8_t *eds, size_t eds_capacity,
                             uint8_t *row_roots, uint8_t *col_roots, size_t roots_capacity, uint8_t *data_root,
                             uint32_t *square_size, uint32_t *kept, uint32_t *n_kept);

/* Device variant: the layout is planned from the host txs, the shares are
 * written from d_txs (a device copy of the same bytes with >= 16 readable
 * bytes after the end) into d_ods; only enqueues on stream (NULL = HIP's
 * default stream).  The bytes read after the end never reach the shares: a
 * blob's last share is zero-padded whatever follows d_txs.  Of d_ods exactly
 * square_size^2 * 512 bytes are written, whatever ods_capacity is.
 * Alignment: d_txs 4 bytes; d_ods 8. */
int cda_square_construct_device(cda_ctx *ctx, const uint8_t *txs, const uint64_t *tx_off, uint32_t n_txs,
                                const void *d_txs, uint32_t max_square_size, uint32_t threshold, int mode,
                                void *d_ods, size_t ods_capacity, uint32_t *square_size, uint32_t *kept,
                                uint32_t *n_kept, void *stream);

/* ---- Blob share commitments --------------------------
 * go-square v1.1.0 inclusion.CreateCommitment(blob, merkle.HashFromByteSlices,
 * threshold) for n blobs at once (x/blob/types/blob_tx.go:98 ValidateBlobTx;
 * x/blob/types/payforblob.go:53 CreateCommitments).
 *   namespaces: n * 29 bytes (version || id); blob i's data is
 *     data[data_off[i] .. data_off[i+1]) (data_off has n + 1 entries);
 *   share_versions: n bytes or NULL (all ShareVersionZero);
 *   threshold: appconsts.SubtreeRootThreshold (64);
 *   commitments: n * 32 bytes.
 * A blob with empty data commits to sha256("") (no shares).  Invalid share
 * versions / namespaces: CDA_ERR_SQUARE with go-square's message. */
int cda_blob_commitments(cda_ctx *ctx, const uint8_t *namespaces, const uint8_t *data, const uint64_t *data_off,
                         const uint8_t *share_versions, uint32_t n, uint32_t threshold, uint8_t *commitments);
/* Device variant: d_data is a device copy of the blob bytes with >= 16
 * readable bytes after the end, d_commitments is device memory; namespaces /
 * offsets / versions stay on the host (the layout is planned there).  Only
 * enqueues on stream (NULL = HIP's default stream).  The bytes read after the
 * end never reach a commitment.
 * Alignment: d_data 4 bytes; d_commitments 4 (n*32 bytes written). */
int cda_blob_commitments_device(cda_ctx *ctx, const uint8_t *namespaces, const uint64_t *data_off,
                                const uint8_t *share_versions, uint32_t n, uint32_t threshold, const void *d_data,
                                void *d_commitments, void *stream);

/* ---- Resident squares: NMT proofs and commitments from cached nodes -------
 * (SURVEY.md 8(f) row 3).  cda_square_create extends one ODS and keeps in HBM
 * the EDS, every level of every row tree (the reference's
 * EDSSubTreeRootCacher, pkg/inclusion/nmt_caching.go:80-124) and all levels
 * of the data-root tree, so a proof is index arithmetic and one launch.
 * On CDA_ERR_PUSH_ORDER the handle is still created (the EDS exists). */
typedef struct cda_square cda_square;
int cda_square_create(cda_ctx *ctx, const uint8_t *ods, uint32_t n_shares, cda_square **out);
int cda_square_destroy(cda_square *sq);
/* Any output may be NULL: k, row/col roots (2k*90 each), data root (32), EDS ((2k)^2*512). */
int cda_square_dah(cda_square *sq, uint32_t *k, uint8_t *row_roots, uint8_t *col_roots, uint8_t *data_root,
                   uint8_t *eds);
/* proof.NewShareInclusionProofFromEDS (pkg/proof/proof.go:77-145) for the ODS
 * share range [start, end) (row-major ODS indexes), R = end_row - start_row + 1
 * rows, A = log2(4k) aunts, M = 2*log2(2k) node slots per row:
 *   shares        (end - start) * 512: ShareProof.Data, concatenated
 *   nmt_start/end R entries: NMTProof.Start / End (leaf range in the row)
 *   nmt_count     R entries; nmt_nodes R*M*90 B: NMTProof.Nodes of row i at
 *                 [i*M*90, ...) (nmt ProveRange order: maximal subtrees outside
 *                 the range, left to right); NMTProof.LeafHash is empty (only
 *                 cda_square_namespace_proofs' absence segments carry one)
 *   row_roots     R*90: RowProof.RowRoots
 *   row_leaf_hash R*32, row_aunts R*A*32: RowProof.Proofs (merkle proofs of
 *                 the rows among rowRoots || colRoots: Total 4k, Index = row,
 *                 LeafHash, Aunts bottom-up) */
int cda_square_share_proof(cda_square *sq, uint32_t start, uint32_t end, uint8_t *shares, uint32_t *start_row,
                           uint32_t *end_row, int32_t *nmt_start, int32_t *nmt_end, uint32_t *nmt_count,
                           uint8_t *nmt_nodes, uint8_t *row_roots, uint8_t *row_leaf_hash, uint8_t *row_aunts);
/* inclusion.GetCommitment (pkg/inclusion/get_commit.go:12-30) for n blobs:
 * blob i starts at ODS share starts[i] (normalised by NextShareIndex as the
 * reference does) and spans share_lens[i] shares; commitments n*32. */
int cda_square_blob_commitments(cda_square *sq, const uint32_t *starts, const uint32_t *share_lens, uint32_t n,
                                uint32_t threshold, uint8_t *commitments);
/* EDSSubTreeRootCacher.getSubTreeRoot (pkg/inclusion/nmt_caching.go:111-124):
 * the 90-B node of row tree `row` (0 <= row < 2k) reached from its root by
 * walk[0 .. walk_len) (0 = WalkLeft, 1 = WalkRight; GetCommitment prefixes
 * WalkLeft for the ODS half).  A walk longer than the tree's depth fails with
 * the cache's "did not find sub tree root: [...]" (root still receives the
 * leaf it reached); row >= 2k: "row exceeds range of cache: max %d got %d". */
int cda_square_subtree_root(cda_square *sq, uint32_t row, const uint8_t *walk, uint32_t walk_len, uint8_t *root);

/* ---- Data-availability samples: serve and check cells of the EDS ------------
 * What a full node does with an EDS after building it: answer samples of any
 * of its cells, parity included, each proved against the row or the column
 * root.  The square also keeps every level of every column tree for this. */
#define CDA_AXIS_ROW 0
#define CDA_AXIS_COL 1
/* n samples of the EDS of a resident square.  Sample i is cell (rows[i], cols[i]), 0 <= both < 2k, proved
 * against the row root (axes[i] == 0) or the column root (1); axes == NULL means all rows.
 * D = log2(2k) proof nodes and A = log2(4k) aunts per sample, fixed strides, any output may be NULL:
 *   shares      n*512    the cell
 *   namespaces  n*29     the leaf namespace: share[0:29] if row < k && col < k, else ParitySharesNamespace
 *   nmt_nodes   n*D*90   nmt ProveRange(p, p+1) of the axis tree, p = col (row axis) or row (column axis):
 *                        left siblings top-down, then right siblings bottom-up
 *   axis_roots  n*90     the row / column root
 *   leaf_hash   n*32, aunts n*A*32   merkle proof of that root among rowRoots || colRoots:
 *                        Total 4k, Index = row (row axis) or 2k + col (column axis), aunts bottom-up
 * Coordinates are checked on the host before anything is enqueued: CDA_ERR_INVALID naming the sample and
 * the field, outputs untouched.  n == 0 returns CDA_OK.  One launch per call, whatever n; host buffers,
 * complete when the call returns.  A square created with CDA_ERR_PUSH_ORDER serves samples like any other. */
int cda_square_sample_proofs(cda_square *sq, const uint32_t *rows, const uint32_t *cols, const uint8_t *axes,
                             uint32_t n, uint8_t *shares, uint8_t *namespaces, uint8_t *nmt_nodes,
                             uint8_t *axis_roots, uint8_t *leaf_hash, uint8_t *aunts);
/* The verifying side of cda_square_sample_proofs for a square of ODS width k: same arrays, plus one data
 * root per sample (n*32).  The namespace, the leaf position and the merkle Index/Total are derived from
 * (row, col, axis) here, never taken from the prover.  verdict[i]: 0 valid, 1 the axis root does not
 * verify against the data root, 2 the cell does not verify against the axis root (1 wins).
 * Coordinates out of range, or k not a power of two <= 1024: CDA_ERR_INVALID, verdict untouched.
 * Cells with verdict 0 are what cda_repair's `present` mask is meant to be filled from. */
int cda_sample_proofs_verify(cda_ctx *ctx, uint32_t k, uint32_t n, const uint8_t *data_roots,
                             const uint32_t *rows, const uint32_t *cols, const uint8_t *axes,
                             const uint8_t *shares, const uint8_t *nmt_nodes, const uint8_t *axis_roots,
                             const uint8_t *leaf_hash, const uint8_t *aunts, uint8_t *verdict);

/* ---- Sets of resident squares: built from a batch, sampled across ----------------
 * What cda_square_create keeps for one square, built for n squares of one ODS width k in ONE submission
 * (no per-square launch or copy), from a batch that lies on the host or is already in HBM: the output
 * of cda_extend_dah_device / _inplace_device, a replayed batch, the squares cda_repair_batch_device
 * repaired.  src / device_src holds
 *   CDA_SET_FROM_ODS  n*k*k*512 bytes: every square is extended, then hashed;
 *   CDA_SET_FROM_EDS  n*(2k)^2*512 bytes: the squares are copied and hashed as they are.  NO Reed-Solomon
 *                     work is done and the parity is NOT checked: the roots commit to the bytes given,
 *                     as NewDataAvailabilityHeader(eds) and cda_dah_from_eds do.  A caller that does not
 *                     trust the source compares cda_square_set_dah's data roots with the ones it trusts.
 * The set owns one arena per part (EDS, row and column tree levels, root slots, RFC-6962 levels, packed
 * roots, data roots, push-order words), square i at base + i * stride with 64-bit offsets, so a set may be
 * larger than 4 GiB per arena; it costs about 1.6 x the EDS bytes of HBM, plus the leaf staging
 * (n*(2k)^2*96) and, for a host ODS source, the uploaded batch while it is built.
 * Push order is per square: an unordered square stays in the set with its blind roots, its status is
 * CDA_ERR_PUSH_ORDER, the create call returns CDA_ERR_PUSH_ORDER (text and cda_push_order_detail: the first
 * such square) and STILL returns the set, as cda_square_create does; cda_push_order_detail_at(ctx, i, ...)
 * names square i's first violation until the next device batch on the context.
 * Both calls return when the set is complete.  The device variant orders its work after `stream` (NULL:
 * the null stream) and waits for its own work only; device_src is read only, 16-byte aligned, and may be
 * released on return.  CDA_ERR_INVALID, *out = NULL and nothing allocated: n == 0 or n >
 * CDA_SET_MAX_SQUARES, k not a power of two <= 1024, an unknown kind, a NULL pointer. */
#define CDA_SET_FROM_ODS 0
#define CDA_SET_FROM_EDS 1
#define CDA_SET_MAX_SQUARES 65535
typedef struct cda_square_set cda_square_set;
int cda_square_set_create(cda_ctx *ctx, const uint8_t *src, int kind, uint32_t k, uint32_t n, cda_square_set **out);
int cda_square_set_create_device(cda_ctx *ctx, const void *device_src, int kind, uint32_t k, uint32_t n, void *stream,
                                 cda_square_set **out);
/* Ends the set and its members (handles from cda_square_set_at are dead afterwards). */
int cda_square_set_destroy(cda_square_set *set);
int cda_square_set_info(cda_square_set *set, uint32_t *k, uint32_t *n);   /* either may be NULL */
/* Square i of the set as a cda_square, BORROWED: its buffers are views into the set's arenas (only the
 * per-call scratch is its own), every cda_square_* call works on it, it lives as long as the set, and
 * cda_square_destroy on it is CDA_ERR_INVALID and leaves set and member intact.  i >= n: CDA_ERR_INVALID. */
int cda_square_set_at(cda_square_set *set, uint32_t i, cda_square **member);
/* Any output may be NULL: row_roots, col_roots n*2k*90 each (square by square), data_roots n*32,
 * status n (CDA_OK / CDA_ERR_PUSH_ORDER).  Host buffers, complete on return. */
int cda_square_set_dah(cda_square_set *set, uint8_t *row_roots, uint8_t *col_roots, uint8_t *data_roots,
                       int32_t *status);
/* cda_square_sample_proofs across the set: sample i is cell (rows[i], cols[i]) of member squares[i] on axis
 * axes[i] (NULL: all rows).  All members share k, so D, A, the six outputs and their strides are those of
 * cda_square_sample_proofs and cda_sample_proofs_verify takes the arrays as they are (with each sample's
 * own data root).  One launch, one upload of the requests and one copy back per requested output, whatever
 * n and however many squares are named.  Validated on the host before anything is enqueued:
 * CDA_ERR_INVALID naming the sample and the field (square, row, col or axis), outputs untouched.
 * n == 0 returns CDA_OK. */
int cda_square_set_sample_proofs(cda_square_set *set, const uint32_t *squares, const uint32_t *rows,
                                 const uint32_t *cols, const uint8_t *axes, uint32_t n, uint8_t *shares,
                                 uint8_t *namespaces, uint8_t *nmt_nodes, uint8_t *axis_roots, uint8_t *leaf_hash,
                                 uint8_t *aunts);

/* ---- Share-inclusion proofs of many ranges in one launch -----------------------
 * proof.NewShareInclusionProofFromEDS (pkg/proof/proof.go:77-145) for n ranges [starts[i], ends[i]) of
 * the ODS of one resident square at once, in the flat layout of cda_share_proof_batch below: the
 * arrays of cda_share_proofs_out carry that struct's field names and layouts, so a batch for
 * cda_share_proofs_verify is filled from them by pointer assignment (ns_len 29, share_len 512,
 * n_nodes / n_aunts / n_shares from the plan).  Proof i covers the rows start_row[i] .. end_row[i], one
 * segment per row; S segments in all.
 *
 * cda_square_share_proofs_plan: host only, no context (the message of an error is
 * cda_last_error(NULL) of the calling thread).  Checks the ranges and returns the sizes to allocate:
 *   n_segments = S, n_nodes, n_aunts = S * aunts_per_segment (log2(4k) each), n_shares.
 * CDA_ERR_INVALID, *out untouched, with a message naming the range and the field
 * ("range 3: end 70 is beyond the 64 shares of the original square") for start >= end, end > k*k, or
 * an offset that does not fit the batch's uint32_t offsets; also for k not a power of two <= 1024.
 * n == 0: CDA_OK, all sizes zero. */
typedef struct {
    uint32_t n_segments, n_nodes, n_aunts, aunts_per_segment;
    uint64_t n_shares;
} cda_share_proofs_plan_t;
int cda_square_share_proofs_plan(uint32_t k, const uint32_t *starts, const uint32_t *ends, uint32_t n,
                                 cda_share_proofs_plan_t *out);
/* Caller-allocated host buffers, any of them NULL (sizes from the plan).
 * Written by the host:
 *   seg_off n+1; nmt_start / nmt_end S; node_off S+1; aunt_off S+1; rfc_total S (all 4k);
 *   rfc_index S (the row); start_row / end_row n.
 * Written by the kernel:
 *   nodes n_nodes*90 (nmt ProveRange order per segment, packed); row_roots S*90; rfc_leaf_hash S*32;
 *   aunts n_aunts*32 (bottom-up); shares n_shares*512 (proof then segment order);
 *   namespaces n*29 (the first share's namespace);
 *   one_namespace n bytes: 1 if every share of the range carries the first share's namespace (what
 *   proof.ParseNamespace tests, pkg/proof/querier.go:134-166), else 0. */
typedef struct cda_share_proofs_out {
    uint32_t *seg_off;
    int32_t *nmt_start;
    int32_t *nmt_end;
    uint32_t *node_off;
    uint8_t *nodes;
    uint8_t *row_roots;
    int64_t *rfc_total;
    int64_t *rfc_index;
    uint8_t *rfc_leaf_hash;
    uint32_t *aunt_off;
    uint8_t *aunts;
    uint8_t *shares;
    uint8_t *namespaces;
    uint32_t *start_row;
    uint32_t *end_row;
    uint8_t *one_namespace;
} cda_share_proofs_out;
/* The ranges are checked as by the plan before anything is enqueued (CDA_ERR_INVALID, outputs
 * untouched).  One kernel launch per call, whatever n and the ranges' lengths; host buffers, complete
 * when the call returns.  A square created with CDA_ERR_PUSH_ORDER serves proofs like any other.
 * cda_square_share_proof returns the same bytes for one range per call. */
int cda_square_share_proofs(cda_square *sq, const uint32_t *starts, const uint32_t *ends, uint32_t n,
                            const cda_share_proofs_out *out);

/* ---- All shares of a namespace, with completeness proofs -----------------------
 * nmt v0.22.0 ProveNamespace and Proof.VerifyNamespace (VerifyLeafHashes with verifyCompleteness = true)
 * over the row trees of a resident square, and the row selection GetSharesByNamespace does on the DAH, for
 * n namespaces (29 bytes each) in one call.  Per query ns and row r:
 *   - r is selected iff min(rowRoot_r) <= ns <= max(rowRoot_r) (the square's own roots, IgnoreMaxNamespace);
 *     only rows < k can be, and rows that are not selected do not appear;
 *   - start = the leaves of the row with namespace < ns, end = start + those with namespace == ns;
 *   - kind 1 (inclusion, end > start): leaf range [start, end), the shares row[start:end] and the nodes of
 *     ProveRange(start, end) in cda_square_share_proofs' order;
 *   - kind 2 (absence, end == start, and then start < k): leaf range [start, start + 1), the nodes of
 *     ProveRange(start, start + 1), the 90-byte leaf node of leaf `start` (NMTProof.LeafHash), no shares.
 * A query's segments are in ascending row order; it may have none (ns below, above or between the rows).
 * The arrays carry cda_share_proofs_out's names and layouts where the meaning is the same (S segments in all):
 *   seg_off n+1; row S; kind S bytes; nmt_start / nmt_end S; node_off S+1; nodes n_nodes*90;
 *   share_off S+1 (in shares); shares n_shares*512; absence_leaf S*90 (zero for inclusion segments).
 *
 * cda_square_namespace_plan: the sizes to allocate.  It runs the search on the GPU: one launch, and one
 * word per (query, row < k) copied back (n*k*4 bytes).  n == 0: CDA_OK, all sizes zero.
 * cda_square_namespace_proofs: caller-allocated host buffers, any of them NULL; complete on return.  It
 * runs the search again (it keeps no state and trusts no table of the caller's): one search launch, one
 * host pass over the words, one launch of cda_square_share_proofs' kernel, whatever n and the run lengths.
 * Both: CDA_ERR_INVALID, outputs untouched, with a message naming the query for a query equal to
 * ParitySharesNamespace (29 x 0xFF) and for null arrays; a square created with CDA_ERR_PUSH_ORDER answers
 * CDA_ERR_PUSH_ORDER (nmt could not have built its trees), outputs untouched. */
typedef struct cda_namespace_plan_t {
    uint64_t n_segments, n_nodes, n_shares;
} cda_namespace_plan_t;
int cda_square_namespace_plan(cda_square *sq, const uint8_t *namespaces, uint32_t n, cda_namespace_plan_t *out);
typedef struct cda_namespace_proofs_out {
    uint32_t *seg_off;
    uint32_t *row;
    uint8_t *kind;
    int32_t *nmt_start;
    int32_t *nmt_end;
    uint32_t *node_off;
    uint8_t *nodes;
    uint64_t *share_off;
    uint8_t *shares;
    uint8_t *absence_leaf;
} cda_namespace_proofs_out;
int cda_square_namespace_proofs(cda_square *sq, const uint8_t *namespaces, uint32_t n,
                                const cda_namespace_proofs_out *out);
/* The verifying side, for a square of ODS width k whose DAH the caller trusts (row_roots: 2k*90).  The
 * arrays are the prover's, by pointer assignment; the row root of every segment is row_roots[row], never
 * the prover's.  verdict[q] (n_queries bytes), the lower number wins:
 *   0 valid;
 *   1 the answer's rows are not exactly the rows the DAH selects for the namespace, in ascending order;
 *   2 a segment does not hash to its row root (VerifyLeafHashes' root comparison; too few or too many
 *     nodes for the range too), or an absence segment's leaf does not have a min namespace > ns;
 *   3 the proof is incomplete: one of the first popcount(nmt_start) nodes (left of the range) has a max
 *     namespace >= ns, or a later node has a min namespace <= ns.
 * Checked on the host before anything is enqueued, CDA_ERR_INVALID with a message naming the query or the
 * segment and the field, verdict untouched: null arrays; a query equal to ParitySharesNamespace; offsets
 * that do not start at 0, decrease or do not end at the counts; kind not 1 or 2; not 0 <= nmt_start <
 * nmt_end <= 2k; an absence segment with nmt_end != nmt_start + 1; row >= 2k; share_off not the running
 * sum of the inclusion segments' lengths, or that sum not n_shares; k not a power of two <= 1024.
 * n_queries == 0 returns CDA_OK. */
#define CDA_NAMESPACE_INCLUSION 1
#define CDA_NAMESPACE_ABSENCE 2
typedef struct cda_namespace_proof_batch {
    uint32_t n_queries;
    const uint8_t *namespaces;     /* n_queries*29 */
    const uint32_t *seg_off;       /* n_queries+1; S = last */
    const uint32_t *row;           /* S */
    const uint8_t *kind;           /* S: CDA_NAMESPACE_INCLUSION / CDA_NAMESPACE_ABSENCE */
    const int32_t *nmt_start;      /* S */
    const int32_t *nmt_end;        /* S */
    const uint32_t *node_off;      /* S+1 */
    const uint8_t *nodes;          /* n_nodes*90 */
    uint32_t n_nodes;
    const uint64_t *share_off;     /* S+1, in shares */
    const uint8_t *shares;         /* n_shares*512 */
    uint64_t n_shares;
    const uint8_t *absence_leaf;   /* S*90: read for absence segments only */
} cda_namespace_proof_batch;
int cda_namespace_proofs_verify(cda_ctx *ctx, uint32_t k, const uint8_t *row_roots,
                                const cda_namespace_proof_batch *b, uint8_t *verdict);

/* ---- Namespace and share-range proofs across a set of resident squares ---------
 * What a node serves from a range of heights, in the launches of ONE square's call whatever n and however
 * many members are named: query i is the namespace namespaces + 29 i of member squares[i], range i is
 * [starts[i], ends[i]) of the ODS of member squares[i].  All members share k, so the output structs, their
 * layouts and their NULL-output rules are those of cda_square_namespace_plan / _proofs and
 * cda_square_share_proofs, unchanged: query i's segments are the bytes that cda_square_namespace_proofs on
 * member squares[i] answers for that namespace alone, placed in request order, and so for the ranges.  The
 * sizes of share ranges do not depend on the square: cda_square_share_proofs_plan sizes the set call as it is.
 *   cda_square_set_namespace_plan    one search launch, one copy back of n*k*4 bytes;
 *   cda_square_set_namespace_proofs  one search launch, one host pass, one proof launch;
 *   cda_square_set_share_proofs      one proof launch;
 * each with one upload of its requests.  All host pointers; complete on return.
 * cda_namespace_proofs_verify_set is cda_namespace_proofs_verify against the DAHs of n_squares squares
 * (row_roots: n_squares*2k*90, square by square, as cda_square_set_dah returns them): query q is checked
 * against the DAH squares[q].  A prover's arrays plus its squares array make the batch by pointer assignment;
 * verdicts, launches (five and one fill) and structural checks are those of cda_namespace_proofs_verify, which
 * equals this call with n_squares = 1 and squares all zero.  Only the DAHs that a query names are uploaded.
 * Share proofs of a set go to cda_share_proofs_verify as they are, with each proof's own data root.
 * Validated on the host before anything is enqueued, outputs untouched: CDA_ERR_INVALID with a message naming
 * the query or range and the field for a null array, for squares[i] not below the set's count or n_squares
 * ("query 3: square 9 is not below the set's 4 squares"), for a query equal to ParitySharesNamespace, and for
 * everything the single-square calls check, with their texts.  n == 0 returns CDA_OK.  A namespace query that
 * names a member whose push order failed answers CDA_ERR_PUSH_ORDER, naming the query, the square and the
 * violation (cda_push_order_detail is set), nothing written; share proofs of such a member are served like
 * any other. */
int cda_square_set_namespace_plan(cda_square_set *set, const uint32_t *squares, const uint8_t *namespaces,
                                  uint32_t n, cda_namespace_plan_t *out);
int cda_square_set_namespace_proofs(cda_square_set *set, const uint32_t *squares, const uint8_t *namespaces,
                                    uint32_t n, const cda_namespace_proofs_out *out);
int cda_namespace_proofs_verify_set(cda_ctx *ctx, uint32_t k, const uint8_t *row_roots, uint32_t n_squares,
                                    const uint32_t *squares, const cda_namespace_proof_batch *b, uint8_t *verdict);
int cda_square_set_share_proofs(cda_square_set *set, const uint32_t *squares, const uint32_t *starts,
                                const uint32_t *ends, uint32_t n, const cda_share_proofs_out *out);

/* ---- Blob inclusion by share commitment ------------------------------------------
 * The proof the square layout was designed for (specs/src/specs/data_square_layout.md): that the blob a
 * PayForBlobs committed to lies in the square with a given data root, shown with the subtree roots the
 * commitment is the Merkle root of instead of the blob's shares.  The object is celestia-node's
 * blob.CommitmentProof (subtree roots, one NMT proof per row, the namespace, the row proof) and the per-row
 * check nmt v0.22.0 Proof.VerifySubtreeRootInclusion, both restated from their published algorithms: no
 * vector of theirs pins them here.  What pins this code is the reference's inclusion.GetCommitment (the
 * Merkle root of the emitted subtree roots), block 408's PFB commitment and the DAH's row roots.
 *
 * A blob is (start, share_len) in row-major shares of the k x k original square.  w = SubTreeWidth(share_len,
 * threshold); start is normalised by NextShareIndex (rounded up to a multiple of w), exactly as
 * cda_square_blob_commitments does.  In every row it touches the blob is a leaf range [s0, e0) of the row
 * tree, and the subtree roots of that range are its greedy aligned cover: from c = s0 the largest power of two
 * r <= w with c % r == 0 and c + r <= e0, node c / r of level log2 r, then on from c + r
 * (calculateSubTreeRootCoordinates).  The NMT nodes of a row are those of ProveRange(s0, e0), byte for byte
 * what cda_square_share_proofs emits for the same range.
 *
 * cda_square_commitment_proofs_plan: host only, no context (the text through cda_last_error(NULL)).  Checks
 * every blob -- share_len >= 1, the blob fits k*k after normalisation, k a power of two <= 1024, threshold >=
 * 1, every offset of the batch fits 32 bits -- and returns the sizes to allocate.  CDA_ERR_INVALID with a
 * message naming the blob and the field.  n == 0: CDA_OK, all sizes zero. */
typedef struct cda_commitment_proofs_plan_t {
    uint32_t n_segments, n_roots, n_nodes, n_aunts, aunts_per_segment;
} cda_commitment_proofs_plan_t;
int cda_square_commitment_proofs_plan(uint32_t k, const uint32_t *starts, const uint32_t *share_lens, uint32_t n,
                                      uint32_t threshold, cda_commitment_proofs_plan_t *out);
/* The proofs of n blobs.  Caller-allocated host buffers of the plan's sizes, any of them NULL (S = n_segments).
 * The arrays carry cda_share_proofs_out's names and layouts where the meaning is the same:
 *   seg_off n+1; nmt_start / nmt_end S; node_off S+1; nodes n_nodes*90; row_roots S*90; rfc_total / rfc_index
 *   S; rfc_leaf_hash S*32; aunt_off S+1; aunts n_aunts*32; namespaces n*29 (the blob's first share's);
 *   start_row / end_row n.
 * There are no shares.  New:
 *   root_off S+1, in roots; subtree_roots n_roots*90, packed, blob then row then left to right;
 *   norm_start n: the normalised start;
 *   commitments n*32 (may be NULL): the RFC-6962 root of each blob's subtree roots, equal to
 *     cda_square_blob_commitments of the same blobs; at most 1365 subtree roots per blob (CDA_ERR_INVALID).
 * The blobs are checked as by the plan before anything is enqueued (CDA_ERR_INVALID, outputs untouched).  One
 * kernel launch per call, whatever n and the blobs' lengths (the kernel of cda_square_share_proofs, whose
 * segments gather subtree roots in the place of shares); commitments costs one further launch.  Host buffers,
 * complete when the call returns.  A square created with CDA_ERR_PUSH_ORDER answers CDA_ERR_PUSH_ORDER, outputs
 * untouched: nmt could not have built its trees (cda_square_namespace_proofs' rule). */
typedef struct cda_commitment_proofs_out {
    uint32_t *seg_off;
    int32_t *nmt_start;
    int32_t *nmt_end;
    uint32_t *node_off;
    uint8_t *nodes;
    uint8_t *row_roots;
    int64_t *rfc_total;
    int64_t *rfc_index;
    uint8_t *rfc_leaf_hash;
    uint32_t *aunt_off;
    uint8_t *aunts;
    uint8_t *namespaces;
    uint32_t *start_row;
    uint32_t *end_row;
    uint32_t *root_off;
    uint8_t *subtree_roots;
    uint32_t *norm_start;
    uint8_t *commitments;
} cda_commitment_proofs_out;
int cda_square_commitment_proofs(cda_square *sq, const uint32_t *starts, const uint32_t *share_lens, uint32_t n,
                                 uint32_t threshold, const cda_commitment_proofs_out *out);
/* The verifying side.  The batch is flat and takes any mix of proofs from squares of any width: a proof's k
 * is rfc_total / 4 of its segments.  A proof's share count is the sum of nmt_end - nmt_start over its
 * segments, and w = SubTreeWidth(that sum, threshold).
 * verdict[p] (n_proofs bytes).  The order is this library's choice -- the published verifier returns on its
 * first failure and fixes no numbering; the lowest number wins, but for 4, which needs no hashing, is decided
 * first and wins over all:
 *   0 valid;
 *   4 not one contiguous blob: the proof's segments do not share one rfc_total = 4k with k a power of two <=
 *     1024; rfc_index is not consecutive or not below k; nmt_start != 0 in a segment but the first; nmt_end
 *     != k in a segment but the last, or nmt_end > k; the first nmt_start is not a multiple of w; the proof
 *     has no segment;
 *   1 a row root fails its Merkle proof against the data root (cda_share_proofs_verify's row half as is);
 *   2 a row's subtree roots and nodes do not rebuild its row root; a subtree root count that is not the
 *     cover's count, and too few or too many nodes for ProveRange(nmt_start, nmt_end) of the 2k-leaf tree,
 *     are this verdict too, decided before anything is read through the counts;
 *   3 the RFC-6962 root of the proof's subtree roots is not the claimed commitment.
 * Checked on the host before anything is enqueued, CDA_ERR_INVALID with a message naming the proof or the
 * segment and the field, verdict untouched (cda_share_proofs_verify's rule): null arrays; ns_len != 29;
 * threshold == 0; offsets that do not start at 0, decrease or do not end at n_roots / n_nodes / n_aunts; not
 * 0 <= nmt_start < nmt_end <= CDA_VERIFY_MAX_LEAVES; a proof with more than 1365 subtree roots.
 * The fold of a row: one wavefront per segment stages its subtree roots and nodes in LDS.  The roots below
 * level log2 w (one per set bit of the range's remainder) are one chain of hashes; the run of level log2 w
 * folds level by level, pairs across lanes, in aligned tiles of CDA_COMMITMENT_FOLD_TILE nodes: a tile folds
 * six levels to one node, the tiles' nodes are the next run, until one tile holds the run and folds to the
 * root (k = 1024 with w = 1: 1024 nodes, 16 tiles, then one).
 * Four launches per call whatever n_proofs (row proofs, row folds, commitments, verdicts), one
 * synchronisation.  n_proofs == 0 returns CDA_OK. */
#define CDA_COMMITMENT_FOLD_TILE 64
typedef struct cda_commitment_proof_batch {
    uint32_t n_proofs;
    uint32_t ns_len;               /* 29: 90-byte nodes */
    uint32_t threshold;            /* SubtreeRootThreshold of the squares (appconsts: 64) */
    const uint8_t *data_roots;     /* n_proofs*32 */
    const uint8_t *commitments;    /* n_proofs*32: the claimed share commitments */
    const uint32_t *seg_off;       /* n_proofs+1; S = last */
    const int32_t *nmt_start;      /* S */
    const int32_t *nmt_end;        /* S */
    const uint32_t *node_off;      /* S+1 */
    const uint8_t *nodes;          /* n_nodes*90 */
    uint32_t n_nodes;
    const uint32_t *root_off;      /* S+1 */
    const uint8_t *subtree_roots;  /* n_roots*90 */
    uint32_t n_roots;
    const uint8_t *row_roots;      /* S*90 */
    const int64_t *rfc_total;      /* S */
    const int64_t *rfc_index;      /* S */
    const uint8_t *rfc_leaf_hash;  /* S*32 */
    const uint32_t *aunt_off;      /* S+1 */
    const uint8_t *aunts;          /* n_aunts*32, bottom-up */
    uint32_t n_aunts;
} cda_commitment_proof_batch;
int cda_commitment_proofs_verify(cda_ctx *ctx, const cda_commitment_proof_batch *b, uint8_t *verdict);

/* ---- Shares back into transactions and blobs -------------------------------------
 * The way back from a square: go-square v1.1.0 shares.ParseShares / ParseTxs / ParseBlobs (parseCompactShares,
 * parseSparseShares), restated from their published algorithms and specs/src/specs/shares.md (go-square is not
 * vendored; what pins this code is that spec, mainnet block 408 and the square builder).
 * The input is n shares of 512 bytes in order.  Per share: namespace = bytes [0, 29), info = byte 29, version =
 * info >> 1, start = info & 1.  A start share opens a sequence and closes the one before it, a continuation
 * extends the open one; the sequence length L is the big-endian word at [30, 34) of the start share.
 *   padding  a start share with L = 0 in any namespace, or one in the tail-padding or primary-reserved-padding
 *            namespace: one share, skipped and counted (n_padding_shares);
 *   compact  TX or PFB namespace: raw data [38, 512) of the start share and [34, 512) of a continuation, the four
 *            bytes in front being the share's reserved bytes;
 *   sparse   every other namespace, a blob: [34, 512) of the start share (478 bytes), [30, 512) of a continuation.
 * A blob is its namespace, share version, the first L bytes of its concatenated raw data, its first share and its
 * share count.  A compact sequence's stream is the first L bytes of its raw data: a uvarint of at most 10 bytes,
 * then that many bytes as one unit, until the stream ends or a uvarint of 0.  A unit reports the shares [start,
 * end) that hold it, length prefix included (for distinct txs what cda_square_tx_share_ranges returns).
 * Errors, CDA_ERR_SQUARE with a message naming the share, outputs untouched, the first in share order:
 *   "share 5: parity-namespace share"; "share 5: unsupported share version 1";
 *   "share 0: the first share of the input is a continuation share" (of a range: "... of range 2 is ...");
 *   "share 5: continuation share's namespace differs from that of its sequence's start share 3";
 *   "sequence at share 3: length 961 needs 3 shares, found 2" when a sequence closes (sparse:
 *     SparseSharesNeeded(L); compact: 1 for L <= 474, else 1 + ceil((L - 474) / 478); padding: 1);
 * then, per compact sequence, TX sequences first:
 *   "share 1: malformed unit length prefix"; "share 1: unit of 700 bytes runs past the sequence length 600"
 *     (the share holding the prefix's first byte; go-square stops silently at both);
 *   "share 2: reserved bytes 0, expected 38": every compact share's reserved bytes must be the offset in the share
 *     of the first unit whose length prefix starts in it, or 0 if none does (go-square does not check them;
 *     square.Construct always writes them so).
 * The zero fill after the data is not checked (go-square does not either).
 *
 * cda_shares_parse_plan / cda_shares_parse: host only, no context (the text through cda_last_error(NULL)); the C
 * restatement, and the yardstick of the device calls.  n_shares == 0: CDA_OK, all sizes zero.
 * cda_square_parse_plan / cda_square_parse: the same over the original square of a resident square, on the
 * device: the first 40 bytes of every share come back through the resident squares' gather kernel (one wavefront
 * per piece, aligned 8-byte stores, byte stores only at a piece's two ends), the sequence table is built and
 * checked on the host, one more launch of that kernel packs the raw bytes (one piece per source share), the
 * compact streams come back for the unit walk.  starts / ends: n_ranges share ranges [starts[i], ends[i]) of the
 * original square, row-major, ascending and disjoint (CDA_ERR_INVALID naming the range otherwise), each parsed as
 * an input of its own: a range that begins at a continuation share or ends inside a sequence fails under the
 * rules above.  n_ranges == 0 (both NULL): the whole k x k square.  blob_start, unit_start and unit_end are
 * indexes into the original square.  A square created with CDA_ERR_PUSH_ORDER parses like any other: share format
 * does not depend on namespace order.  Like the namespace calls, cda_square_parse keeps no state from the plan
 * call and reads the headers again.  Host buffers, complete when the call returns. */
typedef struct cda_parse_plan_t {
    uint32_t n_blobs, n_txs, n_pfbs, n_padding_shares;
    uint64_t blob_bytes, unit_bytes;
} cda_parse_plan_t;
typedef struct cda_parse_out {      /* any pointer may be NULL */
    uint32_t *blob_start, *blob_shares;           /* n_blobs each */
    uint8_t *blob_namespace, *blob_share_version; /* n_blobs*29, n_blobs */
    uint64_t *blob_off;                           /* n_blobs+1 */
    uint8_t *blob_data;                           /* blob_bytes, packed, no gaps */
    uint64_t *unit_off;                           /* n_txs+n_pfbs+1 */
    uint8_t *unit_data;                           /* unit_bytes; txs first, then PFBs (IndexWrapper bytes) */
    uint32_t *unit_start, *unit_end;              /* n_txs+n_pfbs each: share range of each unit */
} cda_parse_out;
int cda_shares_parse_plan(const uint8_t *shares, uint64_t n_shares, cda_parse_plan_t *out);
int cda_shares_parse(const uint8_t *shares, uint64_t n_shares, const cda_parse_out *out);
int cda_square_parse_plan(cda_square *sq, const uint32_t *starts, const uint32_t *ends, uint32_t n_ranges,
                          cda_parse_plan_t *out);
int cda_square_parse(cda_square *sq, const uint32_t *starts, const uint32_t *ends, uint32_t n_ranges,
                     const cda_parse_out *out);

/* ---- Repair ------------------------------------------
 * rsmt2d ExtendedDataSquare.Repair(rowRoots, colRoots) (EXT v0.14.0,
 * go.mod:13; used by light / full nodes after sampling).  eds: w*w*512 bytes,
 * in/out; present: w*w bytes (0 = missing: the cell's bytes are ignored and
 * reconstructed).  row_roots / col_roots: w*90 bytes each (the DAH).
 * Returns CDA_OK (eds complete), CDA_ERR_BYZANTINE (*byz_axis 0 row / 1 col,
 * *byz_index), CDA_ERR_UNREPAIRABLE, or CDA_ERR_INVALID for a complete vector
 * whose root differs from the given one ("bad root input: ...").  The roots
 * are compared as blind ones (no push-order check); a row or column whose Q0
 * namespaces descend is CDA_ERR_BYZANTINE whatever its root is, when rebuilt,
 * when completed by a rebuild, and also when complete in the input. */
int cda_repair(cda_ctx *ctx, uint8_t *eds, const uint8_t *present, uint32_t w, const uint8_t *row_roots,
               const uint8_t *col_roots, int32_t *byz_axis, uint32_t *byz_index);
/* cda_repair on an HBM-resident square (d_eds: w*w*512 device bytes, repaired
 * in place; present and the roots stay host buffers).  Same outcomes and
 * messages; the work is ordered after everything already queued on the
 * device and complete when the call returns.  Cells present in the input are
 * never written, whatever the outcome.  Alignment: d_eds 16 bytes. */
int cda_repair_device(cda_ctx *ctx, void *d_eds, const uint8_t *present, uint32_t w, const uint8_t *row_roots,
                      const uint8_t *col_roots, int32_t *byz_axis, uint32_t *byz_index);
/* ---- Batch repair --------------------------------------------------------------
 * cda_repair_device for n contiguous squares of one width in one submission
 * (a node catching up over a range of heights).  d_eds: n * w*w*512 device
 * bytes (16-byte aligned), repaired in place; present: n * w*w host bytes (any non-zero byte =
 * present); row_roots / col_roots: n * w*90 host bytes each.  status[n],
 * byz_axis[n] (may be NULL), byz_index[n] (may be NULL): written per square
 * with the codes cda_repair returns; byz_axis is -1 where none.
 *
 * Which vectors become decodable in which sweep depends on the presence maps
 * alone, so every sweep of every square is planned on the host before the
 * first launch (cda_repair_batch_plan), uploaded once, and the decode
 * launches of all squares follow each other with no host wait.  One
 * verification per chunk of squares leaves one word per square on the device;
 * only those words come back.  The batch is processed in chunks of
 * min(CDA_REPAIR_BATCH_MAX_SQUARES, CDA_REPAIR_BATCH_SCRATCH_BYTES /
 * (w*w*512)) squares, at least one: the verification's scratch is one
 * EDS-size per square of a chunk.  One synchronisation per chunk.
 * A square whose verification is not clean (byzantine, bad root input) is then
 * run alone through cda_repair_device's path on its slice of the batch, which
 * gives that call's outcome, axis, index and message.
 *
 * Returns CDA_OK whenever every square received a status, whatever the
 * statuses are; another code only when the call itself could not run (a width
 * that is not a power of two in [2, 1024]: CDA_ERR_INVALID; a device error),
 * and status / byz_axis / byz_index are then left untouched.  cda_last_error
 * holds the message of the lowest-numbered square whose status is not CDA_OK,
 * prefixed "square <i>: " (empty when there is none).  n == 0 returns CDA_OK.
 *
 * The bytes of square i afterwards:
 *   CDA_OK, or CDA_ERR_UNREPAIRABLE: byte-equal to what cda_repair_device
 *     leaves for that square alone;
 *   CDA_ERR_BYZANTINE, CDA_ERR_INVALID: every cell present in the input is
 *     unchanged, and every cell cda_repair_device's replay writes holds the
 *     bytes that call writes; other absent cells are unspecified (they may
 *     hold the batch sweeps' decode).
 * cda_repair_batch: the same for host squares (eds: n * w*w*512 host bytes),
 * with one upload and one download of the whole batch through a page-locked
 * view of the caller's buffer, as cda_extend_dah_batch does. */
#define CDA_REPAIR_BATCH_MAX_SQUARES 256
#define CDA_REPAIR_BATCH_SCRATCH_BYTES (2ull << 30)
int cda_repair_batch_device(cda_ctx *ctx, void *d_eds, const uint8_t *present, uint32_t w, uint32_t n,
                            const uint8_t *row_roots, const uint8_t *col_roots, int32_t *status, int32_t *byz_axis,
                            uint32_t *byz_index);
int cda_repair_batch(cda_ctx *ctx, uint8_t *eds, const uint8_t *present, uint32_t w, uint32_t n,
                     const uint8_t *row_roots, const uint8_t *col_roots, int32_t *status, int32_t *byz_axis,
                     uint32_t *byz_index);
/* The sweep plan of such a batch, host only, no context (the text through
 * cda_last_error(NULL)).  Per square, in each iteration every incomplete row
 * with >= w/2 cells is decoded, then, with the counts updated, every such
 * column, until nothing is decodable or every cell is present.  The plan is
 * one list of (square, axis, index) entries cut into segments in launch order
 * -- iteration 0 rows, iteration 0 columns, iteration 1 rows, ... -- each
 * holding the entries of all squares, squares ascending; empty segments are
 * dropped.  Outputs, caller-allocated, any of them NULL:
 *   *n_segments;
 *   seg_off    4w+1 words: segment g owns entries [seg_off[g], seg_off[g+1]);
 *   seg_sweep  4w words: 2 * iteration + axis of segment g, ascending;
 *   entries    n * 2w * 3 words: square, axis (0 row / 1 column), index;
 *   solved     n bytes: 1 when every cell of the square is present at the end.
 * At most 4w segments and 2w entries per square exist.  n == 0: CDA_OK, no
 * segments.  CDA_ERR_INVALID for a width that is not a power of two in
 * [2, 1024]. */
int cda_repair_batch_plan(const uint8_t *present, uint32_t w, uint32_t n, uint32_t *n_segments, uint32_t *seg_off,
                          uint32_t *seg_sweep, uint32_t *entries, uint8_t *solved);
/* rsmt2d Codec.Decode (LeoRSCodec -> reedsolomon Reconstruct): n_codewords
 * codewords of 2*n_shards shards of shard_len bytes (multiple of 64),
 * contiguous; shards with present[] == 0 are reconstructed in place (data
 * and parity).  Fewer than n_shards present: CDA_ERR_UNREPAIRABLE. */
int cda_rs_decode(cda_ctx *ctx, uint8_t *shards, const uint8_t *present, uint32_t n_shards, uint32_t shard_len,
                  uint32_t n_codewords);

/* ---- Bad-encoding fraud proofs ------------------------------------------------
 * The step after CDA_ERR_BYZANTINE: the proof that row or column `index` of a
 * committed square is not a codeword (specs/src/specs/fraud_proofs.md,
 * networking.md "BadEncodingFraudProof", proto/types.proto:247-259; built from
 * rsmt2d's ErrByzantineData and checked by celestia-node's
 * BadEncodingProof.Validate, EXT).  A proof accuses (axis, index) of a square
 * of ODS width k (W = 2k, D = log2 W) and carries m shares of that vector,
 * k <= m <= W, each with its position p along the vector and a single-leaf NMT
 * proof of D nodes (cda_square_sample_proofs' node order) against
 *   the root of the orthogonal axis at p, leaf position index (proof axis =
 *   the other axis: the normal case), or
 *   the root of the accused axis at index, leaf position p (proof axis = the
 *   accused one).
 *
 * cda_befp_build: every provable share of vector (axis, index) of `eds`
 * (w*w*512 bytes: a whole square, or what cda_repair / cda_repair_device leave
 * behind on CDA_ERR_BYZANTINE).  There is no presence mask: cell p is emitted
 * if and only if the orthogonal vector through it hashes (without a push-order
 * check) to its root in the DAH, which a vector with missing or garbage cells
 * cannot.  positions (w), shares (w*512), nmt_nodes (w*D*90): the emitted
 * cells, positions ascending, every proof against the orthogonal root;
 * *n_out their count, which may be below k -- the caller decides what then.
 * The launches do not grow with w but for the log2 w tree levels; one
 * synchronisation per call.  _device: d_eds in HBM (16-byte aligned, read
 * only), complete before the call (as cda_repair_device leaves it); the other
 * buffers stay host buffers.  Of positions, shares and nmt_nodes only the first
 * *n_out entries are written. */
int cda_befp_build(cda_ctx *ctx, const uint8_t *eds, uint32_t w, int axis, uint32_t index,
                   const uint8_t *row_roots, const uint8_t *col_roots, uint32_t *n_out, uint32_t *positions,
                   uint8_t *shares, uint8_t *nmt_nodes);
int cda_befp_build_device(cda_ctx *ctx, const void *d_eds, uint32_t w, int axis, uint32_t index,
                          const uint8_t *row_roots, const uint8_t *col_roots, uint32_t *n_out, uint32_t *positions,
                          uint8_t *shares, uint8_t *nmt_nodes);
/* A batch of fraud proofs of one ODS width (the caller groups by size), flat:
 * proof q owns shares [share_off[q], share_off[q+1]). */
typedef struct cda_befp_batch {
    uint32_t n_proofs, k;
    const uint8_t *axes;           /* n_proofs: accused axis, CDA_AXIS_ROW / CDA_AXIS_COL */
    const uint32_t *indexes;       /* n_proofs: accused index */
    const uint8_t *row_roots;      /* n_proofs*W*90: every proof's DAH */
    const uint8_t *col_roots;      /* n_proofs*W*90 */
    const uint32_t *share_off;     /* n_proofs+1 offsets into the share arrays; m = last */
    const uint32_t *positions;     /* m: position along the accused vector, strictly ascending per proof */
    const uint8_t *proof_axes;     /* m: the axis whose root the share's proof is against; NULL = the
                                      orthogonal root for every share */
    const uint8_t *shares;         /* m*512 */
    const uint8_t *nmt_nodes;      /* m*D*90 */
} cda_befp_batch;
/* The structural checks, host only (no context; the text through
 * cda_last_error(NULL), naming the proof and the field): k a power of two <=
 * 512, axes <= 1, indexes and positions < W, positions strictly ascending
 * within a proof, share_off starting at 0 and never decreasing. */
int cda_befp_batch_check(const cda_befp_batch *b);
/* BadEncodingProof.Validate of every proof against its DAH.  Runs
 * cda_befp_batch_check first (CDA_ERR_INVALID; verdict is then left
 * untouched).  verdict[q] (n_proofs bytes), the lowest number wins:
 *   1  fewer than k shares;
 *   2  a share is not included under the DAH root its proof names (the leaf
 *      namespace, the tree and the leaf position are derived from (axis,
 *      index, position, proof axis), never taken from the prover);
 *   3  the vector rebuilt from the shares (Codec.Decode with every given share
 *      as received, Codec.Encode of its k data shares, the erasured NMT root of
 *      data || parity) has the DAH's root: no fraud;
 *   0  it has another root, or breaks nmt's push order: the proof is valid.
 * rebuilt_roots (n_proofs*90, may be NULL): the rebuilt root, hashed without
 * the push-order check; zeros for proofs with verdict 1 or 2.  Host buffers;
 * at most two synchronisations; n_proofs == 0 returns CDA_OK. */
int cda_befp_verify(cda_ctx *ctx, const cda_befp_batch *b, uint8_t *verdict, uint8_t *rebuilt_roots);

/* ---- Axis halves: serve and check half rows and half columns ----------------------
 * The unit a full node rebuilds a square from (celestia-node's shwap Row and
 * the eds store's AxisHalf, EXT): k consecutive cells of one row or column of
 * the EDS.  Half i is named by axes[i] (0 = row, 1 = column), indexes[i]
 * (0 .. 2k-1, parity rows and columns included) and sides[i]: side 0 = cells
 * 0 .. k-1 of the vector, side 1 = cells k .. 2k-1.  Its k shares are
 * shares[i*k*512 ..], in vector order.  All pointers are host pointers;
 * n == 0 returns CDA_OK; duplicates are allowed.
 *
 * Refused with CDA_ERR_INVALID before anything is written, the text naming
 * the half and the field ("half 3: index 9 is not below the EDS width 8"): an
 * index >= 2k, an axis or a side above 1, squares[i] not below the set's /
 * the DAHs' count, and for the verifier a NULL col_roots where a half has
 * axis 1.
 *
 * cda_square_axis_halves / cda_square_set_axis_halves: n halves of a resident
 * square, or of the members squares[i] of a set, in one gather launch and one
 * copy back (a row half is one piece of k*512 bytes, a column half k pieces).
 *
 * cda_axis_halves_verify: Row.Verify for a batch, left and right halves
 * mixed.  Every half is completed to its vector of 2k cells -- a left half by
 * the encoder, a right half by its mirror, which computes the k data shards
 * from the k parity shards alone -- the vector is hashed as the wrapper's
 * erasured tree (index < k: cells < k keep their namespace, the rest take the
 * parity namespace; index >= k: every cell the parity namespace) and its root
 * compared with root (squares[i], axes[i], indexes[i]) of the DAHs:
 * row_roots / col_roots hold n_squares * 2k roots of 90 bytes, square by
 * square; squares == NULL: one DAH, every half against it.  col_roots may be
 * NULL when no half has axis 1.  verdict[i] (n bytes):
 *   0  the half is the DAH's;
 *   2  nmt would refuse a push of the completed vector, because a namespace
 *      is below the one before it (checked first: a root over such a vector
 *      cannot come from an honest tree, whatever it is);
 *   1  the root differs.
 * vectors (n*2k*512 bytes, may be NULL): every completed vector, whatever its
 * verdict, in the caller's order.  k a power of two <= 1024, else
 * CDA_ERR_INVALID, "square width must be a power of two <= 1024".  One
 * synchronisation. */
int cda_square_axis_halves(cda_square *sq, const uint8_t *axes, const uint32_t *indexes, const uint8_t *sides,
                           uint32_t n, uint8_t *shares);
int cda_square_set_axis_halves(cda_square_set *set, const uint32_t *squares, const uint8_t *axes,
                               const uint32_t *indexes, const uint8_t *sides, uint32_t n, uint8_t *shares);
int cda_axis_halves_verify(cda_ctx *ctx, uint32_t k, const uint8_t *row_roots, const uint8_t *col_roots,
                           uint32_t n_squares, const uint32_t *squares, const uint8_t *axes, const uint32_t *indexes,
                           const uint8_t *sides, uint32_t n, const uint8_t *shares, uint8_t *verdict,
                           uint8_t *vectors);
/* The mirror of cda_rs_encode: the n_shards data shards of every codeword from
 * its n_shards parity shards alone (parity, data: n_codewords * n_shards *
 * shard_len bytes, codeword by codeword).  Leopard's encode is two invertible
 * transforms; this runs their inverses on the encoder's own kernels, without
 * the general decoder's error locator.  n_shards a power of two <= 1024, else
 * CDA_ERR_UNSUPPORTED; shard_len a multiple of 64, else CDA_ERR_CHUNK_SIZE
 * with cda_rs_encode's text. */
int cda_rs_recover_data(cda_ctx *ctx, const uint8_t *parity, uint32_t n_shards, uint32_t shard_len,
                        uint32_t n_codewords, uint8_t *data);

/* ---- Standalone erasured NMT trees -----------
 * wrapper.NewErasuredNamespacedMerkleTree(squareSize, axisIndex), n_cells
 * Pushes and Root() (pkg/wrapper/nmt_wrapper.go:55-124) for trees built
 * outside ComputeExtendedDataSquare (pkg/proof/proof.go:157-189,
 * pkg/inclusion/nmt_caching.go:96-109, test/util/malicious/tree.go:46-70).
 *   cells: n_trees * n_cells * cell_len bytes; push i of tree t at
 *     (t*n_cells + i)*cell_len; cell_len >= 29 (NamespaceSize).  The leaf
 *     namespace is cell[0:29] when i < square_size and axis_index[t] <
 *     square_size (isQuadrantZero, :138-140), else ParitySharesNamespace.
 *   n_cells: any count <= 2*square_size (nmt's RFC-6962 split for non powers
 *     of two); 0 gives NmtHasher.EmptyRoot.
 *   roots: n_trees * 90 bytes; status (n_trees int32, may be NULL): CDA_OK or
 *     CDA_ERR_PUSH_ORDER per tree (nmt Push ErrInvalidPushOrder; the call then
 *     returns CDA_ERR_PUSH_ORDER with the first tree's message).
 * 512-byte cells, a power-of-two n_cells and consecutive axis indexes (rows
 * of a square) run on the square kernels; anything else on generic ones. */
int cda_nmt_axis_roots(cda_ctx *ctx, const uint8_t *cells, uint32_t cell_len, uint32_t n_cells, uint32_t n_trees,
                       uint32_t square_size, const uint32_t *axis_index, uint8_t *roots, int32_t *status);
int cda_nmt_axis_root(cda_ctx *ctx, const uint8_t *cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                      uint32_t axis_index, uint8_t *root);
/* (*ErasuredNamespacedMerkleTree).ProveRange(start, end) (:126-129 -> nmt
 * ProveRange) of the tree above: nodes receives the proof nodes (90 B each, the
 * maximal subtrees outside [start, end) depth first, left to right; at most
 * 2*ceil(log2 n_cells)), *n_nodes their count, root (may be NULL) the root.
 * start >= end or end > n_cells: CDA_ERR_INVALID ("invalid proof range"). */
int cda_nmt_prove_range(cda_ctx *ctx, const uint8_t *cells, uint32_t cell_len, uint32_t n_cells, uint32_t square_size,
                        uint32_t axis_index, uint32_t start, uint32_t end, uint8_t *nodes, uint32_t *n_nodes,
                        uint8_t *root);
/* go-square/merkle HashFromByteSlices (RFC-6962) over n byte slices, item i =
 * items[off[i] .. off[i+1]) (off has n + 1 entries): (*DataAvailabilityHeader)
 * .Hash for any root count and size (data_availability_header.go:92-108).
 * n == 0 gives sha256(""). */
int cda_merkle_root(cda_ctx *ctx, const uint8_t *items, const uint64_t *off, uint32_t n, uint8_t out[32]);

/* ---- Proof verification (the verifying side) ----------
 * The hashed halves of ShareProof.Validate / VerifyProof
 * (pkg/proof/share_proof.go:16-82) and RowProof.Validate
 * (pkg/proof/row_proof.go:13-51) for a batch of independent proofs in one
 * submission: per row of a proof (a "segment") nmt Proof.VerifyInclusion of the
 * row's shares against the row root (EXT nmt v0.22.0, IgnoreMaxNamespace) and
 * go-square/merkle Proof.Verify of the row root against the data root (EXT
 * v1.1.0; any Total, RFC-6962 split).  The structural checks of Validate
 * (counts, negative start, ...) are the caller's (celestia_da.proof).
 * The batch is flat (CSR offsets), so one call takes any mix of proofs; the
 * namespace size is the batch's (the reference's own vector uses 33 bytes):
 * ns_len = 29 with 512-byte shares runs the square's leaf hashing, any other
 * size byte-addressed kernels.
 * Checked on the host before anything is enqueued, CDA_ERR_INVALID with a
 * message naming the proof and the field (verdict is then left untouched):
 * offsets start at 0, never decrease and end at n_nodes / n_aunts; the sum of
 * nmt_end - nmt_start equals n_shares; 1 <= ns_len <= CDA_VERIFY_MAX_NS;
 * 0 <= nmt_start < nmt_end <= CDA_VERIFY_MAX_LEAVES.
 * Verdicts, not errors: rfc_total <= 0, rfc_index outside [0, total) or an
 * aunt count that is not the path's depth (1); too few or too many NMT nodes
 * for the range (2).  n_proofs == 0 returns CDA_OK. */
#define CDA_VERIFY_MAX_NS 64        /* bytes of version||id */
#define CDA_VERIFY_MAX_LEAVES 2048  /* NMTProof.End bound: the widest row the library builds (k = 1024) */
typedef struct cda_share_proof_batch {
    uint32_t n_proofs;
    uint32_t ns_len;               /* 1 + len(NamespaceId); 29 on Celestia; node size N = 2*ns_len + 32 */
    uint32_t share_len;            /* bytes per ShareProof.Data item (512) */
    const uint8_t *data_roots;     /* n_proofs*32; NULL = skip the RowProof half */
    const uint8_t *namespaces;     /* n_proofs*ns_len: version || id */
    const uint32_t *seg_off;       /* n_proofs+1; proof p owns segments (rows) [seg_off[p], seg_off[p+1]); S = last */
    const int32_t *nmt_start;      /* S: NMTProof.Start */
    const int32_t *nmt_end;        /* S: NMTProof.End */
    const uint32_t *node_off;      /* S+1 offsets into nodes, in nodes of N bytes */
    const uint8_t *nodes;          /* n_nodes*N: NMTProof.Nodes */
    uint32_t n_nodes;
    const uint8_t *row_roots;      /* S*N: RowProof.RowRoots */
    const int64_t *rfc_total;      /* S: Proof.Total */
    const int64_t *rfc_index;      /* S: Proof.Index */
    const uint8_t *rfc_leaf_hash;  /* S*32: Proof.LeafHash */
    const uint32_t *aunt_off;      /* S+1 offsets into aunts, in aunts of 32 bytes */
    const uint8_t *aunts;          /* n_aunts*32: Proof.Aunts, bottom-up */
    uint32_t n_aunts;
    const uint8_t *shares;         /* n_shares*share_len: ShareProof.Data, concatenated in proof then segment
                                      order; NULL = skip the NMT half (nmt_*, node*, n_shares are then unused) */
    uint64_t n_shares;
} cda_share_proof_batch;
/* verdict[p] (n_proofs bytes): 0 valid, 1 "row proof failed to verify", 2
 * "share proof failed to verify" (1 wins, as Validate runs the row proof
 * first).  Host buffers; complete when the call returns. */
int cda_share_proofs_verify(cda_ctx *ctx, const cda_share_proof_batch *b, uint8_t *verdict);

/* Stage timing (HIP events on the launch stream).  When enabled, every
 * enqueued stage is bracketed by events; cda_stage_times synchronises them and
 * returns, per stage, the summed milliseconds and launch counts since the
 * previous call, then resets.  Stages: 0 RS Q0 (rows+cols), 1 RS Q3, 2 push-
 * order check, 3 NMT leaves, 4 NMT levels, 5 data root, 6 every launch of
 * cda_square_commitment_proofs, 7 every launch of cda_commitment_proofs_verify. */
#define CDA_NUM_STAGES 8
int cda_set_profiling(cda_ctx *ctx, int enable);
int cda_stage_times(cda_ctx *ctx, double *ms, uint32_t *counts, int n_stages);

#ifdef __cplusplus
}
#endif

#endif /* CDA_H */
