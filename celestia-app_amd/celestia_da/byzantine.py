"""Bad-encoding fraud proofs (libcda.so: cda_befp_build / cda_befp_verify).

The last step of a block's data-availability life: when Repair names a row or
column that is not a codeword (rsmt2d ErrByzantineData, here
ByzantineDataError), a full node turns the cells it holds of that vector into
a proof, and a light node that receives one checks it against the block's
DataAvailabilityHeader before it rejects the block.

    try:
        eds.repair(dah.row_roots, dah.column_roots, present)
    except ByzantineDataError as e:
        proof = build_bad_encoding_proof(eds.array(), dah.row_roots, dah.column_roots, e.axis, e.index)
    ...
    reasons = validate_bad_encoding_proofs([proof], [dah])     # [None]: the fraud is confirmed

Reference: specs/src/specs/fraud_proofs.md, specs/src/specs/networking.md
"BadEncodingFraudProof", proto/types.proto:247-259 (the wire message's height
and header fields are the caller's); the order of the checks is celestia-node's
BadEncodingProof.Validate.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import NMT_ROOT_SIZE, SHARE_SIZE, CdaError, default_context, ptr

AXIS_ROW = _lib.CDA_AXIS_ROW
AXIS_COL = _lib.CDA_AXIS_COL

# cda_befp_verify verdicts (include/cda.h); 0 = the fraud is confirmed
REASONS = {
    1: "fewer shares than the ODS width: the vector cannot be rebuilt",
    2: "a share is not included under the data availability header root its proof names",
    3: "the rebuilt vector has the committed root: no bad encoding",
}


def _log2(x: int) -> int:
    n = 0
    while (1 << n) < x:
        n += 1
    return n


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _roots_array(roots, W: int | None = None) -> np.ndarray:
    """W roots as a contiguous (W, 90) uint8 array, from an array or a list of 90-byte values."""
    if isinstance(roots, np.ndarray):
        a = np.ascontiguousarray(roots, dtype=np.uint8).reshape(-1, NMT_ROOT_SIZE)
    else:
        a = np.frombuffer(b"".join(bytes(r) for r in roots), dtype=np.uint8).reshape(-1, NMT_ROOT_SIZE).copy()
    if W is not None and a.shape[0] != W:
        raise ValueError(f"{a.shape[0]} roots for an EDS of width {W}")
    return a


def _dah_roots(dah):
    """(row_roots, col_roots) of a da.DataAvailabilityHeader or of a (row_roots, col_roots) pair."""
    if hasattr(dah, "row_roots") and hasattr(dah, "column_roots"):
        return dah.row_roots, dah.column_roots
    rows, cols = dah
    return rows, cols


@dataclass
class BadEncodingProof:
    """The shares of one accused vector (axis 0 row / 1 column, index) of a square of ODS width k, each with its
    position along the vector, the axis whose root its NMT proof is against and the proof's D = log2(2k) nodes."""
    k: int
    axis: int
    index: int
    positions: np.ndarray    # (m,) uint32, strictly ascending
    proof_axes: np.ndarray   # (m,) uint8
    shares: np.ndarray       # (m, 512)
    nmt_nodes: np.ndarray    # (m, D, 90)

    def __len__(self) -> int:
        return int(np.asarray(self.positions).shape[0])


BefpBatch = _lib.BefpBatch


def batch_check(batch: BefpBatch, lib=None) -> str | None:
    """cda_befp_batch_check: the library's structural checks of a flat batch (host only, no context): None, or
    the text naming the proof and the field."""
    lib = lib or _lib.load()
    if lib.cda_befp_batch_check(C.byref(batch)) == _lib.CDA_OK:
        return None
    return lib.cda_last_error(None).decode()


def build_shares(eds, row_roots, col_roots, axis: int, index: int, ctx=None):
    """cda_befp_build / cda_befp_build_device: (positions, shares, nmt_nodes) of every provable cell of vector
    (axis, index).  eds: a (W, W, 512) uint8 array, or a device pointer (int) to such a square."""
    ctx = ctx or default_context()
    lib = ctx.lib
    rows = _roots_array(row_roots)
    W = rows.shape[0]
    cols = _roots_array(col_roots, W)
    D = _log2(W)
    n = C.c_uint32(0)
    positions = np.empty(W, dtype=np.uint32)
    shares = np.empty((W, SHARE_SIZE), dtype=np.uint8)
    nodes = np.empty((W, D, NMT_ROOT_SIZE), dtype=np.uint8)
    if isinstance(eds, (int, np.integer)):
        rc = lib.cda_befp_build_device(ctx.h, int(eds), W, axis, index, ptr(rows), ptr(cols), C.byref(n),
                                       _u32p(positions), ptr(shares), ptr(nodes))
    else:
        a = np.ascontiguousarray(eds, dtype=np.uint8)
        if a.size != W * W * SHARE_SIZE:
            raise ValueError(f"an EDS of {a.size} bytes does not match {W} roots per axis")
        rc = lib.cda_befp_build(ctx.h, ptr(a), W, axis, index, ptr(rows), ptr(cols), C.byref(n), _u32p(positions),
                                ptr(shares), ptr(nodes))
    ctx.check(rc)
    m = n.value
    return positions[:m].copy(), shares[:m].copy(), nodes[:m].copy()


def build_bad_encoding_proof(eds, row_roots, col_roots, axis: int, index: int, samples=None,
                             ctx=None) -> BadEncodingProof:
    """The fraud proof of vector (axis, index): the builder's shares, proven against the orthogonal roots, merged
    with the entries of `samples` (a sampling.SampleBatch) that lie on the vector, are not covered yet and whose
    axis_roots entry is the DAH root they name (either proof axis).  Raises CdaError when fewer than k shares
    result: such a proof cannot convince anyone."""
    rows = _roots_array(row_roots)
    W = rows.shape[0]
    cols = _roots_array(col_roots, W)
    k = W // 2
    pos, shares, nodes = build_shares(eds, rows, cols, axis, index, ctx)
    entries = {int(p): (1 - axis, shares[i], nodes[i]) for i, p in enumerate(pos)}
    if samples is not None:
        if samples.k != k:
            raise ValueError(f"samples of a square of ODS width {samples.k}, the roots are of width {k}")
        for i, (r, c, ax) in enumerate(np.asarray(samples.coords).tolist()):
            if (r if axis == AXIS_ROW else c) != index:
                continue
            p = c if axis == AXIS_ROW else r
            if p in entries:
                continue
            named = rows[r] if ax == AXIS_ROW else cols[c]   # the root a sample's proof is against
            if not np.array_equal(np.asarray(samples.axis_roots[i]), named):
                continue
            entries[p] = (ax, np.asarray(samples.shares[i]), np.asarray(samples.nmt_nodes[i]))
    if len(entries) < k:
        raise CdaError(_lib.CDA_ERR_INVALID, f"{len(entries)} provable shares of {'row' if axis == AXIS_ROW else 'col'} "
                                             f"{index}, a fraud proof needs {k}")
    order = sorted(entries)
    D = _log2(W)
    return BadEncodingProof(
        k, axis, index, np.array(order, dtype=np.uint32), np.array([entries[p][0] for p in order], dtype=np.uint8),
        np.stack([entries[p][1] for p in order]).reshape(-1, SHARE_SIZE).astype(np.uint8),
        np.stack([entries[p][2] for p in order]).reshape(-1, D, NMT_ROOT_SIZE).astype(np.uint8))


def structural_error(p: BadEncodingProof) -> str | None:
    """The structural checks of one proof, as cda_befp_batch_check states them for a batch, plus the array
    shapes a flat batch cannot carry wrong: None, or the text."""
    k = int(p.k)
    if k < 1 or k & (k - 1) or k > 512:
        return f"square width {k} is not a power of two <= 512"
    W, D = 2 * k, _log2(2 * k)
    if p.axis not in (AXIS_ROW, AXIS_COL):
        return f"axis {p.axis} is neither 0 (row) nor 1 (column)"
    if not 0 <= int(p.index) < W:
        return f"index {p.index} is outside the EDS width {W}"
    pos = np.asarray(p.positions, dtype=np.int64).reshape(-1)
    m = pos.size
    if np.asarray(p.proof_axes).reshape(-1).size != m:
        return f"{m} positions but {np.asarray(p.proof_axes).size} proof axes"
    if np.asarray(p.shares).size != m * SHARE_SIZE:
        return f"{m} positions but {np.asarray(p.shares).size} bytes of shares"
    if np.asarray(p.nmt_nodes).size != m * D * NMT_ROOT_SIZE:
        return f"{m} positions but {np.asarray(p.nmt_nodes).size} bytes of proof nodes ({D} nodes of 90 bytes each)"
    if m and (pos.min() < 0 or pos.max() >= W):
        return f"a position is outside the EDS width {W}"
    if m > 1 and (np.diff(pos) <= 0).any():
        return "positions are not strictly ascending"
    if m and np.asarray(p.proof_axes).max() > 1:
        return "a proof axis is neither 0 (row) nor 1 (column)"
    return None


def pack_batch(proofs, dahs):
    """(BefpBatch, keep-alive arrays) of proofs of one ODS width with their DAHs."""
    k = int(proofs[0].k)
    W = 2 * k
    n = len(proofs)
    axes = np.array([p.axis for p in proofs], dtype=np.uint8)
    indexes = np.array([p.index for p in proofs], dtype=np.uint32)
    pairs = [_dah_roots(d) for d in dahs]
    rows = np.ascontiguousarray(np.stack([_roots_array(r, W) for r, _ in pairs])) if n else np.zeros((0, W, 90), np.uint8)
    cols = np.ascontiguousarray(np.stack([_roots_array(c, W) for _, c in pairs])) if n else np.zeros((0, W, 90), np.uint8)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) for p in proofs])

    def cat(arrs, dtype, width):
        a = [np.asarray(x, dtype=dtype).reshape(-1, width) for x in arrs]
        return np.ascontiguousarray(np.concatenate(a)) if a else np.zeros((0, width), dtype=dtype)
    D = _log2(W)
    positions = cat([p.positions for p in proofs], np.uint32, 1)
    proof_axes = cat([p.proof_axes for p in proofs], np.uint8, 1)
    shares = cat([p.shares for p in proofs], np.uint8, SHARE_SIZE)
    nodes = cat([p.nmt_nodes for p in proofs], np.uint8, D * NMT_ROOT_SIZE)
    keep = (axes, indexes, rows, cols, off, positions, proof_axes, shares, nodes)
    b = BefpBatch(n, k, ptr(axes), _u32p(indexes), ptr(rows), ptr(cols), _u32p(off), _u32p(positions),
                  ptr(proof_axes), ptr(shares), ptr(nodes))
    return b, keep


def verify_batch(proofs, dahs, ctx=None):
    """cda_befp_verify of proofs of one ODS width: (verdicts (n,) uint8, rebuilt roots (n, 90))."""
    ctx = ctx or default_context()
    lib = ctx.lib
    n = len(proofs)
    verdict = np.full(n, 255, dtype=np.uint8)
    rebuilt = np.zeros((n, NMT_ROOT_SIZE), dtype=np.uint8)
    if n == 0:
        return verdict, rebuilt
    b, keep = pack_batch(proofs, dahs)
    ctx.check(lib.cda_befp_verify(ctx.h, C.byref(b), ptr(verdict), ptr(rebuilt)))
    del keep
    return verdict, rebuilt


def validate_bad_encoding_proofs(proofs, dahs, ctx=None) -> list:
    """BadEncodingProof.Validate of every proof against its DataAvailabilityHeader (a da.DataAvailabilityHeader
    or a (row_roots, col_roots) pair): None where the fraud is confirmed, else the reason text.  Proofs are
    grouped by ODS width, one cda_befp_verify call per group; a structurally malformed proof gets its own text
    and never reaches the library."""
    proofs, dahs = list(proofs), list(dahs)
    if len(proofs) != len(dahs):
        raise ValueError(f"{len(proofs)} proofs but {len(dahs)} data availability headers")
    out: list = [None] * len(proofs)
    groups: dict = {}
    for i, (p, d) in enumerate(zip(proofs, dahs)):
        err = structural_error(p)
        if err is None and len(_dah_roots(d)[0]) != 2 * p.k:
            err = f"the data availability header has {len(_dah_roots(d)[0])} row roots, the proof's square {2 * p.k}"
        if err is not None:
            out[i] = err
            continue
        groups.setdefault(int(p.k), []).append(i)
    for k in sorted(groups):
        ids = groups[k]
        verdict, _ = verify_batch([proofs[i] for i in ids], [dahs[i] for i in ids], ctx)
        for i, v in zip(ids, verdict.tolist()):
            out[i] = None if v == 0 else REASONS.get(v, f"verdict {v}")
    return out
