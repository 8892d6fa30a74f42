"""Axis halves of device-resident squares (libcda.so): the unit a full node
rebuilds a square from.

A half is k consecutive cells of one row or column of the EDS -- side 0 the
cells 0 .. k-1 of the vector, side 1 the cells k .. 2k-1 (celestia-node's shwap
Row and the eds store's AxisHalf).  A serving node hands halves out of a
resident square; a receiving node completes each half to its vector, checks the
vector's erasured NMT root against the DataAvailabilityHeader and hands the
vectors that verified to Repair:

    batch = ResidentSquare(ods).axis_halves(coords)          # cda_square_axis_halves, one launch
    verdicts, vectors = verify_axis_halves(batch, dah, vectors=True)   # cda_axis_halves_verify
    eds, present = assemble(batch, verdicts, vectors)        # -> rsmt2d.ExtendedDataSquare.repair
    eds, present = assemble_batch(batch, verdicts, vectors)  # many squares -> rsmt2d.repair_batch

A right half carries parity only.  Its data shards come from the mirror of the
encoder (cda_rs_recover_data: the inverses of Leopard's two transforms, on the
encoder's own kernels), not from the general erasure decoder.

Reference: the restated behaviour is celestia-node's published Row.Verify and
nmt's push rule over pkg/wrapper/nmt_wrapper.go's erasured tree; the pins are
the oracle's encoder, decoder and axis_root (tests/axis_halves_ref.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import NMT_ROOT_SIZE, SHARE_SIZE, default_context, ptr

AXIS_ROW = _lib.CDA_AXIS_ROW
AXIS_COL = _lib.CDA_AXIS_COL
SIDE_LEFT = 0    # cells 0 .. k-1 of the vector
SIDE_RIGHT = 1   # cells k .. 2k-1

VALID = 0        # verdicts of verify_axis_halves
BAD_ROOT = 1
BAD_PUSH_ORDER = 2


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def split_coords(coords):
    """(squares, axes, indexes, sides) as contiguous uint32 / uint8 / uint32 /
    uint8 arrays from an (n, 4) integer array of (square, axis, index, side).
    Values the ABI's types cannot carry are CDA_ERR_INVALID here, naming the
    half and the field; the range checks against the square are the library's."""
    c = np.asarray(coords, dtype=np.int64)
    if c.size == 0:
        c = c.reshape(0, 4)
    if c.ndim != 2 or c.shape[1] != 4:
        raise ValueError("coords must be an (n, 4) array of (square, axis, index, side)")
    for j, (name, top) in enumerate((("square", 1 << 32), ("axis", 256), ("index", 1 << 32), ("side", 256))):
        bad = np.nonzero((c[:, j] < 0) | (c[:, j] >= top))[0]
        if bad.size:
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"half {bad[0]}: {name} {c[bad[0], j]} out of range")
    return (np.ascontiguousarray(c[:, 0], dtype=np.uint32), np.ascontiguousarray(c[:, 1], dtype=np.uint8),
            np.ascontiguousarray(c[:, 2], dtype=np.uint32), np.ascontiguousarray(c[:, 3], dtype=np.uint8))


@dataclass
class HalfBatch:
    """n axis halves of squares of ODS width k."""
    k: int
    coords: np.ndarray    # (n, 4) int64: square, axis, index, side
    shares: np.ndarray    # (n, k, 512) uint8: the half's cells in vector order

    def __len__(self) -> int:
        return self.coords.shape[0]

    def copy(self) -> "HalfBatch":
        return HalfBatch(self.k, self.coords.copy(), self.shares.copy())


def _coords4(coords, width: int) -> np.ndarray:
    c = np.asarray(coords, dtype=np.int64)
    c = c.reshape(0, width) if c.size == 0 else c
    if c.ndim != 2 or c.shape[1] != width:
        names = "(square, axis, index, side)" if width == 4 else "(axis, index, side)"
        raise ValueError(f"coords must be an (n, {width}) array of {names}")
    if width == 3:
        c = np.concatenate([np.zeros((c.shape[0], 1), dtype=np.int64), c], axis=1)
    return c


def serve(sq, coords) -> HalfBatch:
    """cda_square_axis_halves on a proof.ResidentSquare: coords is an (n, 3)
    array of (axis, index, side); one gather launch and one copy back for the
    whole batch.  The batch's square column is 0."""
    c = _coords4(coords, 3)
    _, axes, indexes, sides = split_coords(c)
    shares = np.empty((c.shape[0], sq.k, SHARE_SIZE), dtype=np.uint8)
    sq.ctx.check(sq.ctx.lib.cda_square_axis_halves(sq.h, ptr(axes), _u32p(indexes), ptr(sides), c.shape[0],
                                                   ptr(shares)))
    return HalfBatch(sq.k, c, shares)


def serve_set(sqset, coords) -> HalfBatch:
    """cda_square_set_axis_halves on a proof.ResidentSquareSet: coords is an
    (n, 4) array of (square, axis, index, side) over any number of members."""
    c = _coords4(coords, 4)
    squares, axes, indexes, sides = split_coords(c)
    shares = np.empty((c.shape[0], sqset.k, SHARE_SIZE), dtype=np.uint8)
    sqset.ctx.check(sqset.ctx.lib.cda_square_set_axis_halves(sqset.h, _u32p(squares), ptr(axes), _u32p(indexes),
                                                             ptr(sides), c.shape[0], ptr(shares)))
    return HalfBatch(sqset.k, c, shares)


def _roots(dahs, W: int):
    """(row_roots, col_roots, n_squares) from one (row_roots, col_roots) pair
    or a pair of per-square stacks; col_roots may be None."""
    rows, cols = dahs
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint8).reshape(-1, W, NMT_ROOT_SIZE))
    if cols is not None:
        cols = np.ascontiguousarray(np.asarray(cols, dtype=np.uint8).reshape(-1, W, NMT_ROOT_SIZE))
        if cols.shape != rows.shape:
            raise ValueError("row_roots and col_roots are of different numbers of squares")
    return rows, cols, rows.shape[0]


def verify_axis_halves(batch: HalfBatch, dahs, ctx=None, vectors: bool = False):
    """cda_axis_halves_verify: a uint8 verdict per half -- 0 the half is the
    DAH's, 2 nmt would refuse a push of the completed vector (checked first),
    1 the root differs.  dahs: (row_roots, col_roots) of one square, (2k, 90)
    each, or of n_squares squares, (n_squares, 2k, 90) each, indexed by the
    batch's square column; col_roots may be None when no half is a column's.
    vectors=True: returns (verdicts, vectors), the completed (n, 2k, 512)
    vectors whatever their verdict."""
    ctx = ctx or default_context()
    n, k, W = len(batch), batch.k, 2 * batch.k
    rows, cols, n_squares = _roots(dahs, W)
    squares, axes, indexes, sides = split_coords(batch.coords)
    shares = np.ascontiguousarray(batch.shares, dtype=np.uint8)
    if shares.size != n * k * SHARE_SIZE:
        raise ValueError(f"{n} halves of {k} shares but {shares.size} bytes")
    verdict = np.full(n, 255, dtype=np.uint8)
    vec = np.empty((n, W, SHARE_SIZE), dtype=np.uint8) if vectors else None
    ctx.check(ctx.lib.cda_axis_halves_verify(ctx.h, k, ptr(rows), ptr(cols), n_squares, _u32p(squares), ptr(axes),
                                             _u32p(indexes), ptr(sides), n, ptr(shares), ptr(verdict), ptr(vec)))
    return (verdict, vec) if vectors else verdict


def assemble(batch: HalfBatch, verdicts, vectors):
    """(eds, present) for rsmt2d.ExtendedDataSquare.repair: the (2k, 2k, 512)
    square with every vector whose verdict is 0 filled in -- the whole row or
    column, the completed half included -- and marked present in the (2k, 2k)
    mask; every other cell zero and absent.  The batch is of one square (its
    square column is ignored)."""
    W = 2 * batch.k
    v = np.asarray(verdicts).reshape(-1)
    if v.size != len(batch):
        raise ValueError(f"{len(batch)} halves but {v.size} verdicts")
    vec = np.asarray(vectors, dtype=np.uint8).reshape(len(batch), W, SHARE_SIZE)
    eds = np.zeros((W, W, SHARE_SIZE), dtype=np.uint8)
    present = np.zeros((W, W), dtype=np.uint8)
    for i in np.nonzero(v == VALID)[0].tolist():
        _, axis, index, _ = batch.coords[i].tolist()
        if axis == AXIS_ROW:
            eds[index], present[index] = vec[i], 1
        else:
            eds[:, index], present[:, index] = vec[i], 1
    return eds, present


def assemble_batch(batch: HalfBatch, verdicts, vectors, n_squares: int | None = None):
    """(eds, present) for rsmt2d.repair_batch: what assemble builds for each
    square of the batch's square column, stacked as (n_squares, 2k, 2k, 512)
    and (n_squares, 2k, 2k).  n_squares defaults to the highest square named
    plus one."""
    W = 2 * batch.k
    v = np.asarray(verdicts).reshape(-1)
    if v.size != len(batch):
        raise ValueError(f"{len(batch)} halves but {v.size} verdicts")
    vec = np.asarray(vectors, dtype=np.uint8).reshape(len(batch), W, SHARE_SIZE)
    sq = batch.coords[:, 0]
    if n_squares is None:
        n_squares = int(sq.max()) + 1 if len(batch) else 0
    eds = np.zeros((n_squares, W, W, SHARE_SIZE), dtype=np.uint8)
    present = np.zeros((n_squares, W, W), dtype=np.uint8)
    for s in range(n_squares):
        pick = np.nonzero(sq == s)[0]
        eds[s], present[s] = assemble(HalfBatch(batch.k, batch.coords[pick], batch.shares[pick]), v[pick], vec[pick])
    return eds, present


def recover_data(parity, ctx=None) -> np.ndarray:
    """cda_rs_recover_data: the data shards (n, k, L) of n codewords from their
    parity shards (n, k, L) alone; k a power of two <= 1024, L a multiple of 64."""
    ctx = ctx or default_context()
    p = np.ascontiguousarray(parity, dtype=np.uint8)
    if p.ndim != 3:
        raise ValueError("parity must be an (n, k, L) array")
    n, k, L = p.shape
    data = np.empty_like(p)
    ctx.check(ctx.lib.cda_rs_recover_data(ctx.h, ptr(p), k, L, n, ptr(data)))
    return data
