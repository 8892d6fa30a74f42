"""Data-availability sampling over a device-resident square (libcda.so).

What a full node does with an EDS once it is built: serve cells of the whole
extended square -- parity quadrants included -- each with its NMT inclusion
proof against the row or the column root and the merkle proof of that root in
the DataAvailabilityHeader; and what a sampling node does with the answers:
check them in one batch and hand the cells that verified to Repair.

    batch = ResidentSquare(ods).sample_proofs(coords)      # cda_square_sample_proofs, one launch
    verdicts = verify_samples(batch, data_root)            # cda_sample_proofs_verify
    eds, present = assemble(batch, verdicts)               # -> cda_repair / rsmt2d.ExtendedDataSquare.repair
    eds, present = assemble_batch(batches, verdicts)       # many squares -> cda_repair_batch / rsmt2d.repair_batch

Reference: rsmt2d's row / column trees built by pkg/wrapper/nmt_wrapper.go
(ErasuredNamespacedMerkleTree: Q0 cells under their own namespace, parity cells
under ParitySharesNamespace), nmt ProveRange / VerifyInclusion, and
pkg/da/data_availability_header.go (the data root over rowRoots || colRoots).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import NAMESPACE_SIZE, NMT_ROOT_SIZE, SHARE_SIZE, default_context, ptr

AXIS_ROW = _lib.CDA_AXIS_ROW
AXIS_COL = _lib.CDA_AXIS_COL


def _log2(x: int) -> int:
    n = 0
    while (1 << n) < x:
        n += 1
    return n


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def split_coords(coords):
    """(rows, cols, axes) as contiguous uint32 / uint32 / uint8 arrays from an
    (n, 3) integer array of (row, col, axis); an (n, 2) array of (row, col)
    gives axes None (every sample on the row axis).  Values a uint32 / uint8
    cannot carry are CDA_ERR_INVALID here, naming the sample and the field; the
    range check against the square is the library's."""
    c = np.asarray(coords, dtype=np.int64)
    if c.size == 0:
        c = c.reshape(0, 3)
    if c.ndim != 2 or c.shape[1] not in (2, 3):
        raise ValueError("coords must be an (n, 3) array of (row, col, axis) or an (n, 2) array of (row, col)")
    for j, (name, top) in enumerate((("row", 1 << 32), ("col", 1 << 32), ("axis", 256))[:c.shape[1]]):
        bad = np.nonzero((c[:, j] < 0) | (c[:, j] >= top))[0]
        if bad.size:
            raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"sample {bad[0]}: {name} {c[bad[0], j]} out of range")
    rows = np.ascontiguousarray(c[:, 0], dtype=np.uint32)
    cols = np.ascontiguousarray(c[:, 1], dtype=np.uint32)
    axes = np.ascontiguousarray(c[:, 2], dtype=np.uint8) if c.shape[1] == 3 else None
    return rows, cols, axes


@dataclass
class SampleBatch:
    """The answer to a batch of samples (cda_square_sample_proofs): numpy
    arrays with the ABI's strides, D = log2(2k) nodes and A = log2(4k) aunts
    per sample."""
    k: int
    coords: np.ndarray       # (n, 3) int64: row, col, axis
    shares: np.ndarray       # (n, 512)
    namespaces: np.ndarray   # (n, 29)
    nmt_nodes: np.ndarray    # (n, D, 90)
    axis_roots: np.ndarray   # (n, 90)
    leaf_hash: np.ndarray    # (n, 32)
    aunts: np.ndarray        # (n, A, 32)

    @staticmethod
    def empty(k: int, coords, fill: int | None = None) -> "SampleBatch":
        """Output arrays for `coords` of a square of ODS width k (uninitialised, or filled with `fill`)."""
        c = np.asarray(coords, dtype=np.int64)
        c = c.reshape(0, 3) if c.size == 0 else c
        if c.ndim == 2 and c.shape[1] == 2:
            c = np.concatenate([c, np.zeros((c.shape[0], 1), dtype=np.int64)], axis=1)
        n, D = c.shape[0], _log2(2 * k)
        mk = (lambda *s: np.empty(s, dtype=np.uint8)) if fill is None else \
            (lambda *s: np.full(s, fill, dtype=np.uint8))
        return SampleBatch(k, c, mk(n, SHARE_SIZE), mk(n, NAMESPACE_SIZE), mk(n, D, NMT_ROOT_SIZE),
                           mk(n, NMT_ROOT_SIZE), mk(n, 32), mk(n, D + 1, 32))

    def __len__(self) -> int:
        return self.coords.shape[0]

    def arrays(self):
        """The six output arrays in the ABI's order."""
        return (self.shares, self.namespaces, self.nmt_nodes, self.axis_roots, self.leaf_hash, self.aunts)

    def copy(self) -> "SampleBatch":
        return SampleBatch(self.k, self.coords.copy(), *(a.copy() for a in self.arrays()))

    def to_share_proofs(self) -> list:
        """The samples as proof.ShareProof objects (one share each), so that
        validate_share_proofs and the reference's ShareProof.Validate accept
        them.  Only row-axis samples have a reference type: RowProof proves
        rows, a column-axis sample raises ValueError."""
        from .proof import NMTProof, Proof, RowProof, ShareProof
        k, out = self.k, []
        for i, (row, col, axis) in enumerate(self.coords.tolist()):
            if axis != AXIS_ROW:
                raise ValueError(f"sample {i}: a column-axis sample has no ShareProof form (RowProof proves rows)")
            ns = self.namespaces[i].tobytes()
            nodes = [self.nmt_nodes[i, q].tobytes() for q in range(self.nmt_nodes.shape[1])]
            merkle = Proof(4 * k, row, self.leaf_hash[i].tobytes(),
                           [self.aunts[i, q].tobytes() for q in range(self.aunts.shape[1])])
            out.append(ShareProof(data=[self.shares[i].tobytes()], share_proofs=[NMTProof(col, col + 1, nodes)],
                                  namespace_id=ns[1:], row_proof=RowProof([self.axis_roots[i].tobytes()], [merkle],
                                                                          row, row),
                                  namespace_version=ns[0]))
        return out


def sample_proofs(sq, coords, out: SampleBatch | None = None) -> SampleBatch:
    """cda_square_sample_proofs on a proof.ResidentSquare: one launch for the
    whole batch.  `out` (SampleBatch.empty) receives the answer in place."""
    rows, cols, axes = split_coords(coords)
    b = out if out is not None else SampleBatch.empty(sq.k, coords)
    if len(b) != rows.size or b.k != sq.k:
        raise ValueError("output batch does not match the coordinates")
    sq.ctx.check(sq.ctx.lib.cda_square_sample_proofs(sq.h, _u32p(rows), _u32p(cols), ptr(axes), rows.size,
                                                     *(ptr(a) for a in b.arrays())))
    return b


@dataclass
class SetSamples:
    """The answer to samples across a proof.ResidentSquareSet
    (cda_square_set_sample_proofs): ONE flat SampleBatch in request order --
    what verify_samples takes, with data_roots(...) as its per-sample roots --
    and the square each sample came from."""
    batch: SampleBatch
    squares: np.ndarray      # (n,) uint32: the member each sample names

    def __len__(self) -> int:
        return len(self.batch)

    def data_roots(self, set_roots) -> np.ndarray:
        """One data root per sample, (n, 32), from the set's (n_squares, 32) data roots."""
        return np.ascontiguousarray(np.asarray(set_roots, dtype=np.uint8).reshape(-1, 32)[self.squares])

    def by_square(self, verdicts=None):
        """[(square, SampleBatch)] -- with `verdicts`, [(square, SampleBatch,
        verdicts of that batch)] -- one entry per square named, ascending: the
        per-square batches assemble_batch takes.  When the requests are grouped
        by square (the square column is non-decreasing) every batch is a view
        of the flat arrays, no byte is copied; otherwise the samples of a
        square are gathered."""
        sq = self.squares
        v = None if verdicts is None else np.asarray(verdicts).reshape(-1)
        if v is not None and v.size != len(self):
            raise ValueError(f"{len(self)} samples but {v.size} verdicts")
        grouped = bool(np.all(sq[1:] >= sq[:-1]))
        out = []
        for s in np.unique(sq).tolist():
            if grouped:
                lo, hi = np.searchsorted(sq, s, "left"), np.searchsorted(sq, s, "right")
                pick = slice(int(lo), int(hi))
            else:
                pick = np.nonzero(sq == s)[0]
            b = SampleBatch(self.batch.k, self.batch.coords[pick], *(a[pick] for a in self.batch.arrays()))
            out.append((s, b) if v is None else (s, b, v[pick]))
        return out


def split_set_coords(coords):
    """(squares, rows, cols, axes) from an (n, 4) integer array of (square,
    row, col, axis), or (n, 3) of (square, row, col): every sample on the row
    axis.  As split_coords for the values a uint32 / uint8 cannot carry."""
    c = np.asarray(coords, dtype=np.int64)
    if c.size == 0:
        c = c.reshape(0, 4)
    if c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError("coords must be an (n, 4) array of (square, row, col, axis) or an (n, 3) array of "
                         "(square, row, col)")
    bad = np.nonzero((c[:, 0] < 0) | (c[:, 0] >= 1 << 32))[0]
    if bad.size:
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"sample {bad[0]}: square {c[bad[0], 0]} out of range")
    return (np.ascontiguousarray(c[:, 0], dtype=np.uint32),) + split_coords(c[:, 1:])


def sample_proofs_set(sqset, coords, out: SampleBatch | None = None) -> SetSamples:
    """cda_square_set_sample_proofs on a proof.ResidentSquareSet: the samples
    `coords` -- rows of (square, row, col, axis) -- of any number of members
    in one launch.  Returns SetSamples: the flat batch in request order plus
    the square column.  `out` (SampleBatch.empty(k, coords[:, 1:])) receives
    the answer in place."""
    squares, rows, cols, axes = split_set_coords(coords)
    c = np.asarray(coords, dtype=np.int64)
    c = c.reshape(0, 4) if c.size == 0 else c
    b = out if out is not None else SampleBatch.empty(sqset.k, c[:, 1:])
    if len(b) != rows.size or b.k != sqset.k:
        raise ValueError("output batch does not match the coordinates")
    sqset.ctx.check(sqset.ctx.lib.cda_square_set_sample_proofs(sqset.h, _u32p(squares), _u32p(rows), _u32p(cols),
                                                               ptr(axes), rows.size, *(ptr(a) for a in b.arrays())))
    return SetSamples(b, squares)


def verify_samples(batch: SampleBatch, data_root, ctx=None) -> np.ndarray:
    """cda_sample_proofs_verify: a uint8 verdict per sample -- 0 valid, 1 the
    axis root does not verify against the data root, 2 the cell does not verify
    against the axis root.  data_root: one 32-byte root, or one per sample.
    The namespace, leaf position and merkle index are derived from the batch's
    coordinates by the library, never taken from the served arrays."""
    ctx = ctx or default_context()
    n = len(batch)
    roots = np.frombuffer(bytes(data_root), dtype=np.uint8) if isinstance(data_root, (bytes, bytearray, memoryview)) \
        else np.asarray(data_root, dtype=np.uint8).reshape(-1)
    if roots.size == 32:
        roots = np.tile(roots, max(n, 1))
    if roots.size != 32 * max(n, 1):
        raise ValueError(f"{n} samples but {roots.size // 32} data roots")
    roots = np.ascontiguousarray(roots)
    rows, cols, axes = split_coords(batch.coords)
    verdict = np.full(n, 255, dtype=np.uint8)
    arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in
            (batch.shares, batch.nmt_nodes, batch.axis_roots, batch.leaf_hash, batch.aunts)]
    ctx.check(ctx.lib.cda_sample_proofs_verify(ctx.h, batch.k, n, ptr(roots), _u32p(rows), _u32p(cols), ptr(axes),
                                               *(ptr(a) for a in arrs), ptr(verdict)))
    return verdict


def assemble(batch: SampleBatch, verdicts):
    """(eds, present) for cda_repair / ExtendedDataSquare.repair: the (2k, 2k,
    512) square with the cells whose verdict is 0 filled in and marked present
    in the (2k, 2k) mask; every other cell zero and absent.  Duplicate samples
    of one cell are fine: a verified cell is the same bytes every time."""
    W = 2 * batch.k
    v = np.asarray(verdicts).reshape(-1)
    if v.size != len(batch):
        raise ValueError(f"{len(batch)} samples but {v.size} verdicts")
    eds = np.zeros((W, W, SHARE_SIZE), dtype=np.uint8)
    present = np.zeros((W, W), dtype=np.uint8)
    ok = v == 0
    r, c = batch.coords[ok, 0], batch.coords[ok, 1]
    eds[r, c] = batch.shares[ok]
    present[r, c] = 1
    return eds, present


def assemble_batch(batches, verdicts):
    """(eds, present) for cda_repair_batch / rsmt2d.repair_batch: what assemble
    builds for each square, stacked as (n, 2k, 2k, 512) and (n, 2k, 2k), so
    that the verified samples of many heights go to one repair call.  batches:
    one SampleBatch per square, all of one ODS width; verdicts: one verdict
    array per batch."""
    batches, verdicts = list(batches), list(verdicts)
    if len(batches) != len(verdicts):
        raise ValueError(f"{len(batches)} sample batches but {len(verdicts)} verdict arrays")
    if not batches:
        raise ValueError("no sample batch: the square size is unknown")
    k = batches[0].k
    if any(b.k != k for b in batches):
        raise ValueError("the batches are of squares of different sizes; group them by size")
    W, n = 2 * k, len(batches)
    eds = np.zeros((n, W, W, SHARE_SIZE), dtype=np.uint8)
    present = np.zeros((n, W, W), dtype=np.uint8)
    for i, (b, v) in enumerate(zip(batches, verdicts)):
        eds[i], present[i] = assemble(b, v)
    return eds, present
