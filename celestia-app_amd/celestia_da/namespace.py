"""All shares of a namespace, with proof that none was left out (libcda.so).

What namespaced Merkle trees are for: a rollup asks a node for its namespace's
data in a block and checks the answer against the DataAvailabilityHeader alone.

    batch = ResidentSquare(ods).namespace_proofs(namespaces)   # cda_square_namespace_plan + _proofs
    verdicts = batch.verify(row_roots)                         # cda_namespace_proofs_verify
    answer = get_shares_by_namespace(ods, ns)                  # [(row, NMTProof, shares)]
    verify_namespaced_shares(row_roots, ns, answer) == 0

and the same over a range of heights, a proof.ResidentSquareSet, in the launches
of one square's call:

    got = sqset.namespace_proofs([(square, ns), ...])          # cda_square_set_namespace_plan + _proofs
    verdicts = got.verify(sqset.dah()[0])                      # cda_namespace_proofs_verify_set
    answers = get_shares_by_namespace_set(sqset, ns)           # one answer per member
    verify_namespaced_shares_set(row_roots, squares, ns, answers)

Reference: nmt v0.22.0 NamespacedMerkleTree.ProveNamespace (an inclusion proof
of the whole run of the namespace in a row, or an absence proof: the proof of
the first leaf above it, carried as NMTProof.leaf_hash) and
Proof.VerifyNamespace (VerifyLeafHashes with verifyCompleteness), and the row
selection of GetSharesByNamespace on the DAH: a row takes part iff
min(rowRoot) <= namespace <= max(rowRoot).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NAMESPACE_SIZE, NMT_ROOT_SIZE, SHARE_SIZE, default_context, ptr

INCLUSION = _lib.CDA_NAMESPACE_INCLUSION
ABSENCE = _lib.CDA_NAMESPACE_ABSENCE


def _namespaces_array(namespaces) -> np.ndarray:
    """(n, 29) uint8 from 29-byte namespaces (bytes, or rows of an array)."""
    if isinstance(namespaces, np.ndarray):
        a = np.ascontiguousarray(namespaces, dtype=np.uint8).reshape(-1, NAMESPACE_SIZE)
    else:
        parts = [bytes(x) for x in namespaces]
        for i, x in enumerate(parts):
            if len(x) != NAMESPACE_SIZE:
                raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"query {i}: namespace of {len(x)} bytes, not {NAMESPACE_SIZE}")
        a = np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(-1, NAMESPACE_SIZE).copy()
    return a


def namespace_plan(sq, namespaces) -> dict:
    """cda_square_namespace_plan: n_segments, n_nodes and n_shares of the answer
    to `namespaces` from the resident square `sq` (one search launch)."""
    ns = _namespaces_array(namespaces)
    p = _lib.NamespacePlanT()
    sq.ctx.check(sq.ctx.lib.cda_square_namespace_plan(sq.h, ptr(ns), len(ns), C.byref(p)))
    return {n: getattr(p, n) for n, _ in _lib.NamespacePlanT._fields_}


class NamespaceProofsBatch:
    """The answers to n namespace queries of one square as the flat arrays of
    cda_namespace_proofs_out (numpy; include/cda.h): query i owns the segments
    (rows) seg_off[i] .. seg_off[i + 1], segment g the nodes node_off[g] ..
    node_off[g + 1] and the shares share_off[g] .. share_off[g + 1]."""

    FIELDS = ("seg_off", "row", "kind", "nmt_start", "nmt_end", "node_off", "nodes", "share_off", "shares",
              "absence_leaf")

    def __init__(self, k, namespaces, **arrays):
        self.k, self.namespaces = k, _namespaces_array(namespaces)
        for name in self.FIELDS:
            setattr(self, name, arrays[name])

    @classmethod
    def empty(cls, k, namespaces, plan, fill=None):
        """Buffers of the plan's sizes (filled with the byte `fill` if given)."""
        ns = _namespaces_array(namespaces)
        n, S = len(ns), plan["n_segments"]
        shapes = {"seg_off": ((n + 1,), np.uint32), "row": ((S,), np.uint32), "kind": ((S,), np.uint8),
                  "nmt_start": ((S,), np.int32), "nmt_end": ((S,), np.int32), "node_off": ((S + 1,), np.uint32),
                  "nodes": ((plan["n_nodes"], NMT_ROOT_SIZE), np.uint8), "share_off": ((S + 1,), np.uint64),
                  "shares": ((plan["n_shares"], SHARE_SIZE), np.uint8),
                  "absence_leaf": ((S, NMT_ROOT_SIZE), np.uint8)}
        arrays = {}
        for name, (shape, dtype) in shapes.items():
            a = np.empty(shape, dtype=dtype)
            if fill is not None:
                a.view(np.uint8).fill(fill)
            arrays[name] = a
        return cls(k, ns, **arrays)

    @classmethod
    def from_answers(cls, k, namespaces, answers):
        """The batch of `answers`, one per namespace, each a list of (row,
        NMTProof, shares) as .answers() returns them.  A proof with a leaf_hash
        is an absence segment."""
        ns = _namespaces_array(namespaces)
        if len(answers) != len(ns):
            raise ValueError(f"{len(ns)} namespaces but {len(answers)} answers")
        segs = [s for a in answers for s in a]
        counts = lambda xs: np.cumsum([0] + list(xs), dtype=np.int64)   # noqa: E731
        cat = lambda parts, width: np.frombuffer(b"".join(bytes(x) for x in parts), dtype=np.uint8).reshape(  # noqa: E731
            -1, width).copy()
        return cls(k, ns,
                   seg_off=counts(len(a) for a in answers).astype(np.uint32),
                   row=np.array([r for r, _, _ in segs], dtype=np.uint32),
                   kind=np.array([ABSENCE if p.leaf_hash else INCLUSION for _, p, _ in segs], dtype=np.uint8),
                   nmt_start=np.array([p.start for _, p, _ in segs], dtype=np.int32),
                   nmt_end=np.array([p.end for _, p, _ in segs], dtype=np.int32),
                   node_off=counts(len(p.nodes) for _, p, _ in segs).astype(np.uint32),
                   nodes=cat([x for _, p, _ in segs for x in p.nodes], NMT_ROOT_SIZE),
                   share_off=counts(len(sh) for _, _, sh in segs).astype(np.uint64),
                   shares=cat([x for _, _, sh in segs for x in sh], SHARE_SIZE),
                   absence_leaf=cat([p.leaf_hash or bytes(NMT_ROOT_SIZE) for _, p, _ in segs], NMT_ROOT_SIZE))

    def __len__(self):
        return len(self.namespaces)

    def arrays(self):
        return tuple(getattr(self, name) for name in self.FIELDS)

    def out_struct(self, skip=()):
        """cda_namespace_proofs_out over the arrays (NULL for the names in `skip`)."""
        o = _lib.NamespaceProofsOut()
        for (name, t), a in zip(_lib.NamespaceProofsOut._fields_, self.arrays()):
            assert name in self.FIELDS
            if name not in skip:
                setattr(o, name, a.ctypes.data_as(t))
        return o

    def batch(self):
        """The cda_namespace_proof_batch over these arrays, unchanged: pointer
        assignment, no per-query objects."""
        b = _lib.NamespaceProofBatch()
        b.n_queries = len(self)
        b.namespaces = ptr(self.namespaces)
        for name, t in _lib.NamespaceProofBatch._fields_:
            if name in self.FIELDS:
                setattr(b, name, getattr(self, name).ctypes.data_as(t))
        b.n_nodes, b.n_shares = len(self.nodes), len(self.shares)
        b._keep = self   # the struct borrows the arrays
        return b

    def verify(self, row_roots, ctx=None) -> np.ndarray:
        """cda_namespace_proofs_verify against the DAH's 2k row roots (a list
        of 90-byte roots or an array): verdict per query -- 0 valid, 1 the rows
        are not the ones the DAH selects, 2 a segment does not hash to its row
        root (or an absence leaf is not above the namespace), 3 incomplete."""
        ctx = ctx or default_context()
        roots = _roots_array(row_roots)
        verdict = np.full(max(1, len(self)), 255, dtype=np.uint8)
        b = self.batch()
        ctx.check(ctx.lib.cda_namespace_proofs_verify(ctx.h, self.k, ptr(roots), C.byref(b), ptr(verdict)))
        return verdict[:len(self)]

    def answers(self) -> list:
        """One answer per query: a list, in row order, of (row, NMTProof(start,
        end, nodes, leaf_hash), shares); leaf_hash is set only for absence."""
        from .proof import NMTProof
        nb, sb, lb = self.nodes.tobytes(), self.shares.tobytes(), self.absence_leaf.tobytes()
        seg_off, node_off, share_off = self.seg_off.tolist(), self.node_off.tolist(), self.share_off.tolist()
        cut = lambda b, lo, hi, sz: [b[i * sz:(i + 1) * sz] for i in range(lo, hi)]  # noqa: E731
        out = []
        for i in range(len(self)):
            ans = []
            for g in range(seg_off[i], seg_off[i + 1]):
                leaf = lb[g * NMT_ROOT_SIZE:(g + 1) * NMT_ROOT_SIZE] if self.kind[g] == ABSENCE else b""
                ans.append((int(self.row[g]),
                            NMTProof(int(self.nmt_start[g]), int(self.nmt_end[g]),
                                     cut(nb, node_off[g], node_off[g + 1], NMT_ROOT_SIZE), leaf),
                            cut(sb, share_off[g], share_off[g + 1], SHARE_SIZE)))
            out.append(ans)
        return out


def _roots_array(row_roots) -> np.ndarray:
    if isinstance(row_roots, np.ndarray):
        return np.ascontiguousarray(row_roots, dtype=np.uint8).reshape(-1)
    return np.frombuffer(b"".join(bytes(r) for r in row_roots), dtype=np.uint8).copy()


def namespace_proofs(sq, namespaces, out: NamespaceProofsBatch | None = None) -> NamespaceProofsBatch:
    """cda_square_namespace_plan, then cda_square_namespace_proofs into buffers
    of the plan's sizes (or into `out`, a NamespaceProofsBatch.empty)."""
    ns = _namespaces_array(namespaces)
    if out is None:
        out = NamespaceProofsBatch.empty(sq.k, ns, namespace_plan(sq, ns))
    o = out.out_struct()
    sq.ctx.check(sq.ctx.lib.cda_square_namespace_proofs(sq.h, ptr(ns), len(ns), C.byref(o)))
    return out


# ------------------------------------------------- the same across a set of squares
def split_set_queries(queries):
    """(squares, namespaces) as (n,) uint32 and (n, 29) uint8 arrays from rows
    of (square, namespace): an iterable of (int, 29 bytes) pairs, or an (n, 30)
    integer array whose first column is the square."""
    if isinstance(queries, np.ndarray):
        q = np.asarray(queries, dtype=np.int64).reshape(-1, 1 + NAMESPACE_SIZE)
        sq, ns = q[:, 0], np.ascontiguousarray(q[:, 1:], dtype=np.uint8)
    else:
        rows = list(queries)
        sq = np.array([int(s) for s, _ in rows], dtype=np.int64)
        ns = _namespaces_array([x for _, x in rows])
    bad = np.nonzero((sq < 0) | (sq >= 1 << 32))[0]
    if bad.size:
        raise _lib.CdaError(_lib.CDA_ERR_INVALID, f"query {bad[0]}: square {sq[bad[0]]} out of range")
    return np.ascontiguousarray(sq, dtype=np.uint32), ns


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def namespace_plan_set(sqset, queries) -> dict:
    """cda_square_set_namespace_plan: the sizes of the answer to `queries`,
    rows of (square, namespace), from a proof.ResidentSquareSet."""
    return _plan_set(sqset, *split_set_queries(queries))


def _plan_set(sqset, squares: np.ndarray, ns: np.ndarray) -> dict:
    p = _lib.NamespacePlanT()
    sqset.ctx.check(sqset.ctx.lib.cda_square_set_namespace_plan(sqset.h, _u32p(squares), ptr(ns), len(ns), C.byref(p)))
    return {n: getattr(p, n) for n, _ in _lib.NamespacePlanT._fields_}


class SetNamespaceProofs:
    """The answer to namespace queries across a proof.ResidentSquareSet
    (cda_square_set_namespace_proofs): ONE flat NamespaceProofsBatch in request
    order and the square each query names."""

    def __init__(self, batch: NamespaceProofsBatch, squares):
        self.batch, self.squares = batch, np.ascontiguousarray(squares, dtype=np.uint32)

    def __len__(self) -> int:
        return len(self.batch)

    def answers(self) -> list:
        """One answer per query, as NamespaceProofsBatch.answers()."""
        return self.batch.answers()

    def verify(self, row_roots, ctx=None) -> np.ndarray:
        """cda_namespace_proofs_verify_set: query q against the DAH squares[q]
        of `row_roots`, the (n_squares, 2k, 90) array of ResidentSquareSet.dah()
        or of trusted DAHs.  Verdicts as NamespaceProofsBatch.verify."""
        ctx = ctx or default_context()
        roots = np.ascontiguousarray(row_roots, dtype=np.uint8).reshape(-1)
        per_dah = 2 * self.batch.k * NMT_ROOT_SIZE
        if roots.size % per_dah:
            raise ValueError(f"{roots.size} bytes of row roots are no whole number of DAHs of {per_dah}")
        verdict = np.full(max(1, len(self)), 255, dtype=np.uint8)
        b = self.batch.batch()
        ctx.check(ctx.lib.cda_namespace_proofs_verify_set(ctx.h, self.batch.k, ptr(roots), roots.size // per_dah,
                                                          _u32p(self.squares), C.byref(b), ptr(verdict)))
        return verdict[:len(self)]


def namespace_proofs_set(sqset, queries, out: NamespaceProofsBatch | None = None) -> SetNamespaceProofs:
    """cda_square_set_namespace_plan, then cda_square_set_namespace_proofs into
    buffers of the plan's sizes (or into `out`, a NamespaceProofsBatch.empty):
    the queries -- rows of (square, namespace) -- of any number of members in
    the launches of one square's call."""
    squares, ns = split_set_queries(queries)
    if out is None:
        out = NamespaceProofsBatch.empty(sqset.k, ns, _plan_set(sqset, squares, ns))
    o = out.out_struct()
    sqset.ctx.check(sqset.ctx.lib.cda_square_set_namespace_proofs(sqset.h, _u32p(squares), ptr(ns), len(ns),
                                                                  C.byref(o)))
    return SetNamespaceProofs(out, squares)


def get_shares_by_namespace_set(sqset, namespace: bytes, squares=None) -> list:
    """GetSharesByNamespace over a range of heights in one call: one answer
    (as get_shares_by_namespace) per member named in `squares`, by default all
    of them."""
    squares = list(range(len(sqset))) if squares is None else [int(s) for s in squares]
    return namespace_proofs_set(sqset, [(s, namespace) for s in squares]).answers()


def verify_namespaced_shares_set(row_roots, squares, namespaces, answers, ctx=None) -> np.ndarray:
    """The verdicts of cda_namespace_proofs_verify_set for answers of
    get_shares_by_namespace_set: answer q is of `namespaces[q]` (one namespace
    for all: 29 bytes) and is checked against the DAH squares[q] of `row_roots`,
    (n_squares, 2k, 90).  0 means that these are all the shares of the
    namespace in that square."""
    roots = np.ascontiguousarray(row_roots, dtype=np.uint8)
    if roots.ndim != 3 or roots.shape[2] != NMT_ROOT_SIZE:
        raise ValueError("row_roots must have the shape (n_squares, 2k, 90)")
    k = roots.shape[1] // 2
    if isinstance(namespaces, (bytes, bytearray)):
        namespaces = [bytes(namespaces)] * len(answers)
    batch = NamespaceProofsBatch.from_answers(k, namespaces, answers)
    return SetNamespaceProofs(batch, np.asarray(squares, dtype=np.uint32)).verify(roots, ctx)


def get_shares_by_namespace(ods_or_square, namespace: bytes, ctx=None) -> list:
    """GetSharesByNamespace: the rows of the square that may hold `namespace`,
    each as (row, NMTProof, shares) -- the row's shares of the namespace with
    their inclusion proof, or no shares and an absence proof."""
    from .proof import ResidentSquare
    if isinstance(ods_or_square, ResidentSquare):
        return ods_or_square.namespace_proofs([namespace]).answers()[0]
    sq = ResidentSquare(ods_or_square, ctx)
    try:
        return sq.namespace_proofs([namespace]).answers()[0]
    finally:
        sq.close()


def verify_namespaced_shares(row_roots, namespace: bytes, answer, ctx=None) -> int:
    """The verdict of cda_namespace_proofs_verify for one answer of
    get_shares_by_namespace against the DAH's 2k row roots: 0 means that these
    are all the shares of `namespace` in the square."""
    roots = _roots_array(row_roots)
    k = roots.size // (2 * NMT_ROOT_SIZE)
    return int(NamespaceProofsBatch.from_answers(k, [namespace], [answer]).verify(roots, ctx)[0])
