"""Data-availability samples from resident squares: cda_square_sample_proofs
(any cell of the EDS, row or column axis, one launch per batch),
cda_sample_proofs_verify and the hand-off to cda_repair.

The checker is CPU code built here from the oracle's pieces
(pyref.erasured_leaves, proofs.nmt_range_proof, proofs.rfc_aunts): for a cell
it gives the six arrays the library must return, byte for byte.  Its own
consistency (the proofs verify with the oracle's nmt_verify_inclusion /
rfc_verify, and fail when tampered) is a CPU test.
"""
import ctypes as C

import numpy as np
import pytest

import coracle
import proofs as opr
import pyref
from celestia_da import CdaError, _lib
from test_share_proof_validate import to_dict


def log2(x):
    return x.bit_length() - 1


class Checker:
    """The expected answer to a sample of the square `ods` (k*k, 512), on the CPU."""

    def __init__(self, k, seed=0):
        self.k, self.W = k, 2 * k
        self.ods = coracle.random_square(k, seed)
        eds, rows, cols, root = coracle.extend_dah(self.ods)
        self.eds = eds.reshape(self.W, self.W, 512)
        self.rows, self.cols, self.root = [bytes(r) for r in rows], [bytes(c) for c in cols], root
        self._leaves, self._rfc = {}, {}

    def leaves(self, axis, t):
        if (axis, t) not in self._leaves:
            cells = self.eds[t] if axis == 0 else self.eds[:, t]
            self._leaves[axis, t] = pyref.erasured_leaves([bytes(c) for c in cells], self.k, t)
        return self._leaves[axis, t]

    def namespace(self, row, col, share):
        return bytes(share[:29]) if row < self.k and col < self.k else pyref.PARITY_NS

    def sample(self, row, col, axis):
        """(share, namespace, nodes, axis root, leaf hash, aunts) of cell (row, col) on `axis`."""
        p, t = (col, row) if axis == 0 else (row, col)
        idx = row if axis == 0 else self.W + col
        if idx not in self._rfc:
            self._rfc[idx] = opr.rfc_aunts(self.rows + self.cols, idx)
        lh, aunts = self._rfc[idx]
        share = bytes(self.eds[row, col])
        return (share, self.namespace(row, col, share), opr.nmt_range_proof(self.leaves(axis, t), p, p + 1),
                (self.rows if axis == 0 else self.cols)[t], lh, aunts)

    def arrays(self, coords):
        """The six arrays of a batch, with the ABI's strides."""
        s = [self.sample(*c) for c in np.asarray(coords).tolist()]
        n, D = len(s), log2(self.W)
        u8 = lambda parts, *shape: np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(n, *shape)  # noqa: E731
        assert all(len(x[2]) == D and len(x[5]) == D + 1 for x in s)
        return (u8([x[0] for x in s], 512), u8([x[1] for x in s], 29), u8([b"".join(x[2]) for x in s], D, 90),
                u8([x[3] for x in s], 90), u8([x[4] for x in s], 32), u8([b"".join(x[5]) for x in s], D + 1, 32))


def oracle_verdict(k, root, row, col, axis, share, nodes, axis_root, leaf_hash, aunts):
    """What cda_sample_proofs_verify must say, from the oracle's verifiers: everything but the served bytes is
    derived from the claimed (row, col, axis)."""
    idx, p = (row, col) if axis == 0 else (2 * k + col, row)
    if not opr.merkle_proof_verify(root, 4 * k, idx, leaf_hash, aunts, axis_root):
        return 1
    ns = bytes(share[:29]) if row < k and col < k else pyref.PARITY_NS
    return 0 if opr.nmt_verify_inclusion(axis_root, nodes, p, p + 1, ns, [bytes(share)]) else 2


def batch_verdicts(batch, roots):
    out = []
    for i, (row, col, axis) in enumerate(batch.coords.tolist()):
        out.append(oracle_verdict(batch.k, bytes(roots[i]), row, col, axis, batch.shares[i].tobytes(),
                                  [batch.nmt_nodes[i, q].tobytes() for q in range(batch.nmt_nodes.shape[1])],
                                  batch.axis_roots[i].tobytes(), batch.leaf_hash[i].tobytes(),
                                  [batch.aunts[i, q].tobytes() for q in range(batch.aunts.shape[1])]))
    return out


def all_cells(k):
    W = 2 * k
    return np.array([(r, c, a) for a in (0, 1) for r in range(W) for c in range(W)], dtype=np.int64)


_checkers = {}


def checker(k):
    """One square per k, computed once and never changed."""
    if k not in _checkers:
        _checkers[k] = Checker(k)
    return _checkers[k]


@pytest.fixture(scope="module")
def resident(ctx):
    """ResidentSquare of checker(k), one per k for the whole module."""
    from celestia_da import proof as gpr
    made = {}

    def get(k):
        if k not in made:
            made[k] = gpr.ResidentSquare(checker(k).ods, ctx)
        return made[k]
    yield get
    for sq in made.values():
        sq.close()


def assert_batch_equals(batch, want):
    for name, got, exp in zip(("shares", "namespaces", "nmt_nodes", "axis_roots", "leaf_hash", "aunts"),
                              batch.arrays(), want):
        assert got.shape == exp.shape, name
        bad = np.nonzero((got != exp).reshape(len(batch), -1).any(axis=1))[0]
        assert bad.size == 0, (name, "first differing sample", batch.coords[bad[0]].tolist())


# ------------------------------------------------------------------ CPU tests
def test_checker_self_consistent():
    """k = 2, every cell on both axes: D nodes, the NMT proof verifies under the namespace rule and fails with
    one share byte flipped, the merkle proof verifies with Index row / 2k + col."""
    k = 2
    ch = checker(k)
    for row, col, axis in all_cells(k).tolist():
        share, ns, nodes, axis_root, lh, aunts = ch.sample(row, col, axis)
        p = col if axis == 0 else row
        assert len(nodes) == log2(2 * k) and len(aunts) == log2(4 * k)
        assert ns == (share[:29] if row < k and col < k else b"\xff" * 29)
        assert opr.nmt_verify_inclusion(axis_root, nodes, p, p + 1, ns, [share])
        flipped = bytearray(share)
        flipped[100] ^= 1
        assert not opr.nmt_verify_inclusion(axis_root, nodes, p, p + 1, ns, [bytes(flipped)])
        idx = row if axis == 0 else 2 * k + col
        assert opr.merkle_proof_verify(ch.root, 4 * k, idx, lh, aunts, axis_root)
        assert not opr.rfc_verify(ch.root, 4 * k, idx ^ 1, lh, aunts)
        assert oracle_verdict(k, ch.root, row, col, axis, share, nodes, axis_root, lh, aunts) == 0


def test_closed_form_node_order():
    """The order the kernel uses (left siblings top-down where bit L of p is set, then right siblings bottom-up
    where it is clear) is nmt's depth-first order, for every leaf of trees of 2 .. 32 leaves."""
    for D in range(1, 6):
        W = 1 << D
        # nodes named by (level, index) instead of hashed: the same recursion as nmt_range_proof
        def proof(p, lo=0, hi=None, level=None):
            hi, level = (W, D) if hi is None else (hi, level)
            if hi <= p or lo > p:
                return [(level, lo >> level)]
            if hi - lo == 1:
                return []
            mid = (lo + hi) // 2
            return proof(p, lo, mid, level - 1) + proof(p, mid, hi, level - 1)
        for p in range(W):
            closed = [(L, (p >> L) ^ 1) for L in range(D - 1, -1, -1) if p >> L & 1] + \
                     [(L, (p >> L) ^ 1) for L in range(D) if not p >> L & 1]
            assert proof(p) == closed, (D, p)


def test_sampling_module_and_symbols():
    import celestia_da
    from celestia_da import sampling
    assert celestia_da.sampling is sampling
    assert {"cda_square_sample_proofs", "cda_sample_proofs_verify"} <= set(_lib.EXPORTED)
    for name in ("SampleBatch", "sample_proofs", "verify_samples", "assemble"):
        assert hasattr(sampling, name), name
    assert hasattr(celestia_da.proof.ResidentSquare, "sample_proofs")


def test_assemble_and_to_share_proofs_host_side():
    """assemble / to_share_proofs need no GPU: verdict 0 cells present (duplicates fine), the rest absent; a
    column-axis sample has no ShareProof form."""
    from celestia_da import sampling
    k = 2
    ch = checker(k)
    coords = np.array([(0, 0, 0), (3, 1, 1), (0, 0, 1), (2, 2, 0)], dtype=np.int64)
    b = sampling.SampleBatch(k, coords, *ch.arrays(coords))
    eds, present = sampling.assemble(b, [0, 2, 0, 1])
    assert present.sum() == 1 and present[0, 0] == 1
    assert np.array_equal(eds[0, 0], ch.eds[0, 0]) and not eds[3, 1].any() and not eds[2, 2].any()
    with pytest.raises(ValueError):
        b.to_share_proofs()
    rows_only = sampling.SampleBatch(k, coords[[0, 3]], *ch.arrays(coords[[0, 3]]))
    for sp in rows_only.to_share_proofs():
        assert opr.share_proof_validate(to_dict(sp), ch.root) is None


# ------------------------------------------------------- GPU: byte for byte
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 8])
def test_every_cell_both_axes(resident, k):
    coords = all_cells(k)
    batch = resident(k).sample_proofs(coords)
    assert batch.k == k and len(batch) == 8 * k * k
    assert batch.nmt_nodes.shape == (len(batch), log2(2 * k), 90) and batch.aunts.shape[1] == log2(4 * k)
    assert_batch_equals(batch, checker(k).arrays(coords))


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", [(32, 257), (128, 64)])
def test_seeded_samples_larger_k(resident, k, n):
    rng = np.random.default_rng(1000 + k)
    coords = np.stack([rng.integers(0, 2 * k, n), rng.integers(0, 2 * k, n), rng.integers(0, 2, n)], axis=1)
    coords[n // 2:n // 2 + 5] = coords[:5]          # repeats
    coords[-1] = (2 * k - 1, 2 * k - 1, 1)          # the last cell: the largest level offsets
    coords[-2] = (2 * k - 1, 0, 0)
    batch = resident(k).sample_proofs(coords)
    assert_batch_equals(batch, checker(k).arrays(coords))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5, 63, 65, 257])
def test_batch_sizes(resident, n):
    k = 8
    rng = np.random.default_rng(n)
    coords = np.stack([rng.integers(0, 2 * k, n), rng.integers(0, 2 * k, n), rng.integers(0, 2, n)], axis=1)
    assert_batch_equals(resident(k).sample_proofs(coords), checker(k).arrays(coords))
    # axes = NULL: every sample on the row axis
    batch = resident(k).sample_proofs(coords[:, :2])
    rows_axis = coords.copy()
    rows_axis[:, 2] = 0
    assert np.array_equal(batch.coords, rows_axis)
    assert_batch_equals(batch, checker(k).arrays(rows_axis))


@pytest.mark.gpu
def test_equals_share_proof_path(resident):
    """k = 4: every Q0 cell on the row axis equals ResidentSquare.share_proof of that one share, field for
    field (that path is pinned by the reference's own vectors)."""
    k = 4
    sq = resident(k)
    coords = np.array([(r, c, 0) for r in range(k) for c in range(k)], dtype=np.int64)
    got = sq.sample_proofs(coords).to_share_proofs()
    for (r, c, _), sp in zip(coords.tolist(), got):
        ns = bytes(checker(k).eds[r, c, :29])
        assert sp == sq.share_proof(ns, r * k + c, r * k + c + 1), (r, c)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8])
def test_column_roots_and_dah_unchanged(resident, k):
    ch = checker(k)
    sq = resident(k)
    assert sq.dah() == (ch.rows, ch.cols, ch.root)
    coords = np.array([(r, c, 1) for r in (0, 2 * k - 1) for c in range(2 * k)], dtype=np.int64)
    batch = sq.sample_proofs(coords)
    _, cols, _ = sq.dah()
    for (r, c, _), root in zip(coords.tolist(), batch.axis_roots):
        assert root.tobytes() == cols[c]


@pytest.mark.gpu
def test_push_order_square_serves_samples(ctx):
    """A square whose Q0 is not namespace ordered is still created (CDA_ERR_PUSH_ORDER) and serves samples:
    its trees are the BlindTree ones."""
    from celestia_da import proof as gpr
    from celestia_da import sampling
    k = 2
    ods = checker(k).ods.copy()
    ods[[0, 1]] = ods[[1, 0]]   # swap two cells of row 0: out of order unless they share a namespace
    assert bytes(ods[0, :29]) > bytes(ods[1, :29])
    sq = gpr.ResidentSquare(ods, ctx)
    try:
        assert sq.push_order_error
        eds = sq.eds()
        rows, cols, root = sq.dah()
        coords = all_cells(k)
        batch = sq.sample_proofs(coords)
        for i, (r, c, a) in enumerate(coords.tolist()):
            cells, t, p = (eds[r], r, c) if a == 0 else (eds[:, c], c, r)
            leaves = pyref.erasured_leaves([bytes(x) for x in cells], k, t, blind=True)
            assert [batch.nmt_nodes[i, q].tobytes() for q in range(2)] == opr.nmt_range_proof(leaves, p, p + 1)
            assert batch.axis_roots[i].tobytes() == (rows if a == 0 else cols)[t]
            assert batch.shares[i].tobytes() == bytes(eds[r, c])
        # the hashing never depended on the order: the samples verify
        assert sampling.verify_samples(batch, root, ctx).tolist() == batch_verdicts(batch, [root] * len(batch))
    finally:
        sq.close()


# ------------------------------------------------------------ GPU: verification
@pytest.mark.gpu
def test_valid_samples_verify(ctx, resident):
    from celestia_da import proof as gpr
    from celestia_da import sampling
    k = 8
    ch = checker(k)
    coords = all_cells(k)
    batch = resident(k).sample_proofs(coords)
    v = sampling.verify_samples(batch, ch.root, ctx)
    assert v.dtype == np.uint8 and v.shape == (512,) and not v.any()
    assert not sampling.verify_samples(batch, np.tile(np.frombuffer(ch.root, dtype=np.uint8), (512, 1)), ctx).any()
    row_half = sampling.SampleBatch(k, coords[:256], *(a[:256] for a in batch.arrays()))
    sps = row_half.to_share_proofs()
    assert gpr.validate_share_proofs(sps, [ch.root] * len(sps), ctx) == [None] * len(sps)
    for sp in sps:
        assert opr.share_proof_validate(to_dict(sp), ch.root) is None
    with pytest.raises(ValueError):
        batch.to_share_proofs()


@pytest.mark.gpu
def test_tampered_samples(ctx, resident):
    """One batch, single samples tampered, their neighbours valid: every verdict is what the oracle's
    nmt_verify_inclusion / rfc_verify give for the same fields."""
    from celestia_da import sampling
    k = 8
    ch = checker(k)
    # Q0, Q1, Q2, Q3 cells on both axes; the tampered ones sit at 1, 4, 7, ... with valid samples between
    cells = [(1, 2), (3, 12), (11, 5), (13, 14), (0, 7), (7, 0), (15, 3), (6, 9), (2, 2), (15, 15)]
    coords = np.array([(r, c, a) for r, c in cells for a in (0, 1, 0)], dtype=np.int64)
    b = resident(k).sample_proofs(coords).copy()
    expected, roots, want = tamper(b, ch.root)
    got = sampling.verify_samples(b, roots, ctx)
    assert got.tolist() == expected


def tamper(b, root):
    """Tampers the 30-sample batch of test_tampered_samples in place; returns the oracle's verdicts, the data
    roots and the verdicts the issue names for the tampered samples."""
    k, n, D = b.k, len(b), b.nmt_nodes.shape[1]
    roots = np.tile(np.frombuffer(root, dtype=np.uint8), (n, 1)).copy()
    want = {}
    b.shares[1, 100] ^= 1             # a share byte
    want[1] = 2
    b.nmt_nodes[4, 0, 70] ^= 1        # the first proof node
    want[4] = 2
    b.nmt_nodes[7, D - 1, 3] ^= 1     # the last proof node
    want[7] = 2
    b.axis_roots[10, 58 + 9] ^= 1     # the axis root's digest
    want[10] = 1
    b.aunts[13, 2, 31] ^= 1           # an aunt
    want[13] = 1
    roots[16, 0] ^= 1                 # a wrong data root
    want[16] = 1
    assert b.coords[18, 2] == 0
    b.coords[18, 1] += 1              # claimed column + 1 on a row-axis sample
    want[18] = 2
    b.coords[22, 2] ^= 1              # claimed axis flipped: whatever the oracle says, but not valid
    r, c, a = b.coords[24].tolist()
    assert r < k and c < k and a == 0
    b.coords[24, 1] = c + k           # a Q0 cell claimed at a parity coordinate: the namespace rule
    want[24] = 2
    expected = batch_verdicts(b, roots)
    for i, w in want.items():
        assert expected[i] == w, (i, expected[i], w)
    assert expected[22] != 0
    assert [i for i, e in enumerate(expected) if e] == sorted(list(want) + [22])
    return expected, roots, want


def test_tamper_cases_on_the_checker():
    """The tampering of test_tampered_samples applied to the checker's own (valid) batch: the oracle gives the
    verdicts the cases are named for, and every untouched neighbour stays valid.  No GPU."""
    from celestia_da import sampling
    k = 8
    ch = checker(k)
    cells = [(1, 2), (3, 12), (11, 5), (13, 14), (0, 7), (7, 0), (15, 3), (6, 9), (2, 2), (15, 15)]
    coords = np.array([(r, c, a) for r, c in cells for a in (0, 1, 0)], dtype=np.int64)
    b = sampling.SampleBatch(k, coords.copy(), *(a.copy() for a in ch.arrays(coords)))
    assert batch_verdicts(b, [ch.root] * len(b)) == [0] * len(b)
    expected, _, want = tamper(b, ch.root)
    assert all(expected[i] == w for i, w in want.items())


# ------------------------------------------------------------------ GPU: flow
def _outside_q0(k):
    W = 2 * k
    cells = [(r, c) for r in range(W) for c in range(W) if not (r < k and c < k)]
    return np.array([(r, c, i & 1) for i, (r, c) in enumerate(cells)], dtype=np.int64)


def _repair(ctx, eds, present, rows, cols):
    from celestia_da import rsmt2d, wrapper
    sq = rsmt2d.new_extended_data_square_with_missing(eds, present, rsmt2d.LeoRSCodec(ctx),
                                                     wrapper.new_constructor(eds.shape[0] // 2))
    sq.repair(rows, cols, present)
    return sq.array().reshape(eds.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("tamper", [(), (5, 100)])
def test_serve_verify_repair(ctx, resident, tamper):
    """k = 8: the 192 cells outside Q0 are sampled (axes alternating), verified, assembled and repaired with the
    square's roots; with two samples tampered their cells are absent and the repair still succeeds."""
    from celestia_da import sampling
    k = 8
    sq = resident(k)
    coords = _outside_q0(k)
    assert len(coords) == 192
    batch = sq.sample_proofs(coords).copy()
    for i in tamper:
        batch.shares[i, 200] ^= 0x80
    rows, cols, root = sq.dah()
    v = sampling.verify_samples(batch, root, ctx)
    assert [i for i in range(192) if v[i]] == list(tamper) and all(v[i] == 2 for i in tamper)
    eds, present = sampling.assemble(batch, v)
    assert present.sum() == 192 - len(tamper) and not present[:k, :k].any()
    for i in tamper:
        assert present[coords[i, 0], coords[i, 1]] == 0
    assert np.array_equal(_repair(ctx, eds, present, rows, cols), sq.eds())


# ---------------------------------------------------------------- GPU: errors
@pytest.mark.gpu
@pytest.mark.parametrize("bad,field", [((16, 0, 0), "row"), ((0, 16, 1), "col"), ((3, 3, 2), "axis")])
def test_bad_coordinates(resident, bad, field):
    from celestia_da import sampling
    k = 8
    coords = np.array([(1, 1, 0), (2, 3, 1), bad, (4, 4, 0)], dtype=np.int64)
    out = sampling.SampleBatch.empty(k, coords, fill=0xAA)
    with pytest.raises(CdaError) as e:
        resident(k).sample_proofs(coords, out=out)
    assert e.value.code == _lib.CDA_ERR_INVALID
    assert "sample 2" in str(e.value) and field in str(e.value)
    for a in out.arrays():
        assert (a == 0xAA).all()


@pytest.mark.gpu
def test_empty_batch_and_verify_errors(ctx, resident):
    from celestia_da import sampling
    from celestia_da._lib import ptr
    k = 8
    sq = resident(k)
    assert len(sq.sample_proofs(np.zeros((0, 3), dtype=np.int64))) == 0
    assert ctx.lib.cda_square_sample_proofs(sq.h, None, None, None, 0, None, None, None, None, None, None) == _lib.CDA_OK
    coords = np.array([(1, 1, 0), (9, 3, 1)], dtype=np.int64)
    b = sq.sample_proofs(coords)
    roots = np.tile(np.frombuffer(checker(k).root, dtype=np.uint8), 2)
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)   # noqa: E731
    u32p = C.POINTER(C.c_uint32)

    def call(kk, rows, cols, axes):
        verdict = np.full(2, 0xAA, dtype=np.uint8)
        rows, cols, axes = u32(rows), u32(cols), np.ascontiguousarray(axes, dtype=np.uint8)
        rc = ctx.lib.cda_sample_proofs_verify(ctx.h, kk, 2, ptr(roots), rows.ctypes.data_as(u32p),
                                              cols.ctypes.data_as(u32p), ptr(axes), ptr(b.shares),
                                              ptr(b.nmt_nodes), ptr(b.axis_roots), ptr(b.leaf_hash), ptr(b.aunts),
                                              ptr(verdict))
        return rc, verdict.tolist(), ctx.lib.cda_last_error(ctx.h).decode()

    assert call(k, coords[:, 0], coords[:, 1], coords[:, 2])[:2] == (_lib.CDA_OK, [0, 0])
    assert call(3, coords[:, 0], coords[:, 1], coords[:, 2])[:2] == (_lib.CDA_ERR_INVALID, [0xAA, 0xAA])
    rc, verdict, msg = call(k, [1, 16], coords[:, 1], coords[:, 2])
    assert (rc, verdict) == (_lib.CDA_ERR_INVALID, [0xAA, 0xAA]) and "sample 1" in msg and "row" in msg
    assert sampling.verify_samples(sampling.SampleBatch.empty(k, np.zeros((0, 3))), checker(k).root, ctx).size == 0
