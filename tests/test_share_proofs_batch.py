"""Share proofs of many ranges of a resident square in one launch:
cda_square_share_proofs (csrc/share_proofs.hip) and its Python surface
(ResidentSquare.share_proofs_batch, new_share_inclusion_proofs,
new_tx_inclusion_proofs).

The single-range call, cda_square_share_proof, is a front end of the same
kernel (n = 1, its own buffer layout), so it is tested here too.  The
yardstick of both is the oracle, on the CPU: the EDS and the roots of
coracle.extend_dah, the leaf nodes of pyref.erasured_leaves, the proof nodes
of proofs.nmt_range_proof and the merkle proofs of proofs.rfc_aunts
(oracle_range).  Every array of a batch, cut by the batch's offsets, and every
buffer of a single call equals those bytes.  No tolerances.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import coracle
import proofs as opr
import pyref
from celestia_da import CdaError, _lib
from celestia_da._lib import ptr
from test_proofs import constructed_square, oracle_eds
from test_share_proof_validate import to_dict

# squares of exactly k x k shares with several namespaces: (blob txs, blob sizes) for constructed_square
SMALL = {1: (0, (1, 2)), 2: (2, (1, 400)), 4: (4, (1, 1500)), 8: (12, (1, 3000))}


def log2(x):
    return x.bit_length() - 1


_squares = {}


def square_of(k):
    """One square per k, computed once and never changed: constructed (namespaced blobs) up to k = 8, random
    above (every share its own namespace)."""
    if k not in _squares:
        if k in SMALL:
            ods, ss, _ = constructed_square(100 + k, k, *SMALL[k])
            assert ss == k
        else:   # k = 512: square 0, the one tests/golden/k512.json records
            ods = coracle.random_square(k, 7 if k <= 128 else 0)
        _squares[k] = np.ascontiguousarray(ods).reshape(k * k, 512)
    return _squares[k]


@pytest.fixture(scope="module")
def resident(ctx):
    """ResidentSquare of square_of(k), one per k for the whole module."""
    from celestia_da import proof as gpr
    made = {}

    def get(k):
        if k not in made:
            made[k] = gpr.ResidentSquare(square_of(k), ctx)
        return made[k]
    yield get
    for sq in made.values():
        sq.close()


class OracleSquare:
    """What the oracle says about one square, cached per row: the leaf nodes, the proof nodes of a leaf range
    and the merkle proof of the row root."""

    def __init__(self, k, eds, rows, cols, blind=False):
        W = 2 * k
        self.k, self.blind = k, blind
        self.eds = np.asarray(eds).reshape(W, W, 512)
        self.rows = [bytes(r) for r in rows]
        self.roots = self.rows + [bytes(c) for c in cols]
        self._leaves, self._nodes, self._merkle = {}, {}, {}

    def leaves(self, row):
        if row not in self._leaves:
            self._leaves[row] = pyref.erasured_leaves([x.tobytes() for x in self.eds[row]], self.k, row, self.blind)
        return self._leaves[row]

    def nodes(self, row, s0, e0):
        if (row, s0, e0) not in self._nodes:
            got = opr.nmt_range_proof(self.leaves(row), s0, e0)
            self._nodes[row, s0, e0] = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(len(got), 90)
        return self._nodes[row, s0, e0]

    def merkle(self, row):
        if row not in self._merkle:
            leaf, aunts = opr.rfc_aunts(self.roots, row)
            self._merkle[row] = (np.frombuffer(leaf, dtype=np.uint8),
                                 np.frombuffer(b"".join(aunts), dtype=np.uint8).reshape(len(aunts), 32))
        return self._merkle[row]

    def range(self, s, e):
        """NewShareInclusionProofFromEDS of [s, e): the pieces of the batch arrays that belong to this range."""
        k = self.k
        r0, r1 = s // k, (e - 1) // k
        R, A = r1 - r0 + 1, log2(4 * k)
        seg = [(r, s % k if r == r0 else 0, (e - 1) % k + 1 if r == r1 else k) for r in range(r0, r1 + 1)]
        nodes = [self.nodes(*g) for g in seg]
        shares = np.concatenate([self.eds[r, s0:e0] for r, s0, e0 in seg])
        assert shares.shape == (e - s, 512) and all(self.merkle(r)[1].shape == (A, 32) for r, _, _ in seg)
        return {"nmt_start": [g[1] for g in seg], "nmt_end": [g[2] for g in seg], "counts": [len(x) for x in nodes],
                "nodes": np.concatenate(nodes),
                "row_roots": np.frombuffer(b"".join(self.rows[r0:r1 + 1]), dtype=np.uint8).reshape(R, 90),
                "rfc_total": [4 * k] * R, "rfc_index": list(range(r0, r1 + 1)),
                "rfc_leaf_hash": np.stack([self.merkle(r)[0] for r, _, _ in seg]),
                "aunts": np.concatenate([self.merkle(r)[1] for r, _, _ in seg]), "aunt_counts": [A] * R,
                "shares": shares, "namespace": shares[0, :29], "start_row": r0, "end_row": r1,
                "one_namespace": int((shares[:, :29] == shares[0, :29]).all())}


_oracles = {}


def oracle_range(sq, s, e):
    """The oracle's pieces for [s, e) of square_of(sq.k).  The EDS and the roots are the C oracle's up to
    k = 128.  At k = 512, beyond what it is used for, they are the resident square's own, checked first: their
    digests and the data root are the ones tests/golden/k512.json records for this square, and the data root is
    the RFC-6962 root of the row and column roots."""
    k = sq.k
    if k not in _oracles:
        if k <= 128:
            eds, rows, cols, _ = oracle_eds(square_of(k), k)
        else:
            want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "k512.json")))["squares"]["0"]
            eds = sq.eds()
            rows, cols, root = sq.dah()
            sha = lambda parts: hashlib.sha256(b"".join(bytes(x) for x in parts)).hexdigest()   # noqa: E731
            assert hashlib.sha256(np.ascontiguousarray(eds).tobytes()).hexdigest() == want["eds_sha256"]
            assert sha(rows) == want["row_roots_sha256"] and sha(cols) == want["col_roots_sha256"]
            assert pyref.merkle_root([bytes(x) for x in rows] + [bytes(x) for x in cols]) == bytes(root)
            assert bytes(root).hex() == want["data_root"]
        _oracles[k] = OracleSquare(k, eds, rows, cols)
    return _oracles[k].range(s, e)


def test_oracle_ranges_verify_against_the_oracle_root():
    """The yardstick itself, no GPU: every segment of every range of the k = 4 square verifies against the
    oracle's row root, and that root against the oracle's data root."""
    k = 4
    ods = square_of(k)
    eds, rows, cols, root = oracle_eds(ods, k)
    oracle = OracleSquare(k, eds, rows, cols)
    for s, e in all_ranges(k):
        p = oracle.range(s, e)
        assert np.array_equal(p["shares"], ods[s:e]) and sum(p["counts"]) == len(p["nodes"])
        at = 0
        for i, (s0, e0, n) in enumerate(zip(p["nmt_start"], p["nmt_end"], p["counts"])):
            row = p["rfc_index"][i]
            nodes = [x.tobytes() for x in p["nodes"][at:at + n]]
            at += n
            assert opr.nmt_verify_range(rows[row], nodes, s0, e0, 2 * k, oracle.leaves(row)[s0:e0]), (s, e, i)
            assert opr.rfc_verify(root, 4 * k, row, p["rfc_leaf_hash"][i].tobytes(),
                                  [x.tobytes() for x in p["aunts"][i * log2(4 * k):(i + 1) * log2(4 * k)]]), (s, e, i)


def assemble(pieces):
    """The sixteen arrays of cda_share_proofs_out from the single-range pieces, in ShareProofsBatch.FIELDS order."""
    def offsets(counts):
        return np.cumsum([0] + counts, dtype=np.int64).astype(np.uint32)

    def cat(name, width):
        return np.concatenate([p[name].reshape(-1, width) for p in pieces] or [np.empty((0, width), dtype=np.uint8)])

    flat = lambda name: [x for p in pieces for x in p[name]]   # noqa: E731
    return (offsets([len(p["nmt_start"]) for p in pieces]), np.array(flat("nmt_start"), dtype=np.int32),
            np.array(flat("nmt_end"), dtype=np.int32), offsets(flat("counts")), cat("nodes", 90), cat("row_roots", 90),
            np.array(flat("rfc_total"), dtype=np.int64), np.array(flat("rfc_index"), dtype=np.int64),
            cat("rfc_leaf_hash", 32), offsets(flat("aunt_counts")), cat("aunts", 32), cat("shares", 512),
            cat("namespace", 29), np.array([p["start_row"] for p in pieces], dtype=np.uint32),
            np.array([p["end_row"] for p in pieces], dtype=np.uint32),
            np.array([p["one_namespace"] for p in pieces], dtype=np.uint8))


def assert_batch_equals(batch, pieces):
    from celestia_da.proof import ShareProofsBatch
    for name, got, exp in zip(ShareProofsBatch.FIELDS, batch.arrays(), assemble(pieces)):
        assert got.dtype == exp.dtype and got.shape == exp.shape, (name, got.shape, exp.shape)
        if not np.array_equal(got, exp):
            bad = np.nonzero((got != exp).reshape(got.shape[0], -1).any(axis=1))[0]
            raise AssertionError((name, "first differing entry", int(bad[0]), "of", got.shape[0]))


def all_ranges(k):
    return [(s, e) for s in range(k * k) for e in range(s + 1, k * k + 1)]


# ------------------------------------------------- 1. exhaustive small squares
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_every_range_of_small_squares(resident, k):
    """Every range [s, e) of the ODS in one call (1, 10, 136, 2 080 ranges; 45 760 shares at k = 8) against the
    oracle's proof of each."""
    sq = resident(k)
    ranges = all_ranges(k)
    assert len(ranges) == k * k * (k * k + 1) // 2
    batch = sq.share_proofs_batch(ranges)
    assert len(batch) == len(ranges) and batch.shares.shape[0] == sum(e - s for s, e in ranges)
    assert_batch_equals(batch, [oracle_range(sq, s, e) for s, e in ranges])


@pytest.mark.gpu
def test_every_range_k4_against_the_oracle(resident):
    """k = 4: the ShareProof objects of the batch equal share_proof's field for field, and every proof that
    ShareProof.Validate applies to (one namespace in the range; the others carry one_namespace = 0) passes the
    oracle's share_proof_validate against the oracle's data root."""
    k = 4
    sq, ods = resident(k), square_of(k)
    _, _, _, root = oracle_eds(ods, k)
    ranges = all_ranges(k)
    batch = sq.share_proofs_batch(ranges)
    firsts = [bytes(ods[s, :29]) for s, _ in ranges]
    proofs = batch.proofs(firsts)
    n_valid = 0
    for (s, e), ns, p, one in zip(ranges, firsts, proofs, batch.one_namespace.tolist()):
        assert p == sq.share_proof(ns, s, e), (s, e)
        assert one == (len({bytes(x[:29]) for x in ods[s:e]}) == 1), (s, e)
        if one:
            assert opr.share_proof_validate(to_dict(p), root) is None, (s, e)
            n_valid += 1
    assert 16 <= n_valid < len(ranges)


# ------------------------------------------------------ 2. edges at larger k
def edge_ranges(k, n=301):
    """The whole square first, then the edges, then seeded ranges of at most three rows, n in all."""
    kk = k * k
    r = [(0, kk), (0, 1), (k - 1, k), (kk - k, kk - k + 1), (kk - 1, kk)]           # the four ODS corners
    r += [(row * k, row * k + k) for row in (0, 1, k // 2, k - 1)]                   # full rows
    r += [(row * k - 1, row * k + 1) for row in (1, 2, k // 2, k - 1)]               # [row end - 1, next row start + 1)
    r += [(k - 3, k + 2), (5, 2 * k + 1), (2 * k - 1, 4 * k), (kk - 2 * k - 1, kk)]  # crossing 2 and 3 rows
    r += [(0, 1), (k - 3, k + 2), (k - 2, k + 3), (k - 3, k + 2), (0, 2 * k), (k, 3 * k)]   # duplicates, overlaps
    rng = np.random.default_rng(k)
    while len(r) < n:
        s = int(rng.integers(0, kk))
        r.append((s, min(kk, s + 1 + int(rng.integers(0, 3 * k)))))
    return r


_edge_pieces = {}


def edge_pieces(sq, k):
    if k not in _edge_pieces:
        _edge_pieces[k] = [oracle_range(sq, s, e) for s, e in edge_ranges(k)]
    return _edge_pieces[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", [(32, 1), (32, 5), (32, 301), (128, 1), (128, 5), (128, 301)])
def test_edges(resident, k, n):
    """The first n of edge_ranges(k) in one call: batch sizes that are no multiple of the workgroup's four
    segments, the whole square alone, and every edge beside 280 seeded ranges."""
    sq = resident(k)
    ranges = edge_ranges(k)
    assert len(ranges) == 301 and ranges[0] == (0, k * k)
    assert_batch_equals(sq.share_proofs_batch(ranges[:n]), edge_pieces(sq, k)[:n])


@pytest.mark.gpu
def test_k512(resident):
    k = 512
    sq = resident(k)
    ranges = [(0, 1), (k - 1, k + 1), (3 * k + 100, 5 * k + 7), (k * k - 1, k * k), (k * k // 2, k * k // 2 + k),
              (k * k - 2 * k - 5, k * k)]
    batch = sq.share_proofs_batch(ranges)
    assert_batch_equals(batch, [oracle_range(sq, s, e) for s, e in ranges])
    assert batch.one_namespace.tolist() == [1, 0, 0, 1, 0, 0]   # a random square: every share its own namespace


def push_order_square():
    """A k = 2 square whose Q0 is not namespace ordered, and the oracle's view of it: the oracle's extension, the
    BlindTree roots (no order check; the hashing never depended on the order)."""
    k = 2
    ods = square_of(4)[[5, 1, 9, 13]].copy()
    assert bytes(ods[0, :29]) > bytes(ods[1, :29])
    eds = coracle.extend(ods).reshape(2 * k, 2 * k, 512)
    rows, cols, _ = pyref.dah_from_eds(eds, blind=True)
    return ods, OracleSquare(k, eds, rows, cols, blind=True)


@pytest.mark.gpu
def test_push_order_square_serves_proofs(ctx):
    """A square whose Q0 is not namespace ordered is still created and serves the oracle's bytes, through the
    batch call and through the single-range call."""
    from celestia_da import proof as gpr
    ods, oracle = push_order_square()
    sq = gpr.ResidentSquare(ods, ctx)
    try:
        assert sq.push_order_error
        ranges = all_ranges(sq.k)
        pieces = [oracle.range(s, e) for s, e in ranges]
        assert_batch_equals(sq.share_proofs_batch(ranges), pieces)
        for (s, e), want in zip(ranges, pieces):
            assert_single_equals(single_call(sq, s, e), want, (s, e))
    finally:
        sq.close()


# ------------------------------------- 2b. the single-range front end (cda_square_share_proof)
SINGLE_OPTIONAL = ("shares", "nmt_nodes", "row_roots", "row_leaf_hash", "row_aunts")
SINGLE_REQUIRED = ("start_row", "end_row", "nmt_start", "nmt_end", "nmt_count")


def single_call(sq, s, e, null=(), rows=None):
    """cda_square_share_proof of [s, e) into buffers pre-filled with 0xAA, sized for the range (or for `rows`
    rows and max(e - s, 1) shares when the range is not valid); the buffers named in `null` are passed as NULL.
    Returns the buffers (those too) with the return code under "rc"."""
    k = sq.k
    R = rows or (e - 1) // k - s // k + 1
    M, A = 2 * log2(2 * k), log2(4 * k)
    shapes = {"shares": (max(e - s, 1), 512), "nmt_nodes": (R, M, 90), "row_roots": (R, 90),
              "row_leaf_hash": (R, 32), "row_aunts": (R * A, 32)}
    b = {name: np.full(shape, 0xAA, dtype=np.uint8) for name, shape in shapes.items()}
    b.update({"start_row": np.full(1, 0xAAAAAAAA, dtype=np.uint32), "end_row": np.full(1, 0xAAAAAAAA, dtype=np.uint32),
              "nmt_start": np.full(R, -0x55555556, dtype=np.int32), "nmt_end": np.full(R, -0x55555556, dtype=np.int32),
              "nmt_count": np.full(R, 0xAAAAAAAA, dtype=np.uint32)})
    order = ("shares", "start_row", "end_row", "nmt_start", "nmt_end", "nmt_count", "nmt_nodes", "row_roots",
             "row_leaf_hash", "row_aunts")
    ctype = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint32): C.c_uint32, np.dtype(np.int32): C.c_int32}
    args = [None if name in null else b[name].ctypes.data_as(C.POINTER(ctype[b[name].dtype])) for name in order]
    b["rc"] = sq.ctx.lib.cda_square_share_proof(sq.h, s, e, *args)
    return b


def untouched(a):
    return bool((a.view(np.uint8) == 0xAA).all())


def assert_single_equals(got, want, what, skip=()):
    """Every buffer of a single call against the oracle's pieces: the first nmt_count[i] node slots of row i at
    stride M (the slots behind them are unspecified), everything else whole.  Buffers in `skip` were passed as
    NULL and must be as they were."""
    assert got["rc"] == _lib.CDA_OK, what
    R = len(want["nmt_start"])
    assert (int(got["start_row"][0]), int(got["end_row"][0])) == (want["start_row"], want["end_row"]), what
    assert got["nmt_start"].tolist() == want["nmt_start"] and got["nmt_end"].tolist() == want["nmt_end"], what
    assert got["nmt_count"].tolist() == want["counts"] and got["nmt_nodes"].shape[0] == R, what
    for name, exp in (("shares", want["shares"]), ("row_roots", want["row_roots"]),
                      ("row_leaf_hash", want["rfc_leaf_hash"]), ("row_aunts", want["aunts"])):
        if name in skip:
            assert untouched(got[name]), (what, name)
        else:
            assert got[name].shape == exp.shape and np.array_equal(got[name], exp), (what, name)
    if "nmt_nodes" in skip:
        assert untouched(got["nmt_nodes"]), what
    else:
        at = 0
        for i, n in enumerate(want["counts"]):
            assert np.array_equal(got["nmt_nodes"][i, :n], want["nodes"][at:at + n]), (what, "nodes of row", i)
            at += n


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 4])
def test_single_call_every_range(resident, k):
    """Every range of the k = 1 (the two-leaf tree), 2 (a range of two rows with nothing between them) and 4 (a
    whole row between two partial ones) squares, one cda_square_share_proof call each: 1, 10 and 136 calls."""
    sq = resident(k)
    ranges = all_ranges(k)
    assert len(ranges) == {1: 1, 2: 10, 4: 136}[k]
    for s, e in ranges:
        assert_single_equals(single_call(sq, s, e), oracle_range(sq, s, e), (s, e))


@pytest.mark.gpu
def test_single_call_edges_k32(resident):
    """The first 25 of edge_ranges(32): the whole square (32 segments from one call), the corners, full rows and
    ranges that cross rows."""
    k = 32
    sq = resident(k)
    ranges = edge_ranges(k)[:25]
    assert ranges[0] == (0, k * k) and (k - 3, k + 2) in ranges and (k, 3 * k) in ranges
    for (s, e), want in zip(ranges, edge_pieces(sq, k)):
        assert_single_equals(single_call(sq, s, e), want, (s, e))


@pytest.mark.gpu
def test_single_call_null_outputs(resident):
    """Each of the five optional buffers NULL in turn: the others as in the full call, the skipped one untouched."""
    k, s, e = 8, 6, 19
    sq = resident(k)
    want = oracle_range(sq, s, e)
    full = single_call(sq, s, e)
    assert_single_equals(full, want, "full")
    for name in SINGLE_OPTIONAL:
        got = single_call(sq, s, e, null=(name,))
        assert_single_equals(got, want, name, skip=(name,))
        for other in SINGLE_OPTIONAL:
            if other not in (name, "nmt_nodes"):
                assert np.array_equal(got[other], full[other]), (name, other)
    got = single_call(sq, s, e, null=SINGLE_OPTIONAL)   # nothing from the device at all
    assert_single_equals(got, want, "all", skip=SINGLE_OPTIONAL)


@pytest.mark.gpu
def test_single_call_errors(ctx, resident):
    k = 8
    sq = resident(k)
    for s, e in ((5, 5), (9, 3), (60, k * k + 1)):
        got = single_call(sq, s, e, rows=2)
        assert got["rc"] == _lib.CDA_ERR_INVALID, (s, e)
        assert ctx.lib.cda_last_error(ctx.h).decode() == "share range out of the original square", (s, e)
        for name in SINGLE_OPTIONAL + ("nmt_start", "nmt_end", "nmt_count"):
            assert untouched(got[name]), (s, e, name)
    for name in SINGLE_REQUIRED:
        got = single_call(sq, 6, 19, null=(name,))
        assert got["rc"] == _lib.CDA_ERR_INVALID, name
        assert ctx.lib.cda_last_error(ctx.h).decode() == "null buffer", name
        for other in SINGLE_OPTIONAL + SINGLE_REQUIRED:
            assert untouched(got[other]), (name, other)


# ------------------------------------------------------------ 3. round trip
def one_namespace_ranges(ods, k):
    """Every maximal run of one namespace, its first share alone and its first half."""
    ns = [bytes(x[:29]) for x in ods]
    out, s = [], 0
    for i in range(1, len(ns) + 1):
        if i == len(ns) or ns[i] != ns[s]:
            out += [(s, i), (s, s + 1), (s, s + max(1, (i - s) // 2))]
            s = i
    return out


@pytest.mark.gpu
def test_round_trip_through_verify(ctx, resident):
    """The arrays go into cda_share_proofs_verify through .batch(root) unchanged: all valid; one flipped node
    byte gives that proof alone verdict 2, one flipped aunt byte that proof alone verdict 1."""
    k = 8
    sq, ods = resident(k), square_of(k)
    root = sq.dah()[2]
    ranges = one_namespace_ranges(ods, k)
    assert len(ranges) >= 12 and any((e - 1) // k > s // k for s, e in ranges)
    batch = sq.share_proofs_batch(ranges)
    assert batch.one_namespace.all()
    b = batch.batch(root)
    assert (b.n_proofs, b.ns_len, b.share_len) == (len(ranges), 29, 512)
    assert C.addressof(b.nodes.contents) == batch.nodes.ctypes.data      # pointer assignment, no copies
    assert C.addressof(b.shares.contents) == batch.shares.ctypes.data
    verdict = np.full(len(ranges), 255, dtype=np.uint8)
    ctx.check(ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
    assert not verdict.any()
    assert not batch.verify(root, ctx).any()
    # proof 4's first node, the digest part
    g = int(batch.seg_off[4])
    batch.nodes[int(batch.node_off[g]), 70] ^= 1
    assert batch.verify(root, ctx).tolist() == [2 if i == 4 else 0 for i in range(len(ranges))]
    batch.nodes[int(batch.node_off[g]), 70] ^= 1
    # the last aunt of proof 7's last segment
    g = int(batch.seg_off[8]) - 1
    batch.aunts[int(batch.aunt_off[g + 1]) - 1, 5] ^= 1
    assert batch.verify(root, ctx).tolist() == [1 if i == 7 else 0 for i in range(len(ranges))]
    batch.aunts[int(batch.aunt_off[g + 1]) - 1, 5] ^= 1
    assert not batch.verify(root, ctx).any()


# ------------------------------------------------------------ 4. one_namespace
@pytest.mark.gpu
def test_one_namespace_flag_and_parse_error(resident):
    from celestia_da import proof as gpr
    k = 8
    sq, ods = resident(k), square_of(k)
    shares = [bytes(x) for x in ods]
    ns = [s[:29] for s in shares]
    inside = one_namespace_ranges(ods, k)
    bounds = [i for i in range(1, k * k) if ns[i] != ns[i - 1]]
    assert len(bounds) >= 3
    # across a boundary: two shares, a long range that differs only in its last share, one that differs from its
    # second share on, the whole square
    across = [(b - 1, b + 1) for b in bounds] + [(0, bounds[0] + 1), (bounds[0] - 1, k * k), (0, k * k)]
    batch = sq.share_proofs_batch(inside + across)
    assert batch.one_namespace.tolist() == [1] * len(inside) + [0] * len(across)
    assert [x.tobytes() for x in batch.namespaces] == [ns[s] for s, _ in inside + across]
    got = sq.share_proofs_batch(inside).proofs()
    assert got == [sq.share_proof(ns[s], s, e) for s, e in inside]
    for s, e in across:
        with pytest.raises(ValueError) as want:
            gpr.parse_namespace(shares, s, e)
        with pytest.raises(ValueError) as err:
            sq.share_proofs_batch([inside[0], (s, e)]).proofs()
        assert str(err.value) == str(want.value)
        assert "different namespaces" in str(err.value)


# ------------------------------------------------------ 5. NULL outputs, errors
@pytest.mark.gpu
def test_null_outputs_empty_batch_and_invalid_ranges(ctx, resident):
    from celestia_da.proof import ShareProofsBatch
    k = 8
    sq = resident(k)
    ranges = [(0, 1), (6, 19), (0, 64), (63, 64), (8, 16), (21, 22), (6, 19)]
    full = sq.share_proofs_batch(ranges)
    r = np.array(ranges, dtype=np.uint32)
    starts, ends = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    u32p = C.POINTER(C.c_uint32)
    call = lambda o, n=len(ranges): ctx.lib.cda_square_share_proofs(   # noqa: E731
        sq.h, starts.ctypes.data_as(u32p), ends.ctypes.data_as(u32p), n, C.byref(o))
    for skip in ShareProofsBatch.FIELDS:
        out = ShareProofsBatch.empty(k, ranges, fill=0xAA)
        assert call(out.out_struct(skip=(skip,))) == _lib.CDA_OK, skip
        for name, got, exp in zip(ShareProofsBatch.FIELDS, out.arrays(), full.arrays()):
            if name == skip:
                assert (got.view(np.uint8) == 0xAA).all(), (skip, name)
            else:
                assert np.array_equal(got, exp), (skip, name)
    # only the flags: no share leaves the device
    out = ShareProofsBatch.empty(k, ranges, fill=0xAA)
    assert call(out.out_struct(skip=tuple(f for f in ShareProofsBatch.FIELDS if f != "one_namespace"))) == _lib.CDA_OK
    assert np.array_equal(out.one_namespace, full.one_namespace) and (out.shares == 0xAA).all()
    # n == 0
    assert len(sq.share_proofs_batch([])) == 0
    assert call(_lib.ShareProofsOut(), 0) == _lib.CDA_OK
    assert ctx.lib.cda_square_share_proofs(sq.h, None, None, 0, C.byref(_lib.ShareProofsOut())) == _lib.CDA_OK
    # invalid ranges: nothing is written
    for bad, text in (((5, 5), "range 3: start 5 is not below end 5"),
                      ((9, 3), "range 3: start 9 is not below end 3"),
                      ((60, 65), "range 3: end 65 is beyond the 64 shares of the original square")):
        bad_ranges = ranges[:3] + [bad] + ranges[3:]
        out = ShareProofsBatch.empty(k, ranges + [(0, 1)], fill=0xAA)
        with pytest.raises(CdaError) as e:
            sq.share_proofs_batch(bad_ranges, out=out)
        assert e.value.code == _lib.CDA_ERR_INVALID and str(e.value) == text
        for a in out.arrays():
            assert (a.view(np.uint8) == 0xAA).all()
    assert ctx.lib.cda_square_share_proofs(sq.h, starts.ctypes.data_as(u32p), ends.ctypes.data_as(u32p),
                                           len(ranges), None) == _lib.CDA_ERR_INVALID


# ------------------------------------------------------------ 6. transactions
def _tx_blocks():
    from test_tx_proofs import _blocks, _reference_shape_block
    b = _blocks()
    return {"reference_shape": (_reference_shape_block(), [0, 49, 50, 99]),
            "share_boundaries": (b["share_boundaries"], None),
            "repeated": (b["repeated"], [4, 0, 1, 1, 3])}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["reference_shape", "share_boundaries", "repeated"])
def test_tx_inclusion_proofs_equal_the_single_call(ctx, name):
    from celestia_da import proof as gpr
    txs, indexes = _tx_blocks()[name]
    got = gpr.new_tx_inclusion_proofs(txs, indexes)
    assert got == [gpr.new_tx_inclusion_proof(txs, i) for i in (range(len(txs)) if indexes is None else indexes)]


@pytest.mark.gpu
def test_tx_inclusion_proofs_block408(ctx):
    """Every transaction of mainnet block 408 from one batch call: equal to the per-index call, and valid against
    the fixture's data root."""
    from celestia_da import proof as gpr
    from test_square import block408
    txs, _, data_hash = block408()
    got = gpr.new_tx_inclusion_proofs(txs)
    assert len(got) == len(txs) == 274
    for i, p in enumerate(got):
        assert opr.share_proof_validate(to_dict(p), data_hash) is None, i
        assert p == gpr.new_tx_inclusion_proof(txs, i), i
