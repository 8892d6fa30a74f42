"""Share proofs of many ranges of a resident square in one launch:
cda_square_share_proofs (csrc/share_proofs.hip) and its Python surface
(ResidentSquare.share_proofs_batch, new_share_inclusion_proofs,
new_tx_inclusion_proofs).

The yardstick is the single-range call, cda_square_share_proof, which the
reference's own vectors pin (test_proofs.py, test_tx_proofs.py): every array
of a batch equals, byte for byte, what a loop of that call returns for the
same ranges, cut by the batch's offsets.  No tolerances.
"""
import ctypes as C

import numpy as np
import pytest

import coracle
import proofs as opr
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
        else:
            ods = coracle.random_square(k, 7)
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


def single_range(sq, s, e):
    """cda_square_share_proof of [s, e): the pieces of the batch arrays that belong to this range."""
    k = sq.k
    W = 2 * k
    R = (e - 1) // k - s // k + 1
    M, A = 2 * log2(W), log2(2 * W)
    shares = np.empty((e - s, 512), dtype=np.uint8)
    ns, ne, cnt = (C.c_int32 * R)(), (C.c_int32 * R)(), (C.c_uint32 * R)()
    nodes = np.empty((R, M, 90), dtype=np.uint8)
    roots, leaf, aunts = (np.empty(shape, dtype=np.uint8) for shape in ((R, 90), (R, 32), (R * A, 32)))
    r0, r1 = C.c_uint32(), C.c_uint32()
    sq.ctx.check(sq.ctx.lib.cda_square_share_proof(sq.h, s, e, ptr(shares), C.byref(r0), C.byref(r1), ns, ne, cnt,
                                                   ptr(nodes), ptr(roots), ptr(leaf), ptr(aunts)))
    return {"nmt_start": list(ns), "nmt_end": list(ne), "counts": list(cnt),
            "nodes": np.concatenate([nodes[i, :cnt[i]] for i in range(R)]), "row_roots": roots,
            "rfc_total": [4 * k] * R, "rfc_index": list(range(r0.value, r0.value + R)), "rfc_leaf_hash": leaf,
            "aunts": aunts, "aunt_counts": [A] * R, "shares": shares, "namespace": shares[0, :29],
            "start_row": r0.value, "end_row": r1.value,
            "one_namespace": int((shares[:, :29] == shares[0, :29]).all())}


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
    loop of single-range calls."""
    sq = resident(k)
    ranges = all_ranges(k)
    assert len(ranges) == k * k * (k * k + 1) // 2
    batch = sq.share_proofs_batch(ranges)
    assert len(batch) == len(ranges) and batch.shares.shape[0] == sum(e - s for s, e in ranges)
    assert_batch_equals(batch, [single_range(sq, s, e) for s, e in ranges])


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
        _edge_pieces[k] = [single_range(sq, s, e) for s, e in edge_ranges(k)]
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
    assert_batch_equals(batch, [single_range(sq, s, e) for s, e in ranges])
    assert batch.one_namespace.tolist() == [1, 0, 0, 1, 0, 0]   # a random square: every share its own namespace


@pytest.mark.gpu
def test_push_order_square_serves_proofs(ctx):
    """A square whose Q0 is not namespace ordered is still created and serves the same bytes as the single call."""
    from celestia_da import proof as gpr
    k = 2
    ods = square_of(4)[[5, 1, 9, 13]].copy()
    assert bytes(ods[0, :29]) > bytes(ods[1, :29])
    sq = gpr.ResidentSquare(ods, ctx)
    try:
        assert sq.push_order_error
        ranges = all_ranges(k)
        assert_batch_equals(sq.share_proofs_batch(ranges), [single_range(sq, s, e) for s, e in ranges])
    finally:
        sq.close()


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
