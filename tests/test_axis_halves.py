"""Axis halves: cda_square_axis_halves / cda_square_set_axis_halves (serving
half rows and half columns of resident squares), cda_axis_halves_verify
(Row.Verify for a batch of left and right halves) and cda_rs_recover_data (the
data shards from the parity shards alone, on the encoder's kernels).

The checker is the oracle: the C oracle's EDS and DAH (coracle.extend_dah) and
encoder (coracle.leopard_encode), pyref.axis_root, and for the recovery
transform and the verdict rule their numpy restatement tests/axis_halves_ref.py,
which the CPU tests below pin to pyref.leopard_encode and
repair.leopard_reconstruct.  Everything is compared byte for byte.
"""
import ctypes as C

import numpy as np
import pytest

import axis_halves_ref as ref
import coracle
import pyref
import repair as orepair
from celestia_da import CdaError, _lib

POW2 = [1 << i for i in range(11)]   # 1 .. 1024
U32P = C.POINTER(C.c_uint32)


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


# ---------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("k", [2, 4, 8, 16, 32, 64, 128, 256])
def test_ref_recovery_equals_reconstruct(k):
    """The swapped-offset transform equals the oracle's decoder with the data half erased."""
    data = _rand((k, 64), 7000 + k)
    parity = pyref.leopard_encode(data)
    shards = np.concatenate([np.zeros_like(parity), parity])
    present = np.array([0] * k + [1] * k, dtype=bool)
    want = orepair.leopard_reconstruct(shards, present)
    assert np.array_equal(want[:k], data) and np.array_equal(want[k:], parity)
    assert np.array_equal(ref.recover_data(parity), want[:k])


@pytest.mark.parametrize("k", POW2)
def test_ref_recovery_round_trips_the_encoder(k):
    data = _rand((k, 64), 7100 + k)
    assert np.array_equal(ref.recover_data(pyref.leopard_encode(data)), data)


def test_ref_verdict_rule():
    k = 4
    ods = coracle.random_square(k, 31).reshape(k, k, 512)
    eds = pyref.extend_square(ods)
    rows, cols, _ = pyref.dah_from_eds(eds)
    for axis, index, side in [(0, 1, 0), (0, 1, 1), (1, 2, 1), (0, 6, 0), (1, 7, 1)]:
        root = (rows if axis == 0 else cols)[index]
        half = ref.half_of(eds, axis, index, side)
        v, vec = ref.verdict(half, side, index, root)
        assert v == 0 and np.array_equal(vec, eds[index] if axis == 0 else eds[:, index])
        bad = half.copy()
        bad[1, 300] ^= 1
        assert ref.verdict(bad, side, index, root)[0] == 1
    swapped = ref.half_of(eds, 0, 1, 0)[[0, 3, 2, 1]]
    assert bytes(swapped[1, :29]) > bytes(swapped[3, :29])
    assert ref.verdict(swapped, 0, 1, rows[1])[0] == 2


# ---------------------------------------------------------------- shared squares
class Square:
    """One oracle square per (k, seed), computed once and never changed."""

    def __init__(self, k, seed=0):
        self.k, self.W = k, 2 * k
        self.ods = coracle.random_square(k, seed)
        eds, rows, cols, root = coracle.extend_dah(self.ods)
        self.eds = eds.reshape(self.W, self.W, 512)
        self.rows, self.cols = np.ascontiguousarray(rows), np.ascontiguousarray(cols)

    def half(self, axis, index, side):
        return ref.half_of(self.eds, axis, index, side)

    def halves(self, coords):
        return np.stack([self.half(a, i, s) for a, i, s in np.asarray(coords).reshape(-1, 3).tolist()]) \
            if len(coords) else np.zeros((0, self.k, 512), dtype=np.uint8)

    def vector(self, axis, index):
        return self.eds[index] if axis == 0 else self.eds[:, index]

    def vectors(self, coords):
        return np.stack([self.vector(a, i) for a, i, _ in np.asarray(coords).reshape(-1, 3).tolist()])


_squares = {}


def square(k, seed=0):
    if (k, seed) not in _squares:
        _squares[k, seed] = Square(k, seed)
    return _squares[k, seed]


@pytest.fixture(scope="module")
def resident(ctx):
    from celestia_da import proof as gpr
    made = {}

    def get(k, seed=0):
        if (k, seed) not in made:
            made[k, seed] = gpr.ResidentSquare(square(k, seed).ods, ctx)
        return made[k, seed]
    yield get
    for sq in made.values():
        sq.close()


def all_halves(k):
    return np.array([(a, i, s) for a in (0, 1) for i in range(2 * k) for s in (0, 1)], dtype=np.int64)


def batch_of(sq, coords, square_col=0):
    """A HalfBatch of the oracle square's own halves (what an honest server sends)."""
    from celestia_da import axis_halves as ah
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    c4 = np.concatenate([np.full((len(c), 1), square_col, dtype=np.int64), c], axis=1)
    return ah.HalfBatch(sq.k, c4, sq.halves(c))


# ---------------------------------------------------------------- GPU: cda_rs_recover_data
@pytest.mark.gpu
@pytest.mark.parametrize("k", POW2)
def test_rs_recover_data(ctx, k):
    """The oracle encodes three codewords, the GPU recovers the data from the parity alone."""
    from celestia_da import axis_halves as ah
    for L in (64, 512):
        data = _rand((3, k, L), 7200 + k + L)
        parity = np.stack([coracle.leopard_encode(d) for d in data])
        assert np.array_equal(ah.recover_data(parity, ctx), data), (k, L)


@pytest.mark.gpu
def test_rs_recover_data_rejections(ctx):
    from celestia_da._lib import ptr

    def call(k, L):
        parity = _rand((2, k, L), 1)
        out = np.full_like(parity, 0xA5)
        rc = ctx.lib.cda_rs_recover_data(ctx.h, ptr(parity), k, L, 2, ptr(out))
        assert (out == 0xA5).all(), "nothing written"
        return rc, ctx.lib.cda_last_error(ctx.h).decode()

    assert call(3, 64) == (_lib.CDA_ERR_UNSUPPORTED, "shard count must be a power of two <= 1024")
    assert call(2048, 64) == (_lib.CDA_ERR_UNSUPPORTED, "shard count must be a power of two <= 1024")
    assert call(8, 96) == (_lib.CDA_ERR_CHUNK_SIZE, "chunkSize 96 must be a multiple of 64 bytes")
    assert ctx.lib.cda_rs_recover_data(ctx.h, None, 8, 64, 0, None) == _lib.CDA_OK


# ---------------------------------------------------------------- GPU: serving
def serve_coords(k):
    """Both axes, both sides, indexes on both sides of k, a duplicate."""
    W = 2 * k
    idx = sorted({0, k - 1, k, W - 1, k // 2, k + k // 2})
    c = [(a, i, s) for a in (0, 1) for i in idx for s in (0, 1)]
    return np.array(c + [c[3], c[3]], dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 8, 128])
def test_serve(resident, k):
    sq, rs = square(k), resident(k)
    coords = serve_coords(k)
    got = rs.axis_halves(coords)
    assert got.k == k and got.shares.shape == (len(coords), k, 512)
    assert np.array_equal(got.shares, sq.halves(coords))
    assert np.array_equal(got.coords[:, 1:], coords) and not got.coords[:, 0].any()
    assert len(rs.axis_halves(np.zeros((0, 3), dtype=np.int64))) == 0
    assert rs.ctx.lib.cda_square_axis_halves(rs.h, None, None, None, 0, None) == _lib.CDA_OK


@pytest.mark.gpu
def test_serve_every_half(resident):
    k = 8
    coords = all_halves(k)
    assert np.array_equal(resident(k).axis_halves(coords).shares, square(k).halves(coords))


@pytest.fixture(scope="module")
def small_set(ctx):
    from celestia_da import proof as gpr
    k, n = 8, 3
    sqs = [square(k, 40 + i) for i in range(n)]
    sqset = gpr.ResidentSquareSet.from_ods(np.stack([s.ods for s in sqs]).reshape(n, k * k, 512), ctx=ctx)
    yield sqset, sqs
    sqset.close()


def set_coords(k, n):
    c = serve_coords(k)
    return np.array([((3 * j + 1) % n, *c[j]) for j in range(len(c))], dtype=np.int64)


@pytest.mark.gpu
def test_serve_set(small_set):
    sqset, sqs = small_set
    k, n = sqset.k, len(sqs)
    coords = set_coords(k, n)
    got = sqset.axis_halves(coords)
    for j, (y, a, i, s) in enumerate(coords.tolist()):
        assert np.array_equal(got.shares[j], sqs[y].half(a, i, s)), j
        assert np.array_equal(got.shares[j], sqset[y].axis_halves([(a, i, s)]).shares[0]), j
    assert len(sqset.axis_halves(np.zeros((0, 4), dtype=np.int64))) == 0


@pytest.mark.gpu
def test_serve_set_past_4gib(ctx):
    """The last member of a set whose EDS arena crosses 4 GiB (as tests/test_square_set.py builds one)."""
    import torch
    from celestia_da import proof as gpr
    k, n, period = 128, 130, 3
    three = np.stack([coracle.random_square(k, 4100 + i) for i in range(period)])
    d_three = torch.from_numpy(three).cuda()
    d_ods = d_three[torch.arange(n, device="cuda") % period].contiguous()
    sqset = gpr.ResidentSquareSet.from_device_ods(d_ods, k, n, ctx=ctx)
    del d_ods
    try:
        assert n * (2 * k) ** 2 * 512 > 1 << 32
        y = n - 1
        eds = coracle.extend(three[y % period]).reshape(2 * k, 2 * k, 512)
        c = serve_coords(k)
        got = sqset.axis_halves(np.concatenate([np.full((len(c), 1), y), c], axis=1))
        member = sqset[y].axis_halves(c)
        want = np.stack([ref.half_of(eds, a, i, s) for a, i, s in c.tolist()])
        assert np.array_equal(got.shares, want) and np.array_equal(member.shares, want)
    finally:
        sqset.close()


# ---------------------------------------------------------------- GPU: honest halves verify
def verify(ctx, batch, dahs, vectors=True):
    from celestia_da import axis_halves as ah
    return ah.verify_axis_halves(batch, dahs, ctx, vectors=vectors)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 4, 32, 128])
def test_verify_every_half(ctx, k):
    sq = square(k)
    coords = all_halves(k)
    v, vec = verify(ctx, batch_of(sq, coords), (sq.rows, sq.cols))
    assert not v.any(), np.nonzero(v)[0][:8]
    assert np.array_equal(vec, sq.vectors(coords))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_verify_right_halves_k128(ctx, n):
    """1, 2, 3 and 5 right halves: one codeword per workgroup, two, and two with a remainder of one."""
    k = 128
    sq = square(k)
    coords = np.array([(j & 1, (37 * j + 5) % (2 * k), 1) for j in range(n)], dtype=np.int64)
    v, vec = verify(ctx, batch_of(sq, coords), (sq.rows, sq.cols))
    assert not v.any() and np.array_equal(vec, sq.vectors(coords))


def sixteen(k):
    W = 2 * k
    idx = [0, 1, k - 1, k - 2, k, k + 1, W - 1, W - 2, 3, 5, k + 7, k + 9, k // 2, k // 2 + 1, W - 3, W - 5]
    return np.array([(j & 1, i, (j >> 1) & 1) for j, i in enumerate(idx)], dtype=np.int64)


@pytest.mark.gpu
def test_verify_k256(ctx):
    k = 256
    sq = square(k)
    coords = sixteen(k)
    assert len(coords) == 16
    v, vec = verify(ctx, batch_of(sq, coords), (sq.rows, sq.cols))
    assert not v.any() and np.array_equal(vec, sq.vectors(coords))


def synthetic(k, picks, seed):
    """Honest vectors without a square: random data under ascending namespaces, parity from the C oracle's
    encoder, the root of each from pyref.axis_root at its index.  (rows, cols, HalfBatch, vectors)."""
    from celestia_da import axis_halves as ah
    W = 2 * k
    rows, cols = np.zeros((W, 90), dtype=np.uint8), np.zeros((W, 90), dtype=np.uint8)
    halves, vectors = [], []
    for j, (axis, index, side) in enumerate(np.asarray(picks).tolist()):
        data = _rand((k, 512), seed + j)
        data[:, :29] = np.sort(_rand((k,), seed + 100 + j))[:, None]
        vec = np.concatenate([data, coracle.leopard_encode(data)])
        root = pyref.axis_root(vec, k, index)
        (rows if axis == 0 else cols)[index] = np.frombuffer(root, dtype=np.uint8)
        halves.append(vec[side * k:(side + 1) * k])
        vectors.append(vec)
    c4 = np.array([(0, *p) for p in np.asarray(picks).tolist()], dtype=np.int64)
    return rows, cols, ah.HalfBatch(k, c4, np.stack(halves)), np.stack(vectors)


@pytest.mark.gpu
def test_verify_k512(ctx):
    """Sixteen halves.  The oracle needs 14 s for the DAH of a k = 512 square, so the vectors are built one by
    one as at k = 1024: the verifier sees a half, its coordinates and a root, never the rest of a square."""
    k = 512
    rows, cols, batch, vectors = synthetic(k, sixteen(k), 7700)
    v, vec = verify(ctx, batch, (rows, cols))
    assert not v.any() and np.array_equal(vec, vectors)


@pytest.mark.gpu
def test_verify_k1024_synthetic(ctx):
    """No square at this width: four vectors, parity from the C oracle, roots from pyref.axis_root."""
    k = 1024
    rows, cols, batch, vectors = synthetic(k, [(0, 3, 0), (0, 700, 1), (1, 1500, 0), (1, 2047, 1)], 7300)
    v, vec = verify(ctx, batch, (rows, cols))
    assert not v.any() and np.array_equal(vec, vectors)


# ---------------------------------------------------------------- GPU: tampering
HONEST = [(0, 2, 0), (0, 3, 1), (1, 1, 0), (1, 6, 1), (0, 13, 0), (1, 12, 1), (0, 5, 1), (1, 9, 0)]


def expect_only(v, i, value):
    want = np.zeros(len(v), dtype=np.uint8)
    want[i] = value
    assert v.tolist() == want.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("i", [0, 3, 5, 7])
def test_flipped_byte(ctx, i):
    sq = square(8)
    b = batch_of(sq, HONEST)
    b.shares[i, 5, 400] ^= 0x10
    v, vec = verify(ctx, b, (sq.rows, sq.cols))
    expect_only(v, i, 1)
    a, idx, s = HONEST[i]
    assert v[i] == ref.verdict(b.shares[i], s, idx, (sq.rows if a == 0 else sq.cols)[idx].tobytes())[0]
    ok = [j for j in range(len(HONEST)) if j != i]
    assert np.array_equal(vec[ok], sq.vectors(HONEST)[ok])
    assert np.array_equal(vec[i], ref.complete(b.shares[i], s)), "the completed vector comes back whatever the verdict"


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["side", "index", "axis"])
def test_wrong_coordinate(ctx, what):
    sq = square(8)
    b = batch_of(sq, HONEST)
    i = 5   # (column 12, right): past k every cell hashes under the parity namespace, so no push can descend
    col = {"axis": 1, "index": 2, "side": 3}[what]
    b.coords[i, col] = {"axis": 0, "index": 13, "side": 0}[what]
    v = verify(ctx, b, (sq.rows, sq.cols), vectors=False)
    expect_only(v, i, 1)
    _, axis, index, side = b.coords[i].tolist()
    assert ref.verdict(b.shares[i], side, index, (sq.rows if axis == 0 else sq.cols)[index].tobytes())[0] == 1


@pytest.mark.gpu
def test_wrong_side_inside_q0(ctx):
    """The right half of a Q0 column sent as its left half: the parity bytes land in Q0 cells, their
    namespaces descend, and the push rule answers before the root does."""
    sq = square(8)
    b = batch_of(sq, HONEST)
    i = 3
    assert HONEST[i] == (1, 6, 1)
    b.coords[i, 3] = 0
    v = verify(ctx, b, (sq.rows, sq.cols), vectors=False)
    want = ref.verdict(b.shares[i], 0, 6, sq.cols[6].tobytes())[0]
    assert want == 2
    expect_only(v, i, want)


@pytest.mark.gpu
def test_wrong_square_of_a_set(ctx):
    k = 8
    sqs = [square(k, 40 + i) for i in range(3)]
    rows, cols = np.stack([s.rows for s in sqs]), np.stack([s.cols for s in sqs])
    from celestia_da import axis_halves as ah
    c4 = np.array([(j % 3, *HONEST[j]) for j in range(len(HONEST))], dtype=np.int64)
    shares = np.stack([sqs[y].half(a, i, s) for y, a, i, s in c4.tolist()])
    assert not verify(ctx, ah.HalfBatch(k, c4, shares), (rows, cols), vectors=False).any()
    c4[4, 0] = (c4[4, 0] + 1) % 3
    expect_only(verify(ctx, ah.HalfBatch(k, c4, shares), (rows, cols), vectors=False), 4, 1)


@pytest.mark.gpu
def test_swapped_q0_shares(ctx):
    sq = square(8)
    b = batch_of(sq, HONEST)
    i = 0   # the left half of Q0 row 2
    assert bytes(b.shares[i, 1, :29]) < bytes(b.shares[i, 6, :29])
    b.shares[i, [1, 6]] = b.shares[i, [6, 1]]
    v = verify(ctx, b, (sq.rows, sq.cols), vectors=False)
    expect_only(v, i, 2)
    assert ref.verdict(b.shares[i], 0, 2, sq.rows[2].tobytes())[0] == 2


@pytest.mark.gpu
def test_descending_row_under_blind_roots(ctx):
    """A square committed over blind roots with Q0 row 1 out of order: its right half rebuilds the committed
    root, and is refused all the same because nmt would not have pushed the recovered data."""
    from celestia_da import axis_halves as ah
    k = 4
    ods = coracle.random_square(k, 33).reshape(k, k, 512).copy()
    ods[1, [0, 3]] = ods[1, [3, 0]]
    eds = pyref.extend_square(ods)
    rows, cols, _ = pyref.dah_from_eds(eds, blind=True)
    to_np = lambda r: np.frombuffer(b"".join(r), dtype=np.uint8).reshape(2 * k, 90)   # noqa: E731
    coords = [(0, 0, 1), (0, 1, 1), (0, 2, 1), (0, 5, 1)]
    c4 = np.array([(0, *c) for c in coords], dtype=np.int64)
    shares = np.stack([ref.half_of(eds, *c) for c in coords])
    v, vec = verify(ctx, ah.HalfBatch(k, c4, shares), (to_np(rows), to_np(cols)))
    expect_only(v, 1, 2)
    assert np.array_equal(vec[1], eds[1])
    assert pyref.axis_root(eds[1], k, 1, blind=True) == rows[1], "the root itself matches"


# ---------------------------------------------------------------- GPU: refused inputs
def raw_verify(ctx, k, rows, cols, n_squares, squares, axes, indexes, sides, shares, want_vectors=True):
    from celestia_da._lib import ptr
    n = len(axes)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint32)   # noqa: E731
    squares, indexes = u32(squares), u32(indexes)
    axes, sides = np.ascontiguousarray(axes, dtype=np.uint8), np.ascontiguousarray(sides, dtype=np.uint8)
    verdict = np.full(n, 0xAA, dtype=np.uint8)
    vec = np.full((n, 2 * k, 512), 0xAA, dtype=np.uint8) if want_vectors else None
    rc = ctx.lib.cda_axis_halves_verify(ctx.h, k, ptr(rows), ptr(cols), n_squares,
                                        None if squares is None else squares.ctypes.data_as(U32P), ptr(axes),
                                        indexes.ctypes.data_as(U32P), ptr(sides), n, ptr(shares), ptr(verdict), ptr(vec))
    untouched = (verdict == 0xAA).all() and (vec is None or (vec == 0xAA).all())
    return rc, ctx.lib.cda_last_error(ctx.h).decode(), untouched, verdict


@pytest.mark.gpu
def test_verify_refused_inputs(ctx):
    k = 8
    sq = square(k)
    c = np.array(HONEST[:4], dtype=np.int64)
    shares = sq.halves(c)
    a, i, s = c[:, 0], c[:, 1], c[:, 2]
    INV = _lib.CDA_ERR_INVALID

    def bad(col, value):
        x = c.copy()
        x[2, col] = value
        return x[:, 0], x[:, 1], x[:, 2]

    rc, msg, clean, v = raw_verify(ctx, k, sq.rows, sq.cols, 1, None, a, i, s, shares)
    assert rc == _lib.CDA_OK and not v.any()
    rc, msg, clean, v = raw_verify(ctx, k, sq.rows, sq.cols, 1, None, a, i, s, shares, want_vectors=False)
    assert rc == _lib.CDA_OK and not v.any(), "a NULL vectors is accepted"
    rc, msg, clean, _ = raw_verify(ctx, k, sq.rows, sq.cols, 1, None, *bad(1, 16), shares)
    assert (rc, clean) == (INV, True) and msg == "half 2: index 16 is not below the EDS width 16"
    rc, msg, clean, _ = raw_verify(ctx, k, sq.rows, sq.cols, 1, None, *bad(0, 2), shares)
    assert (rc, clean) == (INV, True) and msg == "half 2: axis 2 is neither 0 (row) nor 1 (column)"
    rc, msg, clean, _ = raw_verify(ctx, k, sq.rows, sq.cols, 1, None, *bad(2, 2), shares)
    assert (rc, clean) == (INV, True) and msg == "half 2: side 2 is neither 0 (left) nor 1 (right)"
    rc, msg, clean, _ = raw_verify(ctx, k, sq.rows, sq.cols, 1, [0, 0, 0, 1], a, i, s, shares)
    assert (rc, clean) == (INV, True) and msg == "half 3: square 1 is not below the 1 squares"
    rc, msg, clean, _ = raw_verify(ctx, k, sq.rows, None, 1, None, a, i, s, shares)
    assert (rc, clean) == (INV, True) and msg.startswith("half 2: axis 1 (column) needs col_roots")
    rows_only = c[c[:, 0] == 0]
    rc, msg, clean, v = raw_verify(ctx, k, sq.rows, None, 1, None, rows_only[:, 0], rows_only[:, 1], rows_only[:, 2],
                                   sq.halves(rows_only))
    assert rc == _lib.CDA_OK and not v.any(), "col_roots may be NULL when no half is a column's"
    for wide in (3, 2048):
        rc, msg, clean, _ = raw_verify(ctx, wide, sq.rows, sq.cols, 1, None, a[:1], i[:1], s[:1], shares)
        assert (rc, clean) == (INV, True) and msg == "square width must be a power of two <= 1024"
    assert ctx.lib.cda_axis_halves_verify(ctx.h, k, None, None, 0, None, None, None, None, 0, None, None,
                                          None) == _lib.CDA_OK


@pytest.mark.gpu
@pytest.mark.parametrize("col,value,text", [(1, 16, "half 1: index 16 is not below the EDS width 16"),
                                            (0, 2, "half 1: axis 2 is neither 0 (row) nor 1 (column)"),
                                            (2, 3, "half 1: side 3 is neither 0 (left) nor 1 (right)")])
def test_serve_refused_inputs(resident, small_set, col, value, text):
    from celestia_da._lib import ptr
    k = 8
    rs = resident(k)
    c = np.array(HONEST[:3], dtype=np.int64)
    c[1, col] = value
    axes, idx, sides = (np.ascontiguousarray(c[:, 0], dtype=np.uint8), np.ascontiguousarray(c[:, 1], dtype=np.uint32),
                        np.ascontiguousarray(c[:, 2], dtype=np.uint8))
    out = np.full((3, k, 512), 0xAA, dtype=np.uint8)
    rc = rs.ctx.lib.cda_square_axis_halves(rs.h, ptr(axes), idx.ctypes.data_as(U32P), ptr(sides), 3, ptr(out))
    assert rc == _lib.CDA_ERR_INVALID and rs.ctx.lib.cda_last_error(rs.ctx.h).decode() == text
    assert (out == 0xAA).all()
    with pytest.raises(CdaError) as e:
        rs.axis_halves(c)
    assert e.value.code == _lib.CDA_ERR_INVALID and text in str(e.value)
    sqset, _ = small_set
    squares = np.array([0, 2, 1], dtype=np.uint32)
    rc = sqset.ctx.lib.cda_square_set_axis_halves(sqset.h, squares.ctypes.data_as(U32P), ptr(axes),
                                                  idx.ctypes.data_as(U32P), ptr(sides), 3, ptr(out))
    assert rc == _lib.CDA_ERR_INVALID and sqset.ctx.lib.cda_last_error(sqset.ctx.h).decode() == text
    assert (out == 0xAA).all()


@pytest.mark.gpu
def test_serve_set_refuses_a_square_past_the_set(small_set):
    sqset, _ = small_set
    with pytest.raises(CdaError) as e:
        sqset.axis_halves([(0, 0, 1, 0), (3, 1, 2, 1)])
    assert e.value.code == _lib.CDA_ERR_INVALID and "half 1: square 3 is not below the 3 squares" in str(e.value)


# ---------------------------------------------------------------- GPU: end to end
def _repair(ctx, eds, present, rows, cols):
    from celestia_da import rsmt2d, wrapper
    sq = rsmt2d.new_extended_data_square_with_missing(eds, present, rsmt2d.LeoRSCodec(ctx),
                                                     wrapper.new_constructor(eds.shape[0] // 2))
    sq.repair(rows, cols, present)
    return sq.array().reshape(eds.shape)


def random_rows(k, seed):
    """k distinct rows of the EDS with random sides."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(2 * k, size=k, replace=False)
    return np.array([(0, int(r), int(rng.integers(0, 2))) for r in rows], dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [8, 128])
def test_serve_verify_assemble_repair(ctx, resident, k):
    from celestia_da import axis_halves as ah
    sq, rs = square(k), resident(k)
    coords = random_rows(k, 7500 + k)
    assert {0, 1} <= set(coords[:, 2].tolist())
    batch = rs.axis_halves(coords)
    v, vec = ah.verify_axis_halves(batch, (sq.rows, sq.cols), ctx, vectors=True)
    assert not v.any()
    eds, present = ah.assemble(batch, v, vec)
    assert present.sum() == k * 2 * k
    rows, cols = [r.tobytes() for r in sq.rows], [c.tobytes() for c in sq.cols]
    assert np.array_equal(_repair(ctx, eds, present, rows, cols), sq.eds)


@pytest.mark.gpu
def test_serve_verify_assemble_repair_batch(ctx, small_set):
    from celestia_da import axis_halves as ah
    from celestia_da import rsmt2d
    sqset, sqs = small_set
    k, n = sqset.k, len(sqs)
    coords = np.concatenate([np.concatenate([np.full((k, 1), y), random_rows(k, 7600 + y)], axis=1) for y in range(n)])
    batch = sqset.axis_halves(coords)
    rows, cols = np.stack([s.rows for s in sqs]), np.stack([s.cols for s in sqs])
    v, vec = ah.verify_axis_halves(batch, (rows, cols), ctx, vectors=True)
    assert not v.any()
    eds, present = ah.assemble_batch(batch, v, vec)
    assert eds.shape == (n, 2 * k, 2 * k, 512)
    out = rsmt2d.repair_batch(eds, present, rows, cols, ctx)
    assert all(o.ok for o in out)
    assert np.array_equal(eds, np.stack([s.eds for s in sqs]))
