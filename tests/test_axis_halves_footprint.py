"""The footprint of the caller-owned buffers of the axis-half calls, with
tests/guarded.py: every output and every const input lies inside
lead | payload | trail filled with a pattern.

  cda_square_axis_halves       axes n, indexes n*4, sides n (inputs); shares n*k*512
  cda_square_set_axis_halves   squares n*4 and the same
  cda_axis_halves_verify       row_roots, col_roots n_squares*2k*90, squares, axes, indexes, sides,
                               shares n*k*512 (inputs); verdict n, vectors n*2k*512 (or NULL)
  cda_rs_recover_data          parity (input); data, n_codewords*n_shards*shard_len each

Each case asserts: the payload equals the oracle's bytes, the guards still hold
the pattern, a NULL vectors is accepted, a refused call writes nothing, and
every input is byte-identical afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import axis_halves_ref as ref
import coracle
import guarded

U8P, U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
OK, INVALID, UNSUPPORTED, CHUNK = 0, -6, -7, -2


def _p(g, t=U8P):
    return None if g is None else C.cast(g.ptr, t)


def test_argument_errors_that_need_no_device():
    """A NULL square, set or context is refused before any device work, and the mirror knows the symbols."""
    from celestia_da import _lib, axis_halves, proof
    L = _lib.load()
    a = np.zeros(1, dtype=np.uint8)
    i = np.zeros(1, dtype=np.uint32)
    out = np.full((1, 512), 0xAA, dtype=np.uint8)
    u32 = i.ctypes.data_as(U32P)
    assert L.cda_square_axis_halves(None, _lib.ptr(a), u32, _lib.ptr(a), 1, _lib.ptr(out)) == INVALID
    assert L.cda_square_set_axis_halves(None, u32, _lib.ptr(a), u32, _lib.ptr(a), 1, _lib.ptr(out)) == INVALID
    verdict = np.full(1, 0xAA, dtype=np.uint8)
    roots = np.zeros((2, 90), dtype=np.uint8)
    assert L.cda_axis_halves_verify(None, 1, _lib.ptr(roots), _lib.ptr(roots), 1, None, _lib.ptr(a), u32, _lib.ptr(a),
                                    1, _lib.ptr(out), _lib.ptr(verdict), None) == INVALID
    assert L.cda_last_error(None).decode() == "null context"
    assert L.cda_rs_recover_data(None, _lib.ptr(out), 1, 512, 1, _lib.ptr(out)) == INVALID
    assert verdict[0] == 0xAA and (out == 0xAA).all()
    assert all(hasattr(p, "axis_halves") for p in (proof.ResidentSquare, proof.ResidentSquareSet))
    assert all(hasattr(axis_halves, n) for n in ("HalfBatch", "serve", "serve_set", "verify_axis_halves", "assemble",
                                                 "assemble_batch", "recover_data"))


def _coords(k, n, count, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, n, count).astype(np.uint32), rng.integers(0, 2, count).astype(np.uint8),
            rng.integers(0, 2 * k, count).astype(np.uint32), rng.integers(0, 2, count).astype(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,count", [(2, 3, 9), (16, 2, 23)])
def test_serving_and_the_verifier(ctx, k, n, count):
    from celestia_da import proof as gpr
    W, half_b = 2 * k, k * 512
    ods = np.stack([coracle.random_square(k, 9700 + 8 * k + y) for y in range(n)])
    dah = [coracle.extend_dah(o) for o in ods]
    eds = [d[0].reshape(W, W, 512) for d in dah]
    rows, cols = np.stack([d[1] for d in dah]), np.stack([d[2] for d in dah])
    squares, axes, indexes, sides = _coords(k, n, count, 11 * k)
    want = np.stack([ref.half_of(eds[y], a, i, s) for y, a, i, s in zip(squares, axes, indexes, sides)])
    vecs = np.stack([eds[y][i] if a == 0 else eds[y][:, i] for y, a, i in zip(squares, axes, indexes)])
    g_sq = guarded.from_data(squares, align=4, name="squares")
    g_ax = guarded.from_data(axes, align=1, name="axes")
    g_ix = guarded.from_data(indexes, align=4, name="indexes")
    g_sd = guarded.from_data(sides, align=1, name="sides")
    inputs = [g_sq, g_ax, g_ix, g_sd]
    sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    try:
        # serving from the set, and from one member
        g_out = guarded.alloc(count * half_b, stride=half_b, align=1, name="shares")
        assert ctx.lib.cda_square_set_axis_halves(sqset.h, _p(g_sq, U32P), _p(g_ax), _p(g_ix, U32P), _p(g_sd), count,
                                                  _p(g_out)) == OK
        g_out.assert_written(want)
        g_out.assert_guards()
        pick = np.nonzero(squares == squares[0])[0]
        g_one = guarded.alloc(len(pick) * half_b, stride=half_b, align=1, name="shares of one square")
        ax1, ix1, sd1 = (guarded.from_data(x[pick], align=al, name=nm) for x, al, nm in
                         ((axes, 1, "axes"), (indexes, 4, "indexes"), (sides, 1, "sides")))
        member = sqset[int(squares[0])]
        assert ctx.lib.cda_square_axis_halves(member.h, _p(ax1), _p(ix1, U32P), _p(sd1), len(pick), _p(g_one)) == OK
        g_one.assert_written(want[pick])
        g_one.assert_guards()
        for g in (ax1, ix1, sd1):
            g.assert_unchanged()
        # a refused call writes nothing
        bad = indexes.copy()
        bad[count // 2] = W
        g_bad = guarded.from_data(bad, align=4, name="indexes")
        g_out.refill()
        assert ctx.lib.cda_square_set_axis_halves(sqset.h, _p(g_sq, U32P), _p(g_ax), _p(g_bad, U32P), _p(g_sd), count,
                                                  _p(g_out)) == INVALID
        g_out.assert_untouched()
        g_bad.assert_unchanged()
    finally:
        sqset.close()
    # the verifier: vectors given, vectors NULL, refused
    g_rows = guarded.from_data(rows, stride=W * 90, align=1, name="row_roots")
    g_cols = guarded.from_data(cols, stride=W * 90, align=1, name="col_roots")
    g_sh = guarded.from_data(want, stride=half_b, align=1, name="shares")
    inputs += [g_rows, g_cols, g_sh]

    def run(with_vectors, ix=g_ix):
        g_v = guarded.alloc(count, align=1, name="verdict")
        g_vec = guarded.alloc(count * 2 * half_b, stride=2 * half_b, align=1, name="vectors")
        rc = ctx.lib.cda_axis_halves_verify(ctx.h, k, _p(g_rows), _p(g_cols), n, _p(g_sq, U32P), _p(g_ax),
                                            _p(ix, U32P), _p(g_sd), count, _p(g_sh), _p(g_v),
                                            _p(g_vec) if with_vectors else None)
        return rc, g_v, g_vec

    rc, g_v, g_vec = run(True)
    assert rc == OK
    g_v.assert_written(np.zeros(count, dtype=np.uint8))
    g_v.assert_guards()
    g_vec.assert_written(vecs)
    g_vec.assert_guards()
    rc, g_v, g_vec = run(False)
    assert rc == OK
    g_v.assert_written(np.zeros(count, dtype=np.uint8))
    g_v.assert_guards()
    g_vec.assert_untouched()
    rc, g_v, g_vec = run(True, ix=g_bad)
    assert rc == INVALID
    g_v.assert_untouched()
    g_vec.assert_untouched()
    for g in inputs:
        g.assert_unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("k,L", [(4, 64), (128, 512), (128, 192), (256, 512)])
def test_rs_recover_data(ctx, k, L):
    n = 3
    data = np.random.default_rng(k + L).integers(0, 256, size=(n, k, L), dtype=np.uint8)
    parity = np.stack([coracle.leopard_encode(d) for d in data])
    g_in = guarded.from_data(parity, stride=k * L, align=1, name="parity")
    g_out = guarded.alloc(n * k * L, stride=k * L, align=1, name="data")
    assert ctx.lib.cda_rs_recover_data(ctx.h, _p(g_in), k, L, n, _p(g_out)) == OK
    g_out.assert_written(data)
    g_out.assert_guards()
    g_out.refill()
    assert ctx.lib.cda_rs_recover_data(ctx.h, _p(g_in), 3 * k, L, n // 3, _p(g_out)) == UNSUPPORTED
    g_out.assert_untouched()
    assert ctx.lib.cda_rs_recover_data(ctx.h, _p(g_in), k, L // 2 + 16, n, _p(g_out)) == CHUNK
    g_out.assert_untouched()
    g_in.assert_unchanged()
