"""The footprint of the caller-owned buffers of the square-set calls, with
tests/guarded.py as tests/test_output_footprint.py uses it: every output and
every const input lies inside lead | payload | trail filled with a pattern.

  cda_square_set_dah            row_roots, col_roots n*2k*90, data_roots n*32, status n*4
  cda_square_set_sample_proofs  the six arrays of cda_square_sample_proofs
  cda_square_set_create_device  device_src: read only, documented alignment 16

Each case asserts: the payload equals what singly created squares answer, the
guards still hold the pattern, a NULL output or a refused call writes nothing,
and every input is byte-identical afterwards.  The one device pointer is placed
once 256-byte aligned and once at exactly its documented minimum.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coracle
import guarded

HERE = os.path.dirname(os.path.abspath(__file__))
U8P, U32P, I32P = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_int32))
OK, INVALID = 0, -6
SRC_ALIGN = 16   # device_src: the widest access through it is a 16-byte load


def _p(g, t=U8P):
    return C.cast(g.ptr, t)


def log2(x):
    return x.bit_length() - 1


def test_header_states_the_alignment_of_the_device_source():
    """include/cda.h names the device pointer of cda_square_set_create_device and gives it 16 bytes."""
    with open(os.path.join(os.path.dirname(HERE), "include", "cda.h")) as f:
        header = f.read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    args = dict(re.findall(r"\bint\s+(cda_\w+)\s*\(([^)]*)\)\s*;", code))["cda_square_set_create_device"]
    assert re.search(r"const\s+void\s*\*\s*device_src\b", args), args
    flat = " ".join(header.replace("*", " ").split())
    assert re.search(rf"\bdevice_src\b[^.;]*? {SRC_ALIGN}-byte aligned", flat)


def test_argument_errors_that_need_no_device():
    """Without a context nothing can be built: the create calls answer CDA_ERR_INVALID and leave *out NULL; the
    calls on a set refuse a NULL set; destroying NULL is CDA_OK; the mirror knows the symbols."""
    from celestia_da import _lib
    L = _lib.load()
    src = np.zeros(512, dtype=np.uint8)
    for call in (lambda h: L.cda_square_set_create(None, _lib.ptr(src), _lib.CDA_SET_FROM_ODS, 1, 1, C.byref(h)),
                 lambda h: L.cda_square_set_create_device(None, 4096, _lib.CDA_SET_FROM_EDS, 1, 1, None, C.byref(h))):
        h = C.c_void_p(0xDEAD)
        assert call(h) == INVALID and not h.value
    assert L.cda_square_set_create(None, _lib.ptr(src), 0, 1, 1, None) == INVALID
    assert L.cda_square_set_create_device(None, 4096, 0, 1, 1, None, None) == INVALID
    m = C.c_void_p(0xDEAD)
    assert L.cda_square_set_at(None, 0, C.byref(m)) == INVALID
    assert L.cda_square_set_info(None, None, None) == INVALID
    assert L.cda_square_set_dah(None, None, None, None, None) == INVALID
    assert L.cda_square_set_sample_proofs(None, None, None, None, None, 0, None, None, None, None, None, None) == INVALID
    assert L.cda_square_set_destroy(None) == OK
    assert (_lib.CDA_SET_FROM_ODS, _lib.CDA_SET_FROM_EDS) == (0, 1)
    from celestia_da import proof, replay, sampling
    assert all(hasattr(proof.ResidentSquareSet, n) for n in
               ("from_ods", "from_eds", "from_device_ods", "from_device_eds", "__len__", "__getitem__", "dah", "close"))
    assert hasattr(sampling, "sample_proofs_set") and "keep" in replay.replay.__code__.co_varnames


def _ods(k, n):
    return np.stack([coracle.random_square(k, 9100 + 8 * k + i) for i in range(n)])


def _singles(ctx, ods):
    from celestia_da import proof as gpr
    return [gpr.ResidentSquare(o, ctx) for o in ods]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["aligned256", "minimum"])
@pytest.mark.parametrize("k,n", [(1, 3), (2, 3), (4, 17)])
def test_set_create_device_and_dah(ctx, k, n, mode):
    from celestia_da import _lib
    W = 2 * k
    ods = _ods(k, n)
    d_src = guarded.from_data(ods, stride=k * k * 512, align=SRC_ALIGN if mode == "minimum" else 256,
                              backend="torch", name="device_src")
    if mode == "minimum":
        assert d_src.ptr % 256 == SRC_ALIGN
    h = C.c_void_p()
    assert ctx.lib.cda_square_set_create_device(ctx.h, d_src.ptr, _lib.CDA_SET_FROM_ODS, k, n, None, C.byref(h)) == OK
    singles = _singles(ctx, ods)
    try:
        d_src.assert_unchanged()
        want = [s.dah() for s in singles]
        exp_rows = b"".join(b"".join(r) for r, _, _ in want)
        exp_cols = b"".join(b"".join(c) for _, c, _ in want)
        exp_roots = b"".join(d for _, _, d in want)
        names = ("row_roots", "col_roots", "data_roots", "status")
        sizes = (n * W * 90, n * W * 90, n * 32, n * 4)
        strides = (W * 90, W * 90, 32, 4)
        expected = (np.frombuffer(exp_rows, np.uint8), np.frombuffer(exp_cols, np.uint8),
                    np.frombuffer(exp_roots, np.uint8), np.zeros(n, np.int32).view(np.uint8))
        for mask in (15, 1, 2, 4, 8, 5, 10, 0):   # all, each alone, pairs, none
            bufs = [guarded.alloc(sz, stride=st, align=2 if j < 2 else 4, backend="numpy", name=nm)
                    for j, (nm, sz, st) in enumerate(zip(names, sizes, strides))]
            args = [_p(b, I32P if j == 3 else U8P) if mask >> j & 1 else None for j, b in enumerate(bufs)]
            assert ctx.lib.cda_square_set_dah(h, *args) == OK, mask
            for j, b in enumerate(bufs):
                if mask >> j & 1:
                    b.assert_written(expected[j])
                    b.assert_guards()
                else:
                    b.assert_untouched()
        d_src.assert_unchanged()
    finally:
        for s in singles:
            s.close()
        ctx.lib.cda_square_set_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,count", [(1, 3, 7), (2, 3, 33), (4, 5, 258)])
def test_set_sample_proofs(ctx, k, n, count):
    from celestia_da import proof as gpr
    W, D = 2 * k, log2(2 * k)
    ods = _ods(k, n)
    sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    singles = _singles(ctx, ods)
    try:
        rng = np.random.default_rng(count)
        req = [rng.integers(0, n, count).astype(np.uint32), rng.integers(0, W, count).astype(np.uint32),
               rng.integers(0, W, count).astype(np.uint32), rng.integers(0, 2, count).astype(np.uint8)]
        ins = [guarded.from_data(a, align=4 if j < 3 else 1, backend="numpy", name=nm)
               for j, (a, nm) in enumerate(zip(req, ("squares", "rows", "cols", "axes")))]
        in_args = [_p(g, U32P if j < 3 else U8P) for j, g in enumerate(ins)]
        names = ("shares", "namespaces", "nmt_nodes", "axis_roots", "leaf_hash", "aunts")
        item = (512, 29, D * 90, 90, 32, (D + 1) * 32)
        expected = [np.zeros((count, s), np.uint8) for s in item]
        for y in range(n):
            pick = np.nonzero(req[0] == y)[0]
            if pick.size:
                b = singles[y].sample_proofs(np.stack([req[1][pick], req[2][pick], req[3][pick]], axis=1))
                for dst, a in zip(expected, b.arrays()):
                    dst[pick] = a.reshape(pick.size, -1)

        def run(mask, inputs=in_args):
            bufs = [guarded.alloc(count * s, stride=s, align=1, backend="numpy", name=nm) for nm, s in zip(names, item)]
            args = [_p(b) if mask >> j & 1 else None for j, b in enumerate(bufs)]
            return ctx.lib.cda_square_set_sample_proofs(sqset.h, *inputs, count, *args), bufs

        for mask in [63] + [1 << j for j in range(6)] + [63 ^ (1 << j) for j in range(6)] + [0]:
            rc, bufs = run(mask)
            assert rc == OK, mask
            for j, b in enumerate(bufs):
                if mask >> j & 1:
                    b.assert_written(expected[j])
                    b.assert_guards()
                else:
                    b.assert_untouched()
        # a refused call (square out of range in the last sample) writes nothing
        bad_sq = req[0].copy()
        bad_sq[-1] = n
        bad = guarded.from_data(bad_sq, align=4, backend="numpy", name="squares")
        rc, bufs = run(63, [_p(bad, U32P)] + in_args[1:])
        assert rc == INVALID
        assert ctx.lib.cda_last_error(ctx.h).decode().startswith(f"sample {count - 1}: square {n} ")
        for b in bufs:
            b.assert_untouched()
        bad.assert_unchanged()
        for g in ins:
            g.assert_unchanged()
    finally:
        for s in singles:
            s.close()
        sqset.close()
