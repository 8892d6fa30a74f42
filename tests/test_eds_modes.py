"""cda_extend_dah_batch_ex: the caller keeps Q0.

pkg/da/data_availability_header.go:65-75 returns an EDS whose Q0 cells are
the input shares; a cgo caller already holds them, so the library can leave
Q0 out of what it returns: CDA_EDS_SKIP_Q0 (the EDS layout, Q0 untouched) or
CDA_EDS_PARITY (per square Q1 then rows k..2k-1, packed, one linear copy per
chunk).  Both must give the full path's bytes once reassembled, on the small
serial host path and on the chunk pipeline (slot wraps, ragged tail), with
the same roots and push-order status."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import coracle
from celestia_da import CdaError, _lib, da
from knobs import ctx_with

pytestmark = pytest.mark.gpu


def _ctx_with(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(int(os.environ.get("CDA_DEVICE", "-1")))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("k,n,env", [(32, 3, {}), (64, 2, {}), (32, 7, {"CDA_HOST_PIPE_CHUNK": "2"}),
                                     (16, 10, {"CDA_HOST_PIPE_CHUNK": "3"})])
def test_parity_modes_match_full_eds(ctx, k, n, env):
    ods = np.stack([coracle.random_square(k, 1200 + i) for i in range(n)])
    bad = n - 1
    sq = ods[bad].reshape(k, k, 512)
    sq[1, 2, :29], sq[1, 3, :29] = sq[1, 3, :29].copy(), sq[1, 2, :29].copy()
    full = da.extend_dah_batch(ods, ctx=ctx)
    pc = _ctx_with(env) if env else ctx
    try:
        par = da.extend_dah_batch_parity(ods, ctx=pc)
        skip = da.extend_dah_batch_parity(ods, ctx=pc, skip_q0=True)
    finally:
        if env:
            pc.close()
    for got in (par, skip):
        for a, b in zip(full[1:], got[1:]):   # rows, cols, data roots, status
            assert np.array_equal(a, b)
    assert [bool(x) for x in full[4] != 0] == [bool(x) for x in par[4] != 0]
    for i in range(n):
        assert np.array_equal(da.unpack_parity(ods[i], par[0][i]), full[0][i]), i
        assert not skip[0][i][:k, :k].any()                                     # Q0 untouched (zeros)
        assert np.array_equal(skip[0][i][:k, k:], full[0][i][:k, k:])
        assert np.array_equal(skip[0][i][k:], full[0][i][k:])
    assert bytes(full[3][0]) == coracle.extend_dah(ods[0])[3]


# The seams of the host-batch paths' shared head and tail (Engine::host_stage /
# host_finish): k = 8, n = 6 is two chunks (4 + 2) on the small path under
# CDA_HOST_CHUNK's default of 4, and three chunks on the pipeline with
# CDA_HOST_PIPE_CHUNK=2; the cases above stay within one small-path chunk.
SEAM_K, SEAM_N, SEAM_BAD = 8, 6, 5
MODES = {"full": _lib.CDA_EDS_FULL, "skip_q0": _lib.CDA_EDS_SKIP_Q0, "parity": _lib.CDA_EDS_PARITY}


@functools.lru_cache(maxsize=None)
def _seam_batch():
    """(ods, per-square oracle (eds, rows, cols, root)); read-only."""
    ods = np.stack([coracle.random_square(SEAM_K, 1400 + i) for i in range(SEAM_N)])
    ods.setflags(write=False)
    return ods, [coracle.extend_dah(o) for o in ods]


def _batch_ex(c, ods, mode):
    """cda_extend_dah_batch_ex -> (rc, out, rows, cols, roots, status)."""
    n, k, W = len(ods), SEAM_K, 2 * SEAM_K
    out = (np.empty((n, 3 * k * k, 512), dtype=np.uint8) if mode == _lib.CDA_EDS_PARITY
           else np.zeros((n, W, W, 512), dtype=np.uint8))
    rows = np.empty((n, W, 90), dtype=np.uint8)
    cols = np.empty((n, W, 90), dtype=np.uint8)
    roots = np.empty((n, 32), dtype=np.uint8)
    status = np.full(n, 99, dtype=np.int32)
    rc = c.lib.cda_extend_dah_batch_ex(c.h, _lib.ptr(np.ascontiguousarray(ods)), k, n, _lib.ptr(out), mode,
                                       _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(roots),
                                       status.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out, rows, cols, roots, status


@pytest.mark.parametrize("mode", sorted(MODES))
def test_two_chunk_small_path_matches_oracle(ctx, mode):
    ods, want = _seam_batch()
    k = SEAM_K
    rc, out, rows, cols, roots, status = _batch_ex(ctx, ods, MODES[mode])
    assert rc == _lib.CDA_OK and list(status) == [0] * SEAM_N
    for i, (e_eds, e_rows, e_cols, e_root) in enumerate(want):
        e_eds = np.asarray(e_eds).reshape(2 * k, 2 * k, 512)
        if mode == "parity":
            assert np.array_equal(da.unpack_parity(ods[i], out[i]), e_eds), i
        elif mode == "skip_q0":
            assert not out[i][:k, :k].any(), i                                  # Q0 untouched (zeros)
            assert np.array_equal(out[i][:k, k:], e_eds[:k, k:]) and np.array_equal(out[i][k:], e_eds[k:]), i
        else:
            assert np.array_equal(out[i], e_eds), i
        assert [bytes(r) for r in rows[i]] == [bytes(r) for r in e_rows], i
        assert [bytes(c) for c in cols[i]] == [bytes(c) for c in e_cols], i
        assert bytes(roots[i]) == bytes(e_root), i


def _first_violation(q0):
    """Brute-force nmt push-order check of Q0: the smallest (axis, index,
    position) whose namespace is below its predecessor's, rows before columns."""
    k = q0.shape[0]
    ns = [[bytes(q0[r, c, :29]) for c in range(k)] for r in range(k)]
    bad = [(0, r, c) for r in range(k) for c in range(1, k) if ns[r][c] < ns[r][c - 1]]
    bad += [(1, c, r) for c in range(k) for r in range(1, k) if ns[r][c] < ns[r - 1][c]]
    return min(bad) if bad else None


@pytest.mark.parametrize("path", ["small", "pipeline"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_violation_in_second_chunk(ctx, mode, path):
    """A Q0 namespace violation in square 5 only -- the second chunk of the
    small path, the third of the pipeline: the shared tail reports it."""
    k = SEAM_K
    ods = _seam_batch()[0].copy()
    sq = ods[SEAM_BAD].reshape(k, k, 512)
    sq[1, 2, :29], sq[1, 3, :29] = sq[1, 3, :29].copy(), sq[1, 2, :29].copy()
    want = _first_violation(sq)
    assert want is not None and all(_first_violation(o.reshape(k, k, 512)) is None for o in ods[:SEAM_BAD])
    c = ctx_with({"CDA_HOST_PIPE_CHUNK": "2"}) if path == "pipeline" else ctx
    try:
        rc, *_, status = _batch_ex(c, ods, MODES[mode])
        detail = c.push_order_detail()
        text = c.lib.cda_last_error(c.h).decode()
    finally:
        if c is not ctx:
            c.close()
    assert rc == _lib.CDA_ERR_PUSH_ORDER
    assert list(status) == [0, 0, 0, 0, 0, -3]
    assert detail == want
    axis, index, pos = want
    cell = (lambda p: sq[index, p]) if axis == 0 else (lambda p: sq[p, index])
    assert text == ("pushed data has to be lexicographically ordered by namespace IDs: last namespace: "
                    f"{bytes(cell(pos - 1)[:29]).hex()}, pushed: {bytes(cell(pos)[:29]).hex()}")


def test_unknown_eds_mode_rejected(ctx):
    ods = coracle.random_square(4, 0)
    out = np.empty(3 * 16 * 512, dtype=np.uint8)
    rows = np.empty(8 * 90, dtype=np.uint8)
    cols = np.empty(8 * 90, dtype=np.uint8)
    roots = np.empty(32, dtype=np.uint8)
    rc = ctx.lib.cda_extend_dah_batch_ex(ctx.h, _lib.ptr(ods), 4, 1, _lib.ptr(out), 7, _lib.ptr(rows), _lib.ptr(cols),
                                         _lib.ptr(roots), None)
    assert rc == _lib.CDA_ERR_INVALID
    with pytest.raises(CdaError, match="unknown eds_mode"):
        ctx.check(rc)


def test_parity_staging_released_with_context():
    """the packed-parity staging buffer is released when
    its context is destroyed.  Creating a context, making a CDA_EDS_PARITY
    call on the chunk pipeline and closing it, three times over, must not
    keep device memory (each round stages ~170 MiB at k=128, n=6, chunk 3)."""
    import torch
    k, n = 128, 6
    ods = np.stack([coracle.random_square(k, 1300 + i) for i in range(n)])

    def round_trip():
        pc = _ctx_with({"CDA_HOST_PIPE_CHUNK": "3"})
        try:
            da.extend_dah_batch_parity(ods, ctx=pc)
        finally:
            pc.close()

    round_trip()                       # first-use allocations (HIP runtime, pools)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        round_trip()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 128 << 20, f"{(free0 - free1) >> 20} MiB kept after 3 context round trips"
