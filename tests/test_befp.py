"""Bad-encoding fraud proofs on the GPU (cda_befp_build / cda_befp_verify, celestia_da.byzantine) against the CPU
yardstick tests/befp_ref.py, whose own verdicts tests/test_befp_ref.py pins."""
import ctypes as C

import numpy as np
import pytest

import befp_ref as ref
import coracle
import pyref
import repair as orepair
from celestia_da import CdaError, _lib, byzantine
from celestia_da._lib import ptr
from test_befp_check import MALFORMED, break_batch, packed

pytestmark = pytest.mark.gpu


def device_copy(a: np.ndarray):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to("cuda")
    torch.cuda.synchronize()
    return d


# ------------------------------------------------------------------- the builder
@pytest.mark.parametrize("k", [2, 8])
def test_builder_on_an_honest_square(ctx, k):
    sq = ref.honest_square(k)
    W = 2 * k
    rows, cols = sq.rows_array(), sq.cols_array()
    d = device_copy(sq.eds)
    for axis in (ref.ROW, ref.COL):
        for index in (0, k - 1, k, W - 1):
            want = ref.prove(sq, axis, index, range(W))
            pos, shares, nodes = byzantine.build_shares(sq.eds, rows, cols, axis, index, ctx)
            assert pos.tolist() == list(range(W)), (axis, index)
            assert np.array_equal(shares, sq.vector(axis, index)), (axis, index)
            assert np.array_equal(nodes, want.nmt_nodes), (axis, index)
            dpos, dshares, dnodes = byzantine.build_shares(d.data_ptr(), rows, cols, axis, index, ctx)
            assert np.array_equal(dpos, pos) and np.array_equal(dshares, shares) and np.array_equal(dnodes, nodes)


def test_builder_skips_cells_whose_orthogonal_vector_has_a_hole(ctx):
    k, W = 4, 8
    sq = ref.honest_square(k)
    rows, cols = sq.rows_array(), sq.cols_array()
    for axis, index, holes in ((ref.ROW, 1, ((0, 1), (5, 4), (7, 6))), (ref.COL, 6, ((0, 1), (3, 0), (7, 7)))):
        eds = sq.eds.copy()
        skipped = set()
        for r, c in holes:   # (row, col) of the zeroed cell, none of them on the accused vector
            assert (r if axis == ref.ROW else c) != index
            eds[r, c] = 0
            skipped.add(c if axis == ref.ROW else r)
        assert len(skipped) == 3
        pos, shares, nodes = byzantine.build_shares(eds, rows, cols, axis, index, ctx)
        assert pos.tolist() == [p for p in range(W) if p not in skipped]
        want = ref.build(eds, sq.rows, sq.cols, axis, index)
        assert np.array_equal(pos, want.positions) and np.array_equal(shares, want.shares)
        assert np.array_equal(nodes, want.nmt_nodes)


def test_builder_rejects_bad_arguments(ctx):
    sq = ref.honest_square(2)
    rows, cols = sq.rows_array(), sq.cols_array()
    with pytest.raises(CdaError, match="index 4 is not below the EDS width 4"):
        byzantine.build_shares(sq.eds, rows, cols, ref.ROW, 4, ctx)
    with pytest.raises(CdaError, match="axis 2 is neither"):
        byzantine.build_shares(sq.eds, rows, cols, 2, 0, ctx)


# ------------------------------------------------------------------ the verifier
@pytest.mark.parametrize("k", [2, 8])
def test_verifier_mixed_batch_matches_the_yardstick(ctx, k):
    cs = ref.cases(k)
    proofs = [c[1] for c in cs]
    dahs = [(c[2], c[3]) for c in cs]
    want = [ref.validate(p, r, c) for _, p, r, c, _ in cs]
    assert len(cs) >= 9 and {w[0] for w in want} == {0, 1, 2, 3}
    verdict, rebuilt = byzantine.verify_batch(proofs, dahs, ctx)
    for i, (name, *_rest, stated) in enumerate(cs):
        assert verdict[i] == want[i][0] == stated, name
        assert rebuilt[i].tobytes() == want[i][1], name
    # the same proofs one per call
    for i, (name, *_rest) in enumerate(cs):
        v1, r1 = byzantine.verify_batch([proofs[i]], [dahs[i]], ctx)
        assert v1[0] == want[i][0] and r1[0].tobytes() == want[i][1], name
    # and through the public call: None where the fraud is confirmed, else a reason
    reasons = byzantine.validate_bad_encoding_proofs(proofs, dahs, ctx)
    assert [r is None for r in reasons] == [w[0] == 0 for w in want]
    assert all(r == byzantine.REASONS[w[0]] for r, w in zip(reasons, want) if w[0])


def test_verifier_null_proof_axes_and_no_rebuilt_roots(ctx):
    """proof_axes NULL means every proof is against the orthogonal root; rebuilt_roots may be NULL."""
    k = 2
    sq = ref.malicious_square(k)
    r, _ = ref.flipped_cell(k)
    p = ref.prove(sq, ref.ROW, r, range(2 * k))
    b, keep = byzantine.pack_batch([p, ref.prove(ref.honest_square(k), ref.COL, 0, range(2 * k))],
                                   [sq.dah(), ref.honest_square(k).dah()])
    b.proof_axes = None
    verdict = np.full(2, 255, dtype=np.uint8)
    ctx.check(ctx.lib.cda_befp_verify(ctx.h, C.byref(b), ptr(verdict), None))
    assert verdict.tolist() == [0, 3]
    assert ctx.lib.cda_befp_verify(ctx.h, C.byref(_lib.BefpBatch()), None, None) == _lib.CDA_OK
    del keep


@pytest.mark.parametrize("what,text", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_batch_is_invalid_and_leaves_the_verdict(ctx, what, text):
    b, keep = packed()
    break_batch(what, b, keep)
    verdict = np.full(2, 0xAB, dtype=np.uint8)
    rebuilt = np.full((2, 90), 0xCD, dtype=np.uint8)
    assert ctx.lib.cda_befp_verify(ctx.h, C.byref(b), ptr(verdict), ptr(rebuilt)) == _lib.CDA_ERR_INVALID
    assert ctx.lib.cda_last_error(ctx.h).decode() == text
    assert (verdict == 0xAB).all() and (rebuilt == 0xCD).all()


# -------------------------------------------------------------------- end to end
@pytest.mark.parametrize("k", [4, 8])
def test_repair_to_fraud_proof_end_to_end(ctx, k):
    """The malicious square (Q1 cell (k - 1, k) flipped, all roots recomputed) with Q3 withheld.  Checked on the
    CPU first: rows 0..k-1 are complete, so the oracle's pre-repair check names row k - 1 (root equal, parity
    not), and of that row exactly the cells in columns 0..k-1 are provable, their columns being complete
    (Q0 + Q2) while columns k.. miss their Q3 half."""
    from celestia_da import ByzantineDataError, rsmt2d, wrapper
    sq = ref.malicious_square(k)
    r, c = ref.flipped_cell(k)
    W = 2 * k
    present = np.ones((W, W), dtype=bool)
    present[k:, k:] = False
    held = sq.eds.copy()
    held[~present] = 0
    with pytest.raises(orepair.ErrByzantineData) as oe:
        orepair.repair(held, present, sq.rows, sq.cols)
    assert (oe.value.axis, oe.value.index) == (ref.ROW, r)
    assert ref.build(held, sq.rows, sq.cols, ref.ROW, r).positions.tolist() == list(range(k))

    eds = rsmt2d.new_extended_data_square_with_missing(sq.eds, present, rsmt2d.LeoRSCodec(ctx),
                                                      wrapper.new_constructor(k))
    with pytest.raises(ByzantineDataError) as ge:
        eds.repair(sq.rows, sq.cols, present)
    assert (ge.value.axis, ge.value.index) == (ref.ROW, r)
    proof = byzantine.build_bad_encoding_proof(eds.array(), sq.rows, sq.cols, ge.value.axis, ge.value.index, ctx=ctx)
    assert proof.positions.tolist() == list(range(k)) and (proof.proof_axes == ref.COL).all()
    assert byzantine.validate_bad_encoding_proofs([proof], [sq.dah()], ctx) == [None]
    assert ref.validate(proof, sq.rows, sq.cols)[0] == ref.VALID


def test_merged_samples_fill_a_short_builder_output(ctx):
    from celestia_da import proof as gpr
    k, W, index = 4, 8, 2
    sq = ref.honest_square(k)
    rs = gpr.ResidentSquare(pyref.random_namespaced_square(k), ctx)
    coords = np.array([(index, p, p % 2) for p in range(W)] + [(index + 1, 0, 0), (0, 0, 1)], dtype=np.int64)
    batch = rs.sample_proofs(coords)
    eds = sq.eds.copy()
    eds[0, :W - 2] = 0   # holes in columns 0..W-3: the builder proves two cells of row 2, fewer than k
    with pytest.raises(CdaError, match="2 provable shares of row 2, a fraud proof needs 4"):
        byzantine.build_bad_encoding_proof(eds, sq.rows, sq.cols, ref.ROW, index, ctx=ctx)
    proof = byzantine.build_bad_encoding_proof(eds, sq.rows, sq.cols, ref.ROW, index, samples=batch, ctx=ctx)
    assert proof.positions.tolist() == list(range(W))
    assert proof.proof_axes.tolist() == [0, 1, 0, 1, 0, 1, 1, 1]   # the builder's own two are orthogonal
    assert np.array_equal(proof.shares, sq.eds[index])
    assert ref.validate(proof, sq.rows, sq.cols)[0] == ref.ROOT_MATCHES
    assert byzantine.validate_bad_encoding_proofs([proof], [sq.dah()], ctx) == [byzantine.REASONS[3]]
    # a sample whose axis root is not the DAH's is not merged
    forged = batch.copy()
    forged.axis_roots[:, 60] ^= 1
    with pytest.raises(CdaError, match="a fraud proof needs 4"):
        byzantine.build_bad_encoding_proof(eds, sq.rows, sq.cols, ref.ROW, index, samples=forged, ctx=ctx)


# ---------------------------------------------------------------------- GF(2^16)
def test_gf16_square(ctx):
    """k = 256, the smallest width on GF(2^16): one malicious square, extended and hashed by the C oracle."""
    k = 256
    W = 2 * k
    r, c = ref.flipped_cell(k)
    eds = coracle.extend(coracle.random_square(k, 3)).reshape(W, W, 512).copy()
    eds[r, c, 100:104] ^= 0x5A
    rows, cols, _ = coracle.blind_dah(eds, k)
    full = byzantine.build_bad_encoding_proof(eds, rows, cols, ref.ROW, r, ctx=ctx)
    assert full.positions.tolist() == list(range(W))
    assert np.array_equal(full.shares, eds[r])
    half = ref.RefProof(k, ref.ROW, r, full.positions[1:k + 1].copy(), full.proof_axes[1:k + 1].copy(),
                        full.shares[1:k + 1].copy(), full.nmt_nodes[1:k + 1].copy())
    assert len(half) == k and c in half.positions.tolist()
    verdict, rebuilt = byzantine.verify_batch([full, half], [(rows, cols)] * 2, ctx)
    want = [ref.validate(p, rows, cols) for p in (full, half)]
    assert [w[0] for w in want] == [ref.VALID, ref.VALID]
    assert verdict.tolist() == [0, 0]
    assert [rebuilt[i].tobytes() for i in range(2)] == [w[1] for w in want]
    assert rebuilt[0].tobytes() != rows[r].tobytes() and rebuilt[1].tobytes() != rebuilt[0].tobytes()
