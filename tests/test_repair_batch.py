"""Batch repair (cda_repair_batch, cda_repair_batch_device, rsmt2d.repair_batch, sampling.assemble_batch).

Every square of a batch must come out as it does alone: the status, axis and index of oracle/repair.py's Repair, the
bytes of cda_repair_device on that square, and for a bad root input the oracle's text.  The squares of a batch have
different seeds, so different DAHs, and mix every outcome; the host plan behind the call is tested on the CPU in
tests/test_repair_batch_plan.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import befp_ref as ref
import coracle
from test_repair import block408_eds, device_repair, run_oracle, small_eds
from test_repair_batch_plan import deep_pattern

pytestmark = pytest.mark.gpu

OK, INVALID, BYZ, UNREP = 0, -6, -9, -10
I32P, U32P = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def code_of(outcome):
    return BYZ if isinstance(outcome, tuple) else {"ok": OK, "unrep": UNREP, "badroot": INVALID}[outcome]


def honest(k, seed, present):
    eds, rows, cols = small_eds(k, seed)
    return eds, present, rows, cols


def roots_bytes(rows):
    return np.frombuffer(b"".join(bytes(r) for r in rows), dtype=np.uint8)


class Batch:
    """Squares (eds, present, rows, cols) stacked for a batch call: absent cells zeroed, as a node holds them."""

    def __init__(self, cases):
        self.n = len(cases)
        self.W = cases[0][0].shape[0]
        self.held = np.stack([np.where(np.asarray(p, bool)[..., None], e, 0) for e, p, _, _ in cases]).astype(np.uint8)
        self.present = np.stack([np.asarray(p) for _, p, _, _ in cases]).astype(np.uint8)
        self.rows = np.stack([roots_bytes(r) for _, _, r, _ in cases])
        self.cols = np.stack([roots_bytes(c) for _, _, _, c in cases])

    def run(self, ctx, where="device", lo=0, hi=None):
        """(rc, status, axis, index, squares after the call, cda_last_error, device tensor or None) of squares
        [lo, hi) as one call."""
        from celestia_da._lib import ptr
        hi = self.n if hi is None else hi
        n = hi - lo
        status = np.full(n, 77, dtype=np.int32)
        axis = np.full(n, 77, dtype=np.int32)
        index = np.full(n, 77, dtype=np.uint32)
        args = (ptr(np.ascontiguousarray(self.present[lo:hi])), self.W, n, ptr(np.ascontiguousarray(self.rows[lo:hi])),
                ptr(np.ascontiguousarray(self.cols[lo:hi])), status.ctypes.data_as(I32P), axis.ctypes.data_as(I32P),
                index.ctypes.data_as(U32P))
        if where == "device":
            import torch
            d = torch.from_numpy(self.held[lo:hi].reshape(-1).copy()).to("cuda")
            rc = ctx.lib.cda_repair_batch_device(ctx.h, d.data_ptr(), *args)
            text = ctx.lib.cda_last_error(ctx.h).decode()
            out = d.cpu().numpy().reshape(n, self.W, self.W, 512)
        else:
            d = None
            out = self.held[lo:hi].copy()
            rc = ctx.lib.cda_repair_batch(ctx.h, ptr(out), *args)
            text = ctx.lib.cda_last_error(ctx.h).decode()
        return rc, status, axis, index, out, text, d


def check_against_single(ctx, cases, got, oracle=True):
    """Every square of the batch result `got` against the single-square device call and (oracle=True) the oracle."""
    rc, status, axis, index, out, text, _ = got
    assert rc == OK
    first = None
    for i, (eds, p, rows, cols) in enumerate(cases):
        info = {}
        single, _ = device_repair(ctx, eds, p, rows, cols, info)
        assert status[i] == code_of(single), (i, status[i], single)
        if oracle:
            oi = {}
            want, rep = run_oracle(eds, np.asarray(p, bool), rows, cols, oi)
            assert single == want, (i, single, want)
            if want == "ok":
                assert np.array_equal(out[i], rep), i
            if want == "badroot":
                assert info["error"] == oi["error"], i
        if isinstance(single, tuple):
            assert (axis[i], index[i]) == single[1:], (i, axis[i], index[i], single)
        else:
            assert axis[i] == -1, i
        held = np.asarray(p, bool)
        if single in ("ok", "unrep"):
            assert np.array_equal(out[i], info["square"]), i           # byte-equal to the square alone
        else:
            assert np.array_equal(out[i][held], eds[held]), i          # every input cell kept
        if first is None and single != "ok":
            first = (i, info.get("error") or {"unrep": "failed to solve data square"}.get(single) or
                     f"byzantine {'row' if single[1] == 0 else 'col'}: {single[2]}")
    assert text == ("" if first is None else f"square {first[0]}: {first[1]}")


# ------------------------------------------------------------------ honest squares
def honest_patterns(k):
    W = 2 * k
    full = np.ones((W, W), bool)
    q0 = full.copy()
    q0[:k, :k] = False
    rows_only = np.zeros((W, W), bool)
    rows_only[:k - 1] = True
    return [full, q0, np.random.default_rng(50 + k).random((W, W)) < 0.5, deep_pattern(k), rows_only,
            np.zeros((W, W), bool)]


@pytest.mark.parametrize("k", [2, 4, 8])
def test_honest_batch_matches_oracle_and_single(ctx, k):
    cases = [honest(k, 20 + i, p) for i, p in enumerate(honest_patterns(k))]
    assert len({c[2][0] for c in cases}) == 6    # six DAHs
    b = Batch(cases)
    for where in ("device", "host"):
        got = b.run(ctx, where)
        check_against_single(ctx, cases, got)
        assert got[1].tolist()[:2] == [OK, OK] and got[1].tolist()[4:] == [UNREP, UNREP]
        for i in (0, 1):
            assert np.array_equal(got[4][i], cases[i][0])


# ------------------------------------------------------------------ mixed outcomes
@functools.lru_cache(maxsize=None)
def decode_exposed(k):
    """test_repair_byzantine_matches_oracle's construction, the first trial the oracle calls byzantine."""
    eds, rows, cols = small_eds(k, 6)
    W = 2 * k
    rng = np.random.default_rng(2000 + k)
    for _ in range(8):
        bad = eds.copy()
        r, c = rng.integers(0, W, 2)
        bad[r, c, rng.integers(0, 512)] ^= 1 + rng.integers(0, 255)
        p = rng.random((W, W)) < 0.7
        p[r, c] = True
        p[r, (c + 1 + rng.integers(0, W - 1)) % W] = False
        p[(r + 1 + rng.integers(0, W - 1)) % W, c] = False
        if isinstance(run_oracle(bad, p, rows, cols)[0], tuple):
            return bad, p, rows, cols
    raise AssertionError("no byzantine trial")


def mixed_cases(k):
    """[0] honest, Q0 lost; [1] bad root input; [2] honest, random; [3] decode-exposed corruption; [4] honest, deep;
    [5] blind-committed unordered square, Q0 withheld; [6] maliciously committed square, two holes; [7] honest."""
    W = 2 * k
    full = np.ones((W, W), bool)
    q0 = full.copy()
    q0[:k, :k] = False
    e1, r1, c1 = small_eds(k, 31)
    bad = e1.copy()
    bad[1, 2, 77] ^= 0x40
    un, row = ref.unordered_square(k)
    mal = ref.malicious_square(k)
    holes = full.copy()
    holes[k - 1, 0] = holes[k, k] = False
    return [honest(k, 30, q0), (bad, full, r1, c1), honest(k, 32, np.random.default_rng(60 + k).random((W, W)) < 0.6),
            decode_exposed(k), honest(k, 34, deep_pattern(k)), (un.eds, q0, un.rows, un.cols),
            (mal.eds, holes, mal.rows, mal.cols), honest(k, 37, full)]


@pytest.mark.parametrize("k", [4, 8])
def test_mixed_outcomes_and_fraud_proofs(ctx, k):
    from celestia_da import byzantine
    cases = mixed_cases(k)
    b = Batch(cases)
    got = b.run(ctx, "device")
    check_against_single(ctx, cases, got)
    rc, status, axis, index, out, text, d = got
    assert status.tolist() == [OK, INVALID, status[2], BYZ, OK, BYZ, BYZ, OK] and status[2] in (OK, UNREP)
    assert (axis[5], index[5]) == (0, 0) and (axis[6], index[6]) == (0, k - 1)
    assert text.startswith("square 1: bad root input: row 1 expected ")
    for i in (0, 4, 7):
        assert np.array_equal(out[i], cases[i][0])
    host = b.run(ctx, "host")
    check_against_single(ctx, cases, host)
    # the fraud proofs of the two maliciously committed squares, from what the batch call left in HBM
    W = 2 * k
    for i in (5, 6):
        eds, p, rows, cols = cases[i]
        assert len(ref.build(b.held[i], rows, cols, int(axis[i]), int(index[i]))) >= k
        proof = byzantine.build_bad_encoding_proof(d.data_ptr() + i * W * W * 512, rows, cols, int(axis[i]),
                                                   int(index[i]), ctx=ctx)
        assert proof.k == k
        verdicts, _ = byzantine.verify_batch([proof], [(rows, cols)], ctx)
        assert verdicts.tolist() == [0], i
        assert ref.validate(proof, rows, cols)[0] == ref.VALID, i


# ------------------------------------------------------------------ field and kernel variants
def test_k32_through_the_host_entry(ctx):
    """GF(2^8) above the toy widths, block 408 among them."""
    k, W = 32, 64
    b408 = block408_eds()
    rng = np.random.default_rng(408)
    q0 = np.ones((W, W), bool)
    q0[:k, :k] = False
    cases = [honest(k, 41, rng.random((W, W)) < 0.5), (b408[0], q0, b408[1], b408[2]),
             honest(k, 42, rng.random((W, W)) < 0.55)]
    rc, status, axis, index, out, text, _ = Batch(cases).run(ctx, "host")
    assert rc == OK and status.tolist() == [OK, OK, OK] and axis.tolist() == [-1, -1, -1] and text == ""
    for i in range(3):
        assert np.array_equal(out[i], cases[i][0]), i


def test_k256_two_squares_against_the_single_call(ctx):
    """GF(2^16); two 128 MiB squares, Q0 lost."""
    from celestia_da import da, testfactory
    k, W = 256, 512
    q0 = np.ones((W, W), bool)
    q0[:k, :k] = False
    cases = []
    for seed in (1, 2):
        sq = da.extend_shares(testfactory.random_square(k, seed))
        dah = da.new_data_availability_header(sq)
        cases.append((sq.array().copy(), q0, dah.row_roots, dah.column_roots))
    got = Batch(cases).run(ctx, "device")
    check_against_single(ctx, cases, got, oracle=False)
    assert got[1].tolist() == [OK, OK]
    for i in range(2):
        assert np.array_equal(got[4][i], cases[i][0]), i


# ------------------------------------------------------------------ chunking and the call contract
def test_one_more_than_a_chunk(ctx):
    from celestia_da import rsmt2d
    k, W = 2, 4
    n = rsmt2d.repair_batch_chunk(W) + 1
    assert n == 257
    squares = [small_eds(k, 70 + s) for s in range(4)]
    rng = np.random.default_rng(71)
    cases = []
    for i in range(n):
        e, r, c = squares[i % 4]
        cases.append((e, rng.random((W, W)) < (0.35 + 0.1 * (i % 6)), r, c))
    for i in (3, n - 1):      # a bad root input in each chunk
        e, r, c = squares[i % 4]
        bad = e.copy()
        bad[0, 1, 300] ^= 1
        cases[i] = (bad, np.ones((W, W), bool), r, c)
    b = Batch(cases)
    whole = b.run(ctx, "device")
    lo = b.run(ctx, "device", 0, n // 2)
    hi = b.run(ctx, "device", n // 2, n)
    assert whole[0] == lo[0] == hi[0] == OK
    for f in (1, 2, 3, 4):
        assert np.array_equal(whole[f], np.concatenate([lo[f], hi[f]])), f
    assert whole[1][3] == whole[1][n - 1] == INVALID and {OK, UNREP} <= set(whole[1].tolist())
    # the message is the lowest-numbered failing square's, whatever its outcome
    for part in (whole, lo, hi):
        j = int(np.nonzero(part[1])[0][0])
        tail = "failed to solve data square" if part[1][j] == UNREP else "bad root input: row 0 expected "
        assert part[5].startswith(f"square {j}: {tail}"), part[5]
    assert whole[5] == lo[5]
    assert hi[1][n - 1 - n // 2] == INVALID
    # and square by square against the oracle, for the statuses
    for i in range(0, n, 16):
        e, p, r, c = cases[i]
        assert whole[1][i] == code_of(run_oracle(e, p, r, c)[0]), i


def test_call_contract(ctx):
    from celestia_da._lib import ptr
    assert ctx.lib.cda_repair_batch_device(ctx.h, None, None, 8, 0, None, None, None, None, None) == OK
    assert ctx.lib.cda_repair_batch(ctx.h, None, None, 8, 0, None, None, None, None, None) == OK
    k, W = 4, 8
    e, r, c = small_eds(k, 80)
    p = np.random.default_rng(80).random((W, W)) < 0.6
    one = Batch([(e, p, r, c)])
    for where in ("device", "host"):
        check_against_single(ctx, [(e, p, r, c)], one.run(ctx, where))
    # byz_axis / byz_index may be NULL
    held = one.held.copy()
    status = np.full(1, 77, dtype=np.int32)
    assert ctx.lib.cda_repair_batch(ctx.h, ptr(held), ptr(one.present), W, 1, ptr(one.rows), ptr(one.cols),
                                    status.ctypes.data_as(I32P), None, None) == OK
    assert status[0] == code_of(run_oracle(e, p, r, c)[0])
    # a width that is not a power of two: the call fails, the outputs are untouched
    for w in (6, 0, 2048):
        buf = np.zeros(max(w, 1) * max(w, 1) * 512, dtype=np.uint8)
        pres = np.ones(max(w, 1) * max(w, 1), dtype=np.uint8)
        roots = np.zeros(max(w, 1) * 90, dtype=np.uint8)
        status, axis, index = (np.full(1, 77, dtype=t) for t in (np.int32, np.int32, np.uint32))
        if w <= 8:
            rc = ctx.lib.cda_repair_batch(ctx.h, ptr(buf), ptr(pres), w, 1, ptr(roots), ptr(roots),
                                          status.ctypes.data_as(I32P), axis.ctypes.data_as(I32P),
                                          index.ctypes.data_as(U32P))
            assert rc == INVALID, w
        import torch
        d = torch.zeros(512, dtype=torch.uint8, device="cuda")
        rc = ctx.lib.cda_repair_batch_device(ctx.h, d.data_ptr(), ptr(pres), w, 1, ptr(roots), ptr(roots),
                                             status.ctypes.data_as(I32P), axis.ctypes.data_as(I32P),
                                             index.ctypes.data_as(U32P))
        assert rc == INVALID, w
        assert ctx.lib.cda_last_error(ctx.h).decode() == "EDS width must be a power of two in [2, 1024]"
        assert (status[0], axis[0], index[0]) == (77, 77, 77)


# ------------------------------------------------------------------ the Python mirror
def test_python_mirror_on_the_mixed_batch(ctx):
    from celestia_da import ByzantineDataError, rsmt2d
    k = 4
    cases = mixed_cases(k)
    b = Batch(cases)
    for where in ("host", "device"):
        if where == "host":
            eds = b.held.copy()
            outs = rsmt2d.repair_batch(eds, b.present, b.rows, b.cols, ctx)
        else:
            import torch
            d = torch.from_numpy(b.held.copy()).to("cuda")
            outs = rsmt2d.repair_batch_device(d, 2 * k, b.n, b.present, b.rows, b.cols, ctx)
            eds = d.cpu().numpy()
        assert len(outs) == b.n
        for i, (e, p, r, c) in enumerate(cases):
            oi = {}
            want, rep = run_oracle(e, np.asarray(p, bool), r, c, oi)
            o = outs[i]
            assert o.code == code_of(want), (where, i)
            assert (o.ok, o.byzantine, o.unrepairable, o.bad_root) == \
                (want == "ok", isinstance(want, tuple), want == "unrep", want == "badroot")
            if want == "ok":
                assert np.array_equal(eds[i], rep) and o.error() is None
            elif want == "badroot":
                assert o.message == oi["error"]
            elif isinstance(want, tuple):
                assert (o.axis, o.index) == want[1:] and isinstance(o.error(), ByzantineDataError)
    # a second bad root input, not the batch's first failure, still carries its own text
    two = Batch([cases[1], cases[0], cases[1]])
    eds = two.held.copy()
    outs = rsmt2d.repair_batch(eds, two.present, two.rows, two.cols, ctx)
    assert [o.code for o in outs] == [INVALID, OK, INVALID] and outs[2].message == outs[0].message != ""
    assert rsmt2d.repair_batch(np.zeros((0, 8, 8, 512), np.uint8), np.zeros((0, 8, 8)), np.zeros((0, 8, 90)),
                               np.zeros((0, 8, 90)), ctx) == []


def test_samples_of_two_heights_to_one_repair(ctx):
    """Two k = 4 squares, each from 60 % of its cells sampled and verified: assemble_batch -> repair_batch."""
    from celestia_da import proof as gpr
    from celestia_da import rsmt2d, sampling
    k, W = 4, 8
    batches, verdicts, want, rows, cols = [], [], [], [], []
    for h in range(2):
        sq = gpr.ResidentSquare(coracle.random_square(k, 90 + h), ctx)
        rng = np.random.default_rng(90 + h)
        cells = rng.permutation(W * W)[: int(0.6 * W * W)]
        coords = np.stack([cells // W, cells % W, rng.integers(0, 2, cells.size)], axis=1)
        batch = sq.sample_proofs(coords).copy()
        if h == 1:
            batch.shares[0, 99] ^= 1          # one answer tampered: its cell stays absent
        r, c, root = sq.dah()
        v = sampling.verify_samples(batch, root, ctx)
        assert v.tolist() == [2 * (h == 1)] + [0] * (cells.size - 1)
        batches.append(batch)
        verdicts.append(v)
        want.append(sq.eds().copy())
        rows.append(r)
        cols.append(c)
        sq.close()
    eds, present = sampling.assemble_batch(batches, verdicts)
    assert eds.shape == (2, W, W, 512) and present.sum(axis=(1, 2)).tolist() == [38, 37]
    single = [sampling.assemble(b, v) for b, v in zip(batches, verdicts)]
    assert all(np.array_equal(eds[i], single[i][0]) and np.array_equal(present[i], single[i][1]) for i in range(2))
    outs = rsmt2d.repair_batch(eds, present, np.stack([roots_bytes(r) for r in rows]),
                               np.stack([roots_bytes(c) for c in cols]), ctx)
    for i in range(2):
        assert run_oracle(want[i], present[i].astype(bool), rows[i], cols[i])[0] == "ok"
        assert outs[i].ok and np.array_equal(eds[i], want[i]), i
    with pytest.raises(ValueError):
        sampling.assemble_batch(batches, verdicts[:1])
