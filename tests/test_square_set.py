"""Sets of resident squares (cda_square_set_*): n squares built in one
submission from a host or device batch of ODSs or EDSs, every member a
cda_square that answers what a singly created square answers, and samples of
many members from one launch (cda_square_set_sample_proofs).

The yardstick is the code that exists: a square created with cda_square_create
from the same ODS gives the same bytes, no tolerance.  For k <= 4 the samples
are also checked against test_sampling's CPU Checker and the data roots against
the C oracle.  The singles of a case are created once per (k, seeds) and shared.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import coracle
import pyref
from celestia_da import CdaError, _lib, malicious, testfactory
from celestia_da._lib import CDA_ERR_INVALID, CDA_ERR_PUSH_ORDER, CDA_OK, ptr
from nmt_edge_squares import first_violation
from test_sampling import Checker, all_cells

pytestmark = pytest.mark.gpu

U32P, I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
KN = [(1, 1), (1, 5), (2, 3), (4, 5), (8, 3), (32, 3), (128, 2), (256, 2)]


def log2(x):
    return x.bit_length() - 1


def seeds_of(k, n):
    return [7000 + 16 * k + i for i in range(n)]


def ods_batch(k, n):
    return np.stack([coracle.random_square(k, s) for s in seeds_of(k, n)])


def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_singles = {}


@pytest.fixture(scope="module")
def singles(ctx):
    """ResidentSquare of ods_batch(k, n)[i], created singly, once per module."""
    from celestia_da import proof as gpr

    def get(k, n):
        ods = ods_batch(k, n)
        for i, s in enumerate(seeds_of(k, n)):
            if (k, s) not in _singles:
                _singles[k, s] = gpr.ResidentSquare(ods[i], ctx)
        return [_singles[k, s] for s in seeds_of(k, n)]
    yield get
    for sq in _singles.values():
        sq.close()
    _singles.clear()


def outcome(fn):
    """What a call answers, comparable: its arrays as bytes, or its error code and text."""
    try:
        r = fn()
    except CdaError as e:
        return ("error", e.code, str(e))
    if hasattr(r, "arrays"):
        return tuple(np.ascontiguousarray(a).tobytes() for a in r.arrays())
    return r


def sample_coords(k, seed):
    if k <= 4:
        return all_cells(k)
    rng = np.random.default_rng(seed)
    W = 2 * k
    return np.stack([rng.integers(0, W, 256), rng.integers(0, W, 256), rng.integers(0, 2, 256)], axis=1)


def answers(sq, k, seed):
    """Every query of the issue's list on one square, as comparable values."""
    rng = np.random.default_rng(seed)
    n_sh = k * k
    cuts = sorted(set(rng.integers(0, n_sh + 1, 8).tolist()) | {0, n_sh})
    ranges = [(a, b) for a, b in zip(cuts, cuts[1:])]
    eds = sq.eds()
    nss = [eds[0, 0, :29].tobytes(), eds[k - 1, k - 1, :29].tobytes(), bytes(28) + b"\x02"]
    starts = sorted(set(rng.integers(0, n_sh, 3).tolist()))
    lens = [max(1, min(5, n_sh - s)) for s in starts]
    walk = [bool(b) for b in rng.integers(0, 2, int(rng.integers(0, log2(2 * k) + 1)))]
    return {
        "samples": outcome(lambda: sq.sample_proofs(sample_coords(k, seed))),
        "share_proofs": outcome(lambda: sq.share_proofs_batch(ranges)),
        "namespace_proofs": outcome(lambda: sq.namespace_proofs(nss)),
        "commitment_proofs": outcome(lambda: sq.commitment_proofs(starts, lens)),
        "subtree_root": outcome(lambda: sq.subtree_root(int(rng.integers(0, 2 * k)), walk)),
        "parse": outcome(lambda: sq.parse()),
        "eds": eds.tobytes(),
    }


def assert_members_equal(sqset, single_squares, k):
    rows, cols, roots = sqset.dah()
    for i, single in enumerate(single_squares):
        r, c, d = single.dah()
        assert rows[i].tobytes() == b"".join(r) and cols[i].tobytes() == b"".join(c), ("roots", i)
        assert roots[i].tobytes() == d, ("data root", i)
        got, want = answers(sqset[i], k, 31 + i), answers(single, k, 31 + i)
        for name in want:
            assert got[name] == want[name], (name, "square", i)
        assert not isinstance(want["samples"], tuple) or want["samples"][0] != "error"
        assert sqset[i].dah() == (r, c, d)


# ----------------------------------------------------------- 1. equality with single squares
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,n", KN)
def test_set_equals_single_squares(ctx, singles, k, n, where):
    from celestia_da import proof as gpr
    ods = ods_batch(k, n)
    if where == "host":
        sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    else:
        d_ods = device(ods)
        sqset = gpr.ResidentSquareSet.from_device_ods(d_ods, k, n, ctx=ctx)
        assert np.array_equal(d_ods.cpu().numpy(), ods), "the device source changed"
        del d_ods   # may be released on return
    try:
        assert len(sqset) == n and sqset.k == k and sqset.status.tolist() == [0] * n and not sqset.push_order_error
        assert_members_equal(sqset, singles(k, n), k)
        if k <= 4:
            _, _, roots = sqset.dah()
            for i, s in enumerate(seeds_of(k, n)):
                ch = Checker(k, s)
                assert roots[i].tobytes() == ch.root == coracle.extend_dah(ods[i])[3]
                coords = all_cells(k)
                got = sqset.sample_proofs(np.concatenate([np.full((len(coords), 1), i), coords], axis=1))
                for name, a, b in zip(("shares", "namespaces", "nmt_nodes", "axis_roots", "leaf_hash", "aunts"),
                                      got.batch.arrays(), ch.arrays(coords)):
                    assert np.array_equal(a, b), (name, "square", i)
    finally:
        sqset.close()


def test_members_parse_constructed_squares(ctx):
    """coracle.random_square's shares are no transactions (cda_square_parse answers the same error on member and
    single square above); squares that square.Construct built parse, member and single alike."""
    from celestia_da import blobfactory, proof as gpr, square as gsq
    blocks = [blobfactory.random_block(42 + s, 3, 6, (1, 2), (1, 5000)) for s in range(3)]
    ods = [np.frombuffer(gsq.construct(b, 16, 64, ctx=ctx).to_bytes(), dtype=np.uint8) for b in blocks]
    assert len({o.size for o in ods}) == 1
    sqset = gpr.ResidentSquareSet.from_ods(np.stack(ods), ctx)
    try:
        for i, o in enumerate(ods):
            single = gpr.ResidentSquare(o, ctx)
            want = single.parse()
            assert want.txs and want.blobs and sqset[i].parse() == want, i
            k = sqset.k
            ranges = [(0, k), (k, k * k)]
            assert outcome(lambda: sqset[i].parse(ranges)) == outcome(lambda: single.parse(ranges))
            assert sqset[i].parse_plan() == single.parse_plan()
            single.close()
    finally:
        sqset.close()


# ----------------------------------------------------------- 2. from an EDS
@pytest.mark.parametrize("k,n", [(2, 3), (8, 3), (32, 3)])
def test_set_from_eds(ctx, singles, k, n):
    from celestia_da import proof as gpr
    W = 2 * k
    eds = np.stack([s.eds() for s in singles(k, n)])
    for where in ("host", "device"):
        if where == "host":
            sqset = gpr.ResidentSquareSet.from_eds(eds, ctx)
        else:
            d = device(eds)
            sqset = gpr.ResidentSquareSet.from_device_eds(d, k, n, ctx=ctx)
            assert np.array_equal(d.cpu().numpy(), eds)
            del d
        try:
            assert_members_equal(sqset, singles(k, n), k)
        finally:
            sqset.close()
    # one byte of one parity cell of square 1: hashed as given, nothing re-extended
    bad = eds.copy()
    bad[1, W - 1, k, 77] ^= 0x40
    sqset = gpr.ResidentSquareSet.from_eds(bad, ctx)
    try:
        rows, cols, roots = sqset.dah()
        assert np.array_equal(sqset[1].eds(), bad[1])
        r, c, d = (np.empty(W * 90, np.uint8), np.empty(W * 90, np.uint8), np.empty(32, np.uint8))
        ctx.check(ctx.lib.cda_dah_from_eds(ctx.h, ptr(np.ascontiguousarray(bad[1])), W, ptr(r), ptr(c), ptr(d)))
        assert rows[1].tobytes() == r.tobytes() and cols[1].tobytes() == c.tobytes() and roots[1].tobytes() == d.tobytes()
        for i, single in enumerate(singles(k, n)):
            sr, sc, sd = single.dah()
            same = rows[i].tobytes() == b"".join(sr) and cols[i].tobytes() == b"".join(sc) and roots[i].tobytes() == sd
            assert same == (i != 1), i
    finally:
        sqset.close()


# ----------------------------------------------------------- 3. cross-square samples
def call_set_samples(ctx, sqset, req, want_out=(True,) * 6, fill=0xA5):
    """cda_square_set_sample_proofs of req = (n, 4) (square, row, col, axis): (rc, the six arrays or None)."""
    k, n = sqset.k, len(req)
    D = log2(2 * k)
    sizes = (512, 29, D * 90, 90, 32, (D + 1) * 32)
    out = [np.full(max(1, n) * s, fill, dtype=np.uint8) if w else None for s, w in zip(sizes, want_out)]
    sq, r, c = (np.ascontiguousarray(req[:, j], dtype=np.uint32) for j in range(3))
    ax = np.ascontiguousarray(req[:, 3], dtype=np.uint8)
    rc = ctx.lib.cda_square_set_sample_proofs(sqset.h, sq.ctypes.data_as(U32P), r.ctypes.data_as(U32P),
                                              c.ctypes.data_as(U32P), ptr(ax), n, *(ptr(a) for a in out))
    return rc, [None if a is None else a[:n * s].reshape(n, s) for a, s in zip(out, sizes)]


def per_member(sqset, req):
    """The six arrays from one cda_square_sample_proofs call per member, gathered in request order."""
    k, n = sqset.k, len(req)
    D = log2(2 * k)
    sizes = (512, 29, D * 90, 90, 32, (D + 1) * 32)
    out = [np.zeros((n, s), dtype=np.uint8) for s in sizes]
    for y in np.unique(req[:, 0]).tolist():
        pick = np.nonzero(req[:, 0] == y)[0]
        b = sqset[y].sample_proofs(req[pick, 1:])
        for dst, a in zip(out, b.arrays()):
            dst[pick] = a.reshape(len(pick), -1)
    return out


@pytest.fixture(scope="module")
def sample_sets(ctx):
    from celestia_da import proof as gpr
    made = {}

    def get(k, n):
        if (k, n) not in made:
            made[k, n] = gpr.ResidentSquareSet.from_ods(ods_batch(k, n), ctx)
        return made[k, n]
    yield get
    for s in made.values():
        s.close()


def requests(k, n, count, seed):
    rng = np.random.default_rng(seed)
    W = 2 * k
    return np.stack([rng.integers(0, n, count), rng.integers(0, W, count), rng.integers(0, W, count),
                     rng.integers(0, 2, count)], axis=1).astype(np.int64)


@pytest.mark.parametrize("k,n", [(4, 5), (32, 3)])
def test_cross_square_samples(ctx, sample_sets, k, n):
    from celestia_da import sampling
    sqset = sample_sets(k, n)
    req = requests(k, n, 4096, 5 * k + n)
    assert len(np.unique(req[:64, 0])) == n, "squares interleave in request order"
    rc, got = call_set_samples(ctx, sqset, req)
    assert rc == CDA_OK
    want = per_member(sqset, req)
    for name, a, b in zip(("shares", "namespaces", "nmt_nodes", "axis_roots", "leaf_hash", "aunts"), got, want):
        assert np.array_equal(a, b), name
    _, _, roots = sqset.dah()
    D = log2(2 * k)
    batch = sampling.SampleBatch(k, req[:, 1:], got[0], got[1], got[2].reshape(-1, D, 90), got[3], got[4],
                                 got[5].reshape(-1, D + 1, 32))
    verdicts = sampling.verify_samples(batch, roots[req[:, 0]], ctx)
    assert not verdicts.any()
    wrong = sampling.verify_samples(batch, roots[(req[:, 0] + 1) % n], ctx)
    assert (wrong == 1).all(), "a sample verifies only against its own square's data root"


@pytest.mark.parametrize("k,n", [(4, 5), (32, 3)])
def test_cross_square_samples_null_outputs_and_edges(ctx, sample_sets, k, n):
    sqset = sample_sets(k, n)
    req = requests(k, n, 37, 99)   # 37: no multiple of the four samples of a workgroup
    rc, full = call_set_samples(ctx, sqset, req)
    assert rc == CDA_OK
    want = per_member(sqset, req)
    for a, b in zip(full, want):
        assert np.array_equal(a, b)
    for mask in range(63):   # every combination with at least one output NULL
        keep = tuple(bool(mask >> j & 1) for j in range(6))
        rc, got = call_set_samples(ctx, sqset, req, keep)
        assert rc == CDA_OK, mask
        for j in range(6):
            assert (got[j] is None) == (not keep[j])
            assert got[j] is None or np.array_equal(got[j], full[j]), (mask, j)
    for count in (1, 2, 3, 5):
        rc, got = call_set_samples(ctx, sqset, req[:count])
        assert rc == CDA_OK and all(np.array_equal(a, b[:count]) for a, b in zip(got, full))
    # n == 0: CDA_OK, nothing written
    rc, got = call_set_samples(ctx, sqset, req[:0])
    assert rc == CDA_OK
    # all requests on one square
    one = req.copy()
    one[:, 0] = n - 1
    rc, got = call_set_samples(ctx, sqset, one)
    assert rc == CDA_OK
    b = sqset[n - 1].sample_proofs(one[:, 1:])
    for a, e in zip(got, b.arrays()):
        assert np.array_equal(a, e.reshape(len(one), -1))


def test_cross_square_samples_validation(ctx, sample_sets):
    k, n = 4, 5
    sqset = sample_sets(k, n)
    req = requests(k, n, 9, 3)
    for field, col, value in (("square", 0, n), ("row", 1, 2 * k), ("col", 2, 2 * k), ("axis", 3, 2)):
        bad = req.copy()
        bad[6, col] = value
        rc, got = call_set_samples(ctx, sqset, bad, fill=0x5C)
        assert rc == CDA_ERR_INVALID
        msg = ctx.lib.cda_last_error(ctx.h).decode()
        assert msg.startswith(f"sample 6: {field} {value} "), msg
        assert all((a == 0x5C).all() for a in got), "outputs untouched"


# ----------------------------------------------------------- 4. offsets past 2^32
def test_offsets_past_4gib(ctx):
    import torch
    from celestia_da import proof as gpr
    k, n, period = 128, 130, 3
    three = np.stack([coracle.random_square(k, 4100 + i) for i in range(period)])
    d_three = device(three)
    d_ods = d_three[torch.arange(n, device="cuda") % period].contiguous()
    assert d_ods.numel() == n * k * k * 512
    sqset = gpr.ResidentSquareSet.from_device_ods(d_ods, k, n, ctx=ctx)
    del d_ods
    ones = [gpr.ResidentSquare(three[i], ctx) for i in range(period)]
    try:
        assert n * (2 * k) ** 2 * 512 > 1 << 32
        _, _, roots = sqset.dah()
        want = [s.dah()[2] for s in ones]
        assert len(set(want)) == period
        assert [roots[i].tobytes() for i in range(n)] == [want[i % period] for i in range(n)]
        coords = sample_coords(k, 17)
        for y in (0, 1, 128, 129):
            exp = ones[y % period].sample_proofs(coords)
            got = sqset.sample_proofs(np.concatenate([np.full((len(coords), 1), y), coords], axis=1))
            member = sqset[y].sample_proofs(coords)
            for a, b, c in zip(got.batch.arrays(), exp.arrays(), member.arrays()):
                assert np.array_equal(a, b) and np.array_equal(c, b), y
    finally:
        for s in ones:
            s.close()
        sqset.close()


# ----------------------------------------------------------- 5. push order
def _unordered_square(k, seed):
    """As tests/test_malicious.py builds its squares."""
    ods = testfactory.random_square(k, seed).reshape(k, k, 512).copy()
    ods[1, [0, 3]] = ods[1, [3, 0]]                # row 1 and columns 0 / 3 out of order
    return ods


@pytest.mark.parametrize("where", ["host", "device"])
def test_push_order_per_square(ctx, where):
    k, n, bad = 4, 5, (1, 4)
    ods = np.stack([testfactory.random_square(k, 60 + i).reshape(k, k, 512) for i in range(n)])
    for i in bad:
        ods[i] = _unordered_square(k, 60 + i)
    h = C.c_void_p()
    if where == "host":
        rc = ctx.lib.cda_square_set_create(ctx.h, ptr(np.ascontiguousarray(ods)), _lib.CDA_SET_FROM_ODS, k, n,
                                           C.byref(h))
    else:
        d = device(ods)
        rc = ctx.lib.cda_square_set_create_device(ctx.h, d.data_ptr(), _lib.CDA_SET_FROM_ODS, k, n, None, C.byref(h))
    assert rc == CDA_ERR_PUSH_ORDER and h.value, "the set is still returned"
    try:
        msg = ctx.lib.cda_last_error(ctx.h).decode()
        with pytest.raises(pyref.PushOrderError) as first:
            pyref.dah_from_eds(pyref.extend_square(ods[bad[0]]))
        assert msg == str(first.value)
        for i in range(n):
            v = first_violation(ods[i])
            assert ctx.push_order_detail_at(i) == (v if v is not None else (-1, 0, 0)), i
            assert (v is not None) == (i in bad)
        W = 2 * k
        rows, cols, roots = (np.empty(n * W * 90, np.uint8), np.empty(n * W * 90, np.uint8), np.empty(n * 32, np.uint8))
        status = np.full(n, 99, dtype=np.int32)
        ctx.check(ctx.lib.cda_square_set_dah(h, ptr(rows), ptr(cols), ptr(roots), status.ctypes.data_as(I32P)))
        assert status.tolist() == [0, -3, 0, 0, -3]
        for i in range(n):
            _, dah = malicious.extend_shares_dah(list(ods[i].reshape(k * k, 512)))
            assert rows[i * W * 90:(i + 1) * W * 90].tobytes() == b"".join(dah.row_roots), i
            assert cols[i * W * 90:(i + 1) * W * 90].tobytes() == b"".join(dah.column_roots), i
            assert roots[32 * i:32 * (i + 1)].tobytes() == dah.hash(), i
            if i not in bad:
                assert dah.hash() == coracle.extend_dah(ods[i])[3]
        # the unordered squares still serve samples, equal to the blind trees' proofs
        from celestia_da import proof as gpr, sampling
        sqset = gpr.ResidentSquareSet(ctx, h, rc)
        h = None
        coords = all_cells(k)
        for i in bad:
            req = np.concatenate([np.full((len(coords), 1), i), coords], axis=1)
            got = sqset.sample_proofs(req)
            assert not sampling.verify_samples(got.batch, roots[32 * i:32 * (i + 1)], ctx).any()
            assert sqset[i].push_order_error and not sqset[0].push_order_error
        sqset.close()
    finally:
        if h:
            ctx.lib.cda_square_set_destroy(h)


# ----------------------------------------------------------- 6. lifecycle
def test_member_destroy_is_refused(ctx, sample_sets):
    sqset = sample_sets(4, 5)
    m = C.c_void_p()
    assert ctx.lib.cda_square_set_at(sqset.h, 2, C.byref(m)) == CDA_OK and m.value
    before = sqset[2].sample_proofs(all_cells(4))
    assert ctx.lib.cda_square_destroy(m) == CDA_ERR_INVALID
    assert "cda_square_set" in ctx.lib.cda_last_error(ctx.h).decode()
    after = sqset[2].sample_proofs(all_cells(4))
    assert all(np.array_equal(a, b) for a, b in zip(before.arrays(), after.arrays()))
    assert ctx.lib.cda_square_set_at(sqset.h, 5, C.byref(m)) == CDA_ERR_INVALID and not m.value
    k, n = C.c_uint32(), C.c_uint32()
    assert ctx.lib.cda_square_set_info(sqset.h, C.byref(k), C.byref(n)) == CDA_OK and (k.value, n.value) == (4, 5)


def test_sets_release_their_memory(ctx):
    import torch
    from celestia_da import proof as gpr
    k, n = 128, 8
    d_ods = device(ods_batch(k, 2)[np.arange(n) % 2])
    coords = sample_coords(k, 3)

    def round_trip():
        s = gpr.ResidentSquareSet.from_device_ods(d_ods, k, n, ctx=ctx)
        s.sample_proofs(np.concatenate([np.full((len(coords), 1), n - 1), coords], axis=1))
        s[0].sample_proofs(coords)
        s.close()

    round_trip()                       # first-use allocations (pools, context scratch)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        round_trip()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 128 << 20, f"{(free0 - free1) >> 20} MiB kept after 3 sets"


def test_failed_create_leaves_nothing(ctx):
    import torch
    k, n = 8, 3
    ods = np.ascontiguousarray(ods_batch(k, n))
    d = device(ods)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    cases = [
        lambda h: ctx.lib.cda_square_set_create(ctx.h, None, 0, k, n, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create(ctx.h, ptr(ods), 2, k, n, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create(ctx.h, ptr(ods), 0, k, 0, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create(ctx.h, ptr(ods), 0, 3, n, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create(ctx.h, ptr(ods), 0, 2048, n, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create_device(ctx.h, None, 1, k, n, None, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create_device(ctx.h, d.data_ptr(), -1, k, n, None, C.byref(h)),
        lambda h: ctx.lib.cda_square_set_create_device(ctx.h, d.data_ptr(), 0, 0, n, None, C.byref(h)),
    ]
    for i, call in enumerate(cases):
        h = C.c_void_p(0xDEAD)
        assert call(h) == CDA_ERR_INVALID, i
        assert not h.value, i
        assert ctx.lib.cda_last_error(ctx.h).decode(), i
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free0 - free1) < 1 << 20


def test_python_member_keeps_its_set_alive(ctx):
    from celestia_da import proof as gpr
    k, n = 4, 5
    sqset = gpr.ResidentSquareSet.from_ods(ods_batch(k, n), ctx)
    want = sqset[3].sample_proofs(all_cells(k))
    member = sqset[3]
    del sqset
    gc.collect()
    got = member.sample_proofs(all_cells(k))
    assert all(np.array_equal(a, b) for a, b in zip(got.arrays(), want.arrays()))
    owner = member.owner
    member.close()
    assert owner.h, "closing a member leaves the set"
    # closing the set ends the members it handed out
    member = owner[1]
    owner.close()
    assert member.h is None


# ----------------------------------------------------------- 8. end to end (Python)
def test_end_to_end_sample_repair_serve(ctx):
    from celestia_da import proof as gpr, rsmt2d, sampling
    k, n = 8, 4
    W = 2 * k
    ods = ods_batch(k, n)
    served = gpr.ResidentSquareSet.from_ods(ods, ctx)
    rows, cols, roots = served.dah()
    # a light node samples three quadrants' worth of every square, squares grouped
    rng = np.random.default_rng(8)
    cells = [(y, r, c, int(rng.integers(0, 2))) for y in range(n) for r in range(W) for c in range(W)
             if not (r >= k and c >= k)]
    got = served.sample_proofs(np.array(cells, dtype=np.int64))
    verdicts = sampling.verify_samples(got.batch, got.data_roots(roots), ctx)
    assert not verdicts.any()
    parts = got.by_square(verdicts)
    assert [y for y, _, _ in parts] == list(range(n))
    assert all(np.shares_memory(b.shares, got.batch.shares) for _, b, _ in parts), "views, not copies"
    eds, present = sampling.assemble_batch([b for _, b, _ in parts], [v for _, _, v in parts])
    d_eds = device(eds)
    outcomes = rsmt2d.repair_batch_device(d_eds, W, n, present, rows.reshape(n, -1), cols.reshape(n, -1), ctx=ctx)
    assert all(o.ok for o in outcomes), outcomes
    # the repaired squares become resident without leaving the device
    caught_up = gpr.ResidentSquareSet.from_device_eds(d_eds, k, n, ctx=ctx)
    del d_eds
    assert np.array_equal(caught_up.dah()[2], roots)
    again = sampling.sample_proofs_set(caught_up, requests(k, n, 300, 1))
    assert not sampling.verify_samples(again.batch, again.data_roots(roots), ctx).any()
    assert len(again.by_square()) == n   # interleaved requests: gathered per square
    served.close()
    caught_up.close()


def test_replay_keeps_resident_sets(ctx):
    from celestia_da import blobfactory, replay, sampling
    # six seeded blocks of two square sizes
    blocks = [blobfactory.random_block(41 + s, 3, 6, (1, 2), (1, 5000)) for s in range(3)] + \
             [blobfactory.random_block(50 + s, 1, 1, (1, 1), (1, 300)) for s in range(3)]
    plain = replay.replay(blocks, max_square_size=16, ctx=ctx)
    results, kept = replay.replay(blocks, max_square_size=16, ctx=ctx, keep=True)
    assert [(r.square_size, r.data_root, r.error) for r in results] == \
        [(r.square_size, r.data_root, r.error) for r in plain]
    sizes = {r.square_size for r in results if r.square_size}
    assert len(sizes) == 2 and set(kept) == sizes, sizes
    seen = []
    for k, batches in kept.items():
        for kb in batches:
            _, _, roots = kb.squares.dah()
            for j, i in enumerate(kb.blocks):
                assert results[i].square_size == k
                if results[i].error is None:
                    assert roots[j].tobytes() == results[i].data_root
                seen.append(i)
            s = sampling.sample_proofs_set(kb.squares, requests(k, len(kb.blocks), 64, k))
            ok = [results[kb.blocks[y]].error is None for y in s.squares.tolist()]
            v = sampling.verify_samples(s.batch, s.data_roots(roots), ctx)
            assert not v[np.array(ok)].any()
            kb.squares.close()
    assert sorted(seen) == [i for i, r in enumerate(results) if r.square_size]
