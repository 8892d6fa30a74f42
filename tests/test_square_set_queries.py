"""Namespace and share-range proofs across a set of resident squares:
cda_square_set_namespace_plan / _namespace_proofs / _share_proofs and
cda_namespace_proofs_verify_set, with their Python faces.

Two yardsticks, no tolerance anywhere: the single-square calls on sqset[i] and
on singly created squares (which the existing suite pins to the restatement and
the oracle), and for k <= 8 tests/nmt_namespace_ref.py directly.
"""
import ctypes as C

import numpy as np
import pytest

import coracle
import nmt_namespace_ref as ref
from celestia_da import PushOrderError, _lib, testfactory
from celestia_da._lib import CDA_ERR_INVALID, CDA_ERR_PUSH_ORDER, CDA_OK, ptr
from celestia_da.namespace import NamespaceProofsBatch, SetNamespaceProofs, split_set_queries
from celestia_da.proof import ShareProofsBatch
from test_namespace_proofs import assert_batch_equals, assert_plan_equals, run_square
from test_square_set import _unordered_square, device

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)
KN = {1: 5, 2: 3, 4: 5, 8: 3}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def p32(a):
    return a.ctypes.data_as(U32P)


def member_ods(k):
    """The ref squares of width k, then coracle.random_square seeds, KN[k] in all."""
    out = [ref.squares()[f"small{k}"].ods] + ([ref.squares()["hand"].ods] if k == 2 else [])
    out += [np.asarray(coracle.random_square(k, 8800 + 16 * k + i)).reshape(-1, 512) for i in range(KN[k] - len(out))]
    return out


@pytest.fixture(scope="module")
def sets(ctx):
    """k -> (the set, a RefSquare per member, a singly created ResidentSquare per member), made once."""
    from celestia_da import proof as gpr
    made = {}

    def get(k):
        if k not in made:
            ods = member_ods(k)
            refs = [ref.squares()[f"small{k}"]] + ([ref.squares()["hand"]] if k == 2 else [])
            refs += [ref.RefSquare(o) for o in ods[len(refs):]]
            made[k] = (gpr.ResidentSquareSet.from_ods(np.stack(ods), ctx), refs, [gpr.ResidentSquare(o, ctx) for o in ods])
        return made[k]
    yield get
    for sqset, _, singles in made.values():
        for s in singles:
            s.close()
        sqset.close()


_answers = {}


def ref_answer(r, ns):
    if (id(r), ns) not in _answers:
        _answers[id(r), ns] = (r, ref.get_shares_by_namespace(r, ns))   # r kept: its id is not reused
    return _answers[id(r), ns][1]


def interleave(per_member):
    """[(member, item)] round robin over the members' lists."""
    out = []
    for j in range(max(len(x) for x in per_member)):
        out += [(y, x[j]) for y, x in enumerate(per_member) if j < len(x)]
    return out


def plain(answers):
    return [[(r, p.start, p.end, list(p.nodes), p.leaf_hash, list(sh)) for r, p, sh in a] for a in answers]


def share_pieces(b):
    """One comparable value per proof of a ShareProofsBatch: every array cut by the offsets, the offsets rebased."""
    so, no, ao = b.seg_off.tolist(), b.node_off.tolist(), b.aunt_off.tolist()
    assert so[0] == no[0] == ao[0] == 0 and so[-1] == len(b.nmt_start) == len(b.row_roots)
    assert no[-1] == len(b.nodes) and ao[-1] == len(b.aunts)
    out, at = [], 0
    for i in range(len(b)):
        g0, g1 = so[i], so[i + 1]
        n_sh = int((b.nmt_end[g0:g1] - b.nmt_start[g0:g1]).sum())
        out.append((b.nmt_start[g0:g1].tobytes(), b.nmt_end[g0:g1].tobytes(), (b.node_off[g0:g1 + 1] - no[g0]).tobytes(),
                    b.nodes[no[g0]:no[g1]].tobytes(), b.row_roots[g0:g1].tobytes(), b.rfc_total[g0:g1].tobytes(),
                    b.rfc_index[g0:g1].tobytes(), b.rfc_leaf_hash[g0:g1].tobytes(),
                    (b.aunt_off[g0:g1 + 1] - ao[g0]).tobytes(), b.aunts[ao[g0]:ao[g1]].tobytes(),
                    b.shares[at:at + n_sh].tobytes(), b.namespaces[i].tobytes(), int(b.start_row[i]),
                    int(b.end_row[i]), int(b.one_namespace[i])))
        at += n_sh
    assert at == len(b.shares)
    return out


def ranges_of(k, seed):
    """Every range of a random cut list, single shares, whole rows and the whole ODS."""
    rng = np.random.default_rng(seed)
    n_sh = k * k
    cuts = sorted(set(rng.integers(0, n_sh + 1, 6).tolist()) | {0, n_sh})
    out = [(a, b) for a, b in zip(cuts, cuts[1:])]
    out += [(s, s + 1) for s in sorted(set(rng.integers(0, n_sh, 4).tolist()) | {0, n_sh - 1})]
    out += [(r * k, (r + 1) * k) for r in range(k)] + [(0, n_sh)]
    return out


def assert_ranges_equal_members(sqset, squares_of, req):
    """The set's answer to req = [(square, (start, end))] against share_proofs_batch of each named square."""
    got = sqset.share_proofs_batch([(y, s, e) for y, (s, e) in req])
    assert got.squares.tolist() == [y for y, _ in req]
    pieces = share_pieces(got.batch)
    for y in sorted({y for y, _ in req}):
        idx = [i for i, (m, _) in enumerate(req) if m == y]
        for sq in squares_of(y):
            want = share_pieces(sq.share_proofs_batch([req[i][1] for i in idx]))
            assert [pieces[i] for i in idx] == want, ("square", y)
    return got


# ----------------------------------------------------------- 1. bytes
@pytest.mark.parametrize("k", sorted(KN))
def test_namespace_answers_equal_the_restatement_and_the_members(sets, k):
    sqset, refs, singles = sets(k)
    assert len(sqset) == KN[k] == len(refs)
    every = interleave([ref.queries(r) for r in refs])
    assert len({y for y, _ in every[:len(refs)]}) == len(refs), "members interleave in request order"
    assert any(not ref_answer(refs[y], ns) for y, ns in every) and any(ref_answer(refs[y], ns) for y, ns in every)
    for qs in (every, (every * 37)[:37]):   # 37: no multiple of the four waves of a workgroup
        nss = [ns for _, ns in qs]
        got = sqset.namespace_proofs(qs)
        assert got.squares.tolist() == [y for y, _ in qs]
        want = assert_batch_equals(got.batch, k, nss, [ref_answer(refs[y], ns) for y, ns in qs])
        assert_plan_equals(sqset.namespace_plan(qs), want)
        answers = plain(got.answers())
        for y in range(len(refs)):
            idx = [i for i, (m, _) in enumerate(qs) if m == y]
            for sq in (singles[y], sqset[y]):
                assert plain(sq.namespace_proofs([nss[i] for i in idx]).answers()) == [answers[i] for i in idx], y
    none = sqset.namespace_proofs([])
    assert len(none) == 0 and none.batch.seg_off.tolist() == [0]
    assert sqset.namespace_plan([]) == {"n_segments": 0, "n_nodes": 0, "n_shares": 0}


@pytest.mark.parametrize("k", sorted(KN))
def test_share_ranges_equal_the_members(sets, k):
    sqset, refs, singles = sets(k)
    every = interleave([ranges_of(k, 10 * k + y) for y in range(len(refs))])
    for req in (every, (every * 37)[:37]):
        got = assert_ranges_equal_members(sqset, lambda y: (singles[y], sqset[y]), req)
        from celestia_da.proof import share_proofs_plan
        p = share_proofs_plan(k, [r for _, r in req])   # the host-only plan sizes the set call as it is
        b = got.batch
        assert (p["n_segments"], p["n_nodes"], p["n_aunts"], p["n_shares"]) == \
            (len(b.row_roots), len(b.nodes), len(b.aunts), len(b.shares))
    assert len(sqset.share_proofs_batch(np.zeros((0, 3), np.int64))) == 0


# ----------------------------------------------------------- 2. row blocks
@pytest.fixture(scope="module")
def big_pair(ctx):
    from celestia_da import proof as gpr
    ref_sq, nss = run_square()
    ods = [ref_sq.ods, np.asarray(coracle.random_square(128, 4321)).reshape(-1, 512)]
    sqset = gpr.ResidentSquareSet.from_ods(np.stack(ods), ctx)
    singles = [gpr.ResidentSquare(o, ctx) for o in ods]
    yield sqset, singles, nss
    for s in singles:
        s.close()
    sqset.close()


def test_row_blocks_at_k128(big_pair):
    sqset, singles, nss = big_pair
    assert len(nss) == 64
    qs = interleave([nss, nss])
    got = sqset.namespace_proofs(qs)
    answers = plain(got.answers())
    for y in range(2):
        want = plain(singles[y].namespace_proofs(nss).answers())
        assert [answers[i] for i in range(y, 128, 2)] == want, y
    run = answers[2 * 2]   # run 40 of member 0: both 64-row blocks
    assert [r for r, *_ in run] == [62, 63, 64]
    assert any(r >= 64 and leaf for a in answers[0::2] for r, _, _, _, leaf, _ in a), "absences in rows >= 64"
    plan = sqset.namespace_plan(qs)
    assert plan == {"n_segments": len(got.batch.row), "n_nodes": len(got.batch.nodes), "n_shares": len(got.batch.shares)}
    k = 128
    req = interleave([[(62 * k + 100, 65 * k + 3), (0, 1), (k * k - 1, k * k)], [(63 * k, 64 * k), (5, 700)]])
    assert_ranges_equal_members(sqset, lambda y: (singles[y],), req)


# ----------------------------------------------------------- 3. offsets past 2^32
def test_offsets_past_4gib(ctx):
    import torch
    from celestia_da import proof as gpr
    k, n, period = 128, 130, 3
    three = np.stack([coracle.random_square(k, 4100 + i) for i in range(period)])
    d_three = device(three)
    d_ods = d_three[torch.arange(n, device="cuda") % period].contiguous()
    sqset = gpr.ResidentSquareSet.from_device_ods(d_ods, k, n, ctx=ctx)
    del d_ods
    ones = [gpr.ResidentSquare(three[i], ctx) for i in range(period)]
    try:
        assert n * (2 * k) ** 2 * 512 > 1 << 32
        members = (0, 1, 128, 129)
        per = []
        for y in members:
            o = three[y % period].reshape(k * k, 512)
            present = [o[i, :29].tobytes() for i in (0, 64 * k + 5, k * k - 1, 70 * k)]
            absent = [(int.from_bytes(ns, "big") + 1).to_bytes(29, "big") for ns in present[:2]]
            per.append(present + absent)
        qs = [(members[j], ns) for j, ns in interleave(per)]
        answers = plain(sqset.namespace_proofs(qs).answers())
        assert any(a for a in answers)
        for j, y in enumerate(members):
            idx = [i for i, (m, _) in enumerate(qs) if m == y]
            assert [answers[i] for i in idx] == plain(ones[y % period].namespace_proofs(per[j]).answers()), y
        req = [(members[j], r) for j, r in interleave([[(0, 3), (64 * k - 2, 64 * k + 2), (k * k - 5, k * k)]] * 4)]
        assert_ranges_equal_members(sqset, lambda y: (ones[y % period],), req)
    finally:
        for s in ones:
            s.close()
        sqset.close()


# ----------------------------------------------------------- 4. NULL outputs
def test_null_outputs(ctx, sets):
    k = 4
    sqset, refs, _ = sets(k)
    qs = interleave([ref.queries(r) for r in refs])[:41]
    squares, nss = u32([y for y, _ in qs]), [ns for _, ns in qs]
    full = sqset.namespace_proofs(qs).batch
    plan = sqset.namespace_plan(qs)
    assert plan["n_shares"] and (full.kind == 2).any() and (full.kind == 1).any()
    fields = NamespaceProofsBatch.FIELDS
    for skip in [(f,) for f in fields] + [fields]:
        out = NamespaceProofsBatch.empty(k, nss, plan, fill=0xAA)
        o = out.out_struct(skip=skip)
        assert ctx.lib.cda_square_set_namespace_proofs(sqset.h, p32(squares), ptr(full.namespaces), len(qs),
                                                       C.byref(o)) == CDA_OK, skip
        for name, got, exp in zip(fields, out.arrays(), full.arrays()):
            assert (got.view(np.uint8) == 0xAA).all() if name in skip else np.array_equal(got, exp), (skip, name)
    assert ctx.lib.cda_square_set_namespace_proofs(sqset.h, p32(squares), ptr(full.namespaces), len(qs), None) == CDA_ERR_INVALID
    assert ctx.lib.cda_square_set_namespace_plan(sqset.h, p32(squares), ptr(full.namespaces), len(qs), None) == CDA_ERR_INVALID

    req = interleave([ranges_of(k, 70 + y) for y in range(len(refs))])[:41]
    r = np.array([(y, s, e) for y, (s, e) in req], dtype=np.int64)
    sq_col, starts, ends = u32(r[:, 0]), u32(r[:, 1]), u32(r[:, 2])
    full = sqset.share_proofs_batch(r).batch
    fields = ShareProofsBatch.FIELDS
    for skip in [(f,) for f in fields] + [fields]:
        out = ShareProofsBatch.empty(k, r[:, 1:], fill=0xAA)
        o = out.out_struct(skip=skip)
        assert ctx.lib.cda_square_set_share_proofs(sqset.h, p32(sq_col), p32(starts), p32(ends), len(r), C.byref(o)) == CDA_OK, skip
        for name, got, exp in zip(fields, out.arrays(), full.arrays()):
            assert (got.view(np.uint8) == 0xAA).all() if name in skip else np.array_equal(got, exp), (skip, name)
    assert ctx.lib.cda_square_set_share_proofs(sqset.h, p32(sq_col), p32(starts), p32(ends), len(r), None) == CDA_ERR_INVALID


# ----------------------------------------------------------- 5. verifier
def verify_set(ctx, k, row_roots, squares, nss, answers):
    batch = NamespaceProofsBatch.from_answers(k, nss, answers)
    return SetNamespaceProofs(batch, u32(squares)).verify(row_roots, ctx).tolist()


@pytest.mark.parametrize("k", sorted(KN))
def test_honest_batches_verify(ctx, sets, k):
    sqset, refs, _ = sets(k)
    rows, _, _ = sqset.dah()
    for y, r in enumerate(refs):
        assert rows[y].tobytes() == b"".join(r.row_roots), y
    qs = interleave([ref.queries(r) for r in refs])
    got = sqset.namespace_proofs(qs)
    assert not got.verify(rows, ctx).any()
    import celestia_da
    ns = refs[0].namespaces()[0]
    answers = celestia_da.get_shares_by_namespace_set(sqset, ns)
    assert plain(answers) == plain([ref_answer(r, ns) for r in refs])
    assert celestia_da.verify_namespaced_shares_set(rows, range(len(refs)), ns, answers, ctx).tolist() == \
        [ref.answer_verdict(r.row_roots, ns, a) for r, a in zip(refs, answers)] == [0] * len(refs)
    some = celestia_da.get_shares_by_namespace_set(sqset, ns, squares=[len(refs) - 1, 0])
    assert plain(some) == plain([answers[-1], answers[0]])


@pytest.mark.parametrize("k", [2, 4, 8])
def test_tampers_among_honest_queries(ctx, sets, k):
    """Every tamper of member 0 (the ref square), each between honest queries of the other members."""
    sqset, refs, _ = sets(k)
    rows, _, _ = sqset.dah()
    tampers = ref.tampers(f"small{k}")
    assert len(tampers) >= 6
    others = interleave([ref.queries(r) for r in refs[1:]])
    squares, nss, answers, want = [], [], [], []
    for j, (label, ns, answer, verdict) in enumerate(tampers):
        y, hns = others[j % len(others)]
        for sq_i, q_ns, q_ans in ((y + 1, hns, ref_answer(refs[y + 1], hns)), (0, ns, answer)):
            squares.append(sq_i)
            nss.append(q_ns)
            answers.append(q_ans)
            want.append(ref.answer_verdict(refs[sq_i].row_roots, q_ns, q_ans))
        assert want[-1] == verdict and want[-2] == 0, label
    assert verify_set(ctx, k, rows, squares, nss, answers) == want
    # cda_namespace_proofs_verify is the set call with n_squares = 1: the queries of member 0 alone
    mine = [i for i, s in enumerate(squares) if s == 0]
    batch = NamespaceProofsBatch.from_answers(k, [nss[i] for i in mine], [answers[i] for i in mine])
    single = batch.verify(rows[0], ctx).tolist()
    assert single == [want[i] for i in mine]
    assert SetNamespaceProofs(batch, np.zeros(len(mine), np.uint32)).verify(rows[:1], ctx).tolist() == single


def test_an_answer_under_another_members_index(ctx, sets):
    k = 4
    sqset, refs, _ = sets(k)
    rows, _, _ = sqset.dah()
    squares, nss, answers, want = [], [], [], []
    for y, r in enumerate(refs):
        other = (y + 1) % len(refs)
        for ns in r.namespaces()[:4]:
            squares.append(other)
            nss.append(ns)
            answers.append(ref_answer(r, ns))
            want.append(ref.answer_verdict(refs[other].row_roots, ns, answers[-1]))
    assert all(want) and len(want) >= 8
    assert verify_set(ctx, k, rows, squares, nss, answers) == want
    own = [(s - 1) % len(refs) for s in squares]
    assert verify_set(ctx, k, rows, own, nss, answers) == [0] * len(want)


def test_share_proofs_of_a_set_verify_with_their_own_roots(ctx, sets):
    """Every range of ranges_of and every run of one namespace of every member, in one batch, through
    cda_share_proofs_verify with each proof's own data root.  The yardstick is the verdict the singly created
    square's own batch of the same ranges gets against its own root.  ShareProof.Validate hashes every share
    under the proof's one namespace, so -- as tests/test_share_proofs_batch.py states for a single square -- a
    range that holds more than one namespace (one_namespace = 0) gets verdict 2 there and here, every other 0."""
    k = 4
    sqset, refs, singles = sets(k)
    _, _, roots = sqset.dah()
    runs = [[(r * k + p.start, r * k + p.end) for ns in m.namespaces() for r, p, _ in ref_answer(m, ns)
             if not p.leaf_hash] for m in refs]
    req = interleave([ranges_of(k, 90 + y) + runs[y] for y in range(len(refs))])
    got = sqset.share_proofs_batch([(y, s, e) for y, (s, e) in req])
    want = np.zeros(len(req), dtype=np.uint8)
    for y, single in enumerate(singles):
        idx = [i for i, (m, _) in enumerate(req) if m == y]
        want[idx] = single.share_proofs_batch([req[i][1] for i in idx]).verify(single.dah()[2], ctx)
    one = got.batch.one_namespace.astype(bool)
    assert one.sum() > 4 * len(refs) and (~one).sum() > len(refs)
    assert any(e - s > 1 and one[i] for i, (_, (s, e)) in enumerate(req))
    assert want.tolist() == np.where(one, 0, 2).tolist()
    assert got.verify(roots, ctx).tolist() == want.tolist()
    wrong = got.batch.verify(roots[(got.squares + 1) % len(refs)], ctx)
    assert (wrong == 1).all(), "a proof verifies only against its own square's data root"
    hit = int(np.nonzero(one)[0][7])
    first = int(sum(e - s for _, (s, e) in req[:hit]))
    got.batch.shares[first, 300] ^= 0x10
    v = got.verify(roots, ctx).tolist()
    assert v == [2 if i == hit else int(w) for i, w in enumerate(want)], "caught in its proof alone"


# ----------------------------------------------------------- 6. validation
def filled(batch):
    return all((a.view(np.uint8) == 0xAA).all() for a in batch.arrays())


def test_validation(ctx, sets):
    k = 4
    sqset, refs, _ = sets(k)
    n = len(refs)
    err = lambda: ctx.lib.cda_last_error(ctx.h).decode()   # noqa: E731
    qs = interleave([ref.queries(r)[:3] for r in refs])
    squares, ns_arr = split_set_queries(qs)
    plan = sqset.namespace_plan(qs)
    big = {f: v + 8 for f, v in plan.items()}

    def ns_calls(sq_col, ns_col, count):
        out = NamespaceProofsBatch.empty(k, ns_arr, big, fill=0xAA)
        o = out.out_struct()
        p = _lib.NamespacePlanT(0xAAAA, 0xAAAA, 0xAAAA)
        rc = (ctx.lib.cda_square_set_namespace_plan(sqset.h, sq_col, ns_col, count, C.byref(p)), err(),
              ctx.lib.cda_square_set_namespace_proofs(sqset.h, sq_col, ns_col, count, C.byref(o)), err())
        assert filled(out) and (p.n_segments, p.n_nodes, p.n_shares) == (0xAAAA,) * 3
        return rc

    bad = squares.copy()
    bad[3] = 9
    text = f"query 3: square 9 is not below the set's {n} squares"
    assert ns_calls(p32(bad), ptr(ns_arr), len(qs)) == (CDA_ERR_INVALID, text, CDA_ERR_INVALID, text)
    par = ns_arr.copy()
    par[5] = 0xFF
    text = "query 5: namespace is the parity shares namespace"
    assert ns_calls(p32(squares), ptr(par), len(qs)) == (CDA_ERR_INVALID, text, CDA_ERR_INVALID, text)
    # the set's own array by its name, the namespaces with the single-square call's text
    for a, b, text in ((None, ptr(ns_arr), "null squares"), (p32(squares), None, "null buffer")):
        assert ns_calls(a, b, len(qs)) == (CDA_ERR_INVALID, text, CDA_ERR_INVALID, text)
    # n == 0: CDA_OK, whatever the arrays
    p = _lib.NamespacePlanT(7, 7, 7)
    assert ctx.lib.cda_square_set_namespace_plan(sqset.h, None, None, 0, C.byref(p)) == CDA_OK
    assert (p.n_segments, p.n_nodes, p.n_shares) == (0, 0, 0)
    assert ctx.lib.cda_square_set_namespace_proofs(sqset.h, None, None, 0, C.byref(_lib.NamespaceProofsOut())) == CDA_OK

    # share ranges
    req = np.array([(y, s, e) for y, (s, e) in interleave([ranges_of(k, y)[:3] for y in range(n)])], dtype=np.int64)
    sq_col, starts, ends = u32(req[:, 0]), u32(req[:, 1]), u32(req[:, 2])

    def share_call(a, b, c, count=len(req)):
        out = ShareProofsBatch.empty(k, req[:, 1:], fill=0xAA)
        o = out.out_struct()
        rc = ctx.lib.cda_square_set_share_proofs(sqset.h, a, b, c, count, C.byref(o))
        assert filled(out)
        return rc, err()

    bad = sq_col.copy()
    bad[4] = n
    assert share_call(p32(bad), p32(starts), p32(ends)) == \
        (CDA_ERR_INVALID, f"range 4: square {n} is not below the set's {n} squares")
    bad_end = ends.copy()
    bad_end[2] = k * k + 6
    rc, text = share_call(p32(sq_col), p32(starts), p32(bad_end))
    single = ShareProofsBatch.empty(k, req[:, 1:], fill=0xAA)
    assert sqset[0].ctx.lib.cda_square_share_proofs(sqset[0].h, p32(starts), p32(bad_end), len(req),
                                                    C.byref(single.out_struct())) == CDA_ERR_INVALID
    assert rc == CDA_ERR_INVALID and text == err() and text.startswith("range 2: end ")
    assert share_call(None, p32(starts), p32(ends)) == (CDA_ERR_INVALID, "null squares")
    for args in ((p32(sq_col), None, p32(ends)), (p32(sq_col), p32(starts), None)):
        assert share_call(*args) == (CDA_ERR_INVALID, "null buffer")
    assert ctx.lib.cda_square_set_share_proofs(sqset.h, None, None, None, 0, C.byref(_lib.ShareProofsOut())) == CDA_OK


def test_verifier_validation(ctx, sets):
    k = 4
    sqset, refs, _ = sets(k)
    rows, _, _ = sqset.dah()
    n = len(refs)
    qs = interleave([ref.queries(r)[:4] for r in refs])
    got = sqset.namespace_proofs(qs)
    roots = np.ascontiguousarray(rows).reshape(-1)

    def call(b, squares=got.squares, n_squares=n, row_roots=roots, width=k):
        verdict = np.full(len(qs), 0xAA, dtype=np.uint8)
        rc = ctx.lib.cda_namespace_proofs_verify_set(ctx.h, width, None if row_roots is None else ptr(row_roots),
                                                     n_squares, None if squares is None else p32(squares),
                                                     None if b is None else C.byref(b), ptr(verdict))
        assert rc != CDA_OK and (verdict == 0xAA).all()
        return rc, ctx.lib.cda_last_error(ctx.h).decode()

    def single_text(b):
        """The text cda_namespace_proofs_verify answers to the same batch."""
        verdict = np.full(len(qs), 0xAA, dtype=np.uint8)
        assert ctx.lib.cda_namespace_proofs_verify(ctx.h, k, ptr(roots), C.byref(b), ptr(verdict)) == CDA_ERR_INVALID
        return ctx.lib.cda_last_error(ctx.h).decode()

    bad = got.squares.copy()
    bad[6] = n + 2
    assert call(got.batch.batch(), squares=bad) == \
        (CDA_ERR_INVALID, f"query 6: square {n + 2} is not below the {n} squares of row_roots")
    assert call(got.batch.batch(), n_squares=1)[1].startswith("query 1: square 1 is not below the 1 squares")
    assert call(got.batch.batch(), squares=None) == (CDA_ERR_INVALID, "null squares")
    assert call(got.batch.batch(), row_roots=None) == (CDA_ERR_INVALID, "null row_roots / namespaces / seg_off")
    assert call(None) == (CDA_ERR_INVALID, "null batch")
    assert call(got.batch.batch(), width=3)[0] == CDA_ERR_INVALID
    # the structural errors of cda_namespace_proofs_verify, reached through the set call, with its texts
    g = int(np.nonzero(got.batch.kind == 2)[0][0])
    seen = set()
    for field, at, value in (("kind", 1, 3), ("row", 2, 2 * k), ("nmt_start", 0, -1), ("nmt_end", g, int(got.batch.nmt_start[g]) + 2),
                             ("node_off", 1, 10 ** 6), ("share_off", 1, 10 ** 6), ("seg_off", 0, 1)):
        saved = getattr(got.batch, field).copy()
        getattr(got.batch, field)[at] = value
        b = got.batch.batch()
        rc, text = call(b)
        assert rc == CDA_ERR_INVALID and text == single_text(b) and text, field
        seen.add(text)
        getattr(got.batch, field)[:] = saved
    assert len(seen) == 7
    par = got.batch.namespaces.copy()
    got.batch.namespaces[2] = 0xFF
    assert call(got.batch.batch()) == (CDA_ERR_INVALID, "query 2: namespace is the parity shares namespace")
    got.batch.namespaces[:] = par
    b = got.batch.batch()
    b.n_shares += 1
    assert call(b)[1].startswith("n_shares is ")
    assert not got.verify(rows, ctx).any()
    b = got.batch.batch()
    b.n_queries = 0
    assert ctx.lib.cda_namespace_proofs_verify_set(ctx.h, k, None, 0, None, C.byref(b), None) == CDA_OK


# ----------------------------------------------------------- 7. push order
def test_push_order_of_a_member(ctx):
    from celestia_da import proof as gpr
    k, n, bad = 4, 5, (1, 4)
    ods = np.stack([testfactory.random_square(k, 60 + i).reshape(k, k, 512) for i in range(n)])
    for i in bad:
        ods[i] = _unordered_square(k, 60 + i)
    sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    lone = gpr.ResidentSquare(ods[4], ctx)
    try:
        assert sqset.status.tolist() == [0, CDA_ERR_PUSH_ORDER, 0, 0, CDA_ERR_PUSH_ORDER]
        qs = [(y, ods[y, 0, 0, :29].tobytes()) for y in (0, 2, 4, 3)]
        nss = [ns for _, ns in qs]
        out = NamespaceProofsBatch.empty(k, nss, {"n_segments": 16, "n_nodes": 64, "n_shares": 16}, fill=0xAA)
        with pytest.raises(PushOrderError) as e:
            sqset.namespace_proofs(qs, out=out)
        assert e.value.code == CDA_ERR_PUSH_ORDER
        assert str(e.value).startswith("query 2: square 4: the square's row 1 is not ordered by namespace at position ")
        assert filled(out)
        assert ctx.push_order_detail()[:2] == (0, 1)
        with pytest.raises(PushOrderError):
            sqset.namespace_plan(qs)
        ok = [q for q in qs if q[0] != 4]
        got = sqset.namespace_proofs(ok)
        for (y, ns), a in zip(ok, plain(got.answers())):
            assert a == plain(sqset[y].namespace_proofs([ns]).answers())[0] and a
        req = [(4, (0, 3)), (0, (2, 9)), (4, (5, 16)), (1, (0, 16))]
        assert_ranges_equal_members(sqset, lambda y: (lone,) if y == 4 else (sqset[y],), req)
    finally:
        lone.close()
        sqset.close()


# ----------------------------------------------------------- 8. end to end
def test_end_to_end_one_namespace_over_heights(ctx):
    import celestia_da
    from celestia_da import blobfactory, proof as gpr, shares, square as gsq
    rng = np.random.default_rng(2024)
    mine = blobfactory.random_blob_namespace_id(rng)
    ns = b"\x00" + mine
    submitted, ods = [], []
    for h in range(6):
        block = blobfactory.random_block(300 + h, 2, 4, (1, 2), (1, 3000))
        data = []
        if h % 2 == 0:   # every other height holds blobs of the namespace
            data = [rng.integers(0, 256, int(rng.integers(1, 2500)), dtype=np.uint8).tobytes() for _ in range(1 + h // 2)]
            block.append(blobfactory.blob_tx(b"\x01" * 250, [(mine, d) for d in data]))
        submitted.append(data)
        sq = gsq.construct(block, 16, 64, ctx=ctx)
        ods.append(np.frombuffer(sq.to_bytes(), dtype=np.uint8))
    assert len({o.size for o in ods}) == 1, "the blocks are of one width"
    sqset = gpr.ResidentSquareSet.from_ods(np.stack(ods), ctx)
    try:
        rows, _, _ = sqset.dah()
        answers = celestia_da.get_shares_by_namespace_set(sqset, ns)
        assert len(answers) == 6
        assert not celestia_da.verify_namespaced_shares_set(rows, range(6), ns, answers, ctx).any()
        for h, (data, answer) in enumerate(zip(submitted, answers)):
            want = ref.get_shares_by_namespace(ref.RefSquare(ods[h]), ns)   # a temporary: not through the id cache
            assert plain([answer]) == plain([want]), h
            got = [x for _, _, sh in answer for x in sh]
            if data:
                blobs = shares.parse_blobs(got)
                assert [b.data for b in blobs] == data and all(b.namespace == ns for b in blobs), h
            else:
                assert not got and all(p.leaf_hash for _, p, _ in answer), h   # absence proofs, or no rows
        # one height's answer does not pass for another's
        swapped = celestia_da.verify_namespaced_shares_set(rows, [2, 1, 0, 3, 4, 5], ns, answers, ctx)
        assert swapped[0] and swapped[2] and not swapped[1]
    finally:
        sqset.close()
