"""All shares of a namespace from a resident square: cda_square_namespace_plan / cda_square_namespace_proofs
(csrc/namespace_proofs.hip) and ResidentSquare.namespace_proofs, against the CPU restatement of nmt
ProveNamespace and GetSharesByNamespace's row selection (tests/nmt_namespace_ref.py).  Every output array, cut
by the offsets, equals the restatement's bytes; inclusion segments are also tied to share_proofs_batch, whose
bytes the oracle pins.  No tolerances.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import nmt_namespace_ref as ref
import pyref
from celestia_da import CdaError, PushOrderError, _lib, testfactory
from celestia_da._lib import ptr
from celestia_da.namespace import NamespaceProofsBatch, namespace_plan

NAMES = ("small1", "small2", "small4", "small8", "hand")


@pytest.fixture(scope="module")
def resident(ctx):
    """ResidentSquare of a RefSquare, one per square for the whole module."""
    from celestia_da import proof as gpr
    made = {}

    def get(sq):
        if id(sq) not in made:
            made[id(sq)] = gpr.ResidentSquare(sq.ods, ctx)
        return made[id(sq)]
    yield get
    for sq in made.values():
        sq.close()


def assert_batch_equals(got, k, namespaces, answers):
    want = NamespaceProofsBatch.from_answers(k, namespaces, answers)
    for name, g, w in zip(NamespaceProofsBatch.FIELDS, got.arrays(), want.arrays()):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
            raise AssertionError((name, "first differing entry", int(bad[0]), "of", g.shape[0]))
    return want


def assert_plan_equals(plan, batch):
    assert plan == {"n_segments": len(batch.row), "n_nodes": len(batch.nodes), "n_shares": len(batch.shares)}


# ------------------------------------------------------------ 1. bytes against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_answers_equal_the_restatement(resident, name):
    """Every query of the square's inventory in one call, each alone, and no query at all."""
    ref_sq = ref.squares()[name]
    sq = resident(ref_sq)
    nss = [ns for ns, _ in ref.honest(name)]
    answers = [a for _, a in ref.honest(name)]
    want = assert_batch_equals(sq.namespace_proofs(nss), sq.k, nss, answers)
    assert_plan_equals(namespace_plan(sq, nss), want)
    for ns, a in zip(nss, answers):
        one = assert_batch_equals(sq.namespace_proofs([ns]), sq.k, [ns], [a])
        assert_plan_equals(namespace_plan(sq, [ns]), one)
        got = sq.namespace_proofs([ns]).answers()[0]
        assert [(r, p.start, p.end, p.nodes, p.leaf_hash, sh) for r, p, sh in got] == \
            [(r, p.start, p.end, p.nodes, p.leaf_hash, sh) for r, p, sh in a]
    none = sq.namespace_proofs([])
    assert len(none) == 0 and none.seg_off.tolist() == [0] and none.node_off.tolist() == [0]
    assert none.share_off.tolist() == [0]
    assert namespace_plan(sq, []) == {"n_segments": 0, "n_nodes": 0, "n_shares": 0}


@pytest.mark.gpu
def test_module_level_calls(ctx, resident):
    import celestia_da
    ref_sq = ref.squares()["hand"]
    b = ref_sq.ods[2, :29].tobytes()
    for source in (resident(ref_sq), ref_sq.ods):
        ans = celestia_da.get_shares_by_namespace(source, b)
        assert [(r, p.start, p.end, bool(p.leaf_hash), sh) for r, p, sh in ans] == \
            [(0, 1, 2, True, []), (1, 0, 1, False, [ref_sq.ods[2].tobytes()])]
        assert celestia_da.verify_namespaced_shares(ref_sq.row_roots, b, ans) == 0
        assert celestia_da.verify_namespaced_shares(ref_sq.row_roots, b, ans[1:]) == 1


# ------------------------------------------------------------ 2. NULL outputs
@pytest.mark.gpu
def test_every_subset_of_null_outputs(ctx, resident):
    """Every strict subset of the ten outputs passed as NULL (1 023 calls): the others as in the full call, the
    skipped ones untouched."""
    name = "small4"
    sq = resident(ref.squares()[name])
    nss = [ns for ns, _ in ref.honest(name)]
    full = sq.namespace_proofs(nss)
    plan = namespace_plan(sq, nss)
    assert plan["n_shares"] and (full.kind == 2).any() and (full.kind == 1).any()
    ns_arr = full.namespaces
    fields = NamespaceProofsBatch.FIELDS
    n_calls = 0
    for m in range(len(fields)):
        for skip in itertools.combinations(fields, m):
            out = NamespaceProofsBatch.empty(sq.k, nss, plan, fill=0xAA)
            o = out.out_struct(skip=skip)
            assert ctx.lib.cda_square_namespace_proofs(sq.h, ptr(ns_arr), len(nss), C.byref(o)) == _lib.CDA_OK, skip
            n_calls += 1
            for fname, got, exp in zip(fields, out.arrays(), full.arrays()):
                if fname in skip:
                    assert (got.view(np.uint8) == 0xAA).all(), (skip, fname)
                else:
                    assert np.array_equal(got, exp), (skip, fname)
    assert n_calls == 2 ** len(fields) - 1
    assert ctx.lib.cda_square_namespace_proofs(sq.h, ptr(ns_arr), len(nss),
                                               C.byref(_lib.NamespaceProofsOut())) == _lib.CDA_OK
    assert ctx.lib.cda_square_namespace_proofs(sq.h, ptr(ns_arr), len(nss), None) == _lib.CDA_ERR_INVALID


# ------------------------------------------------------------ 3. the reference-pinned path
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small8", "hand"])
def test_inclusion_segments_equal_share_proofs_batch(resident, name):
    sq = resident(ref.squares()[name])
    k = sq.k
    got = sq.namespace_proofs([ns for ns, _ in ref.honest(name)])
    inc = np.nonzero(got.kind == 1)[0]
    assert len(inc) >= 2
    ranges = [(int(got.row[g]) * k + int(got.nmt_start[g]), int(got.row[g]) * k + int(got.nmt_end[g])) for g in inc]
    tied = sq.share_proofs_batch(ranges)
    assert tied.seg_off.tolist() == list(range(len(inc) + 1))
    share_at = 0
    for i, g in enumerate(inc):
        n_sh = ranges[i][1] - ranges[i][0]
        assert np.array_equal(got.nodes[got.node_off[g]:got.node_off[g + 1]],
                              tied.nodes[tied.node_off[i]:tied.node_off[i + 1]]), g
        assert np.array_equal(got.shares[int(got.share_off[g]):int(got.share_off[g + 1])],
                              tied.shares[share_at:share_at + n_sh]), g
        share_at += n_sh


# ------------------------------------------------------------ 4. runs across rows at k = 128
_run = {}


def run_square():
    """pyref.random_namespaced_square(128) with share i under the namespace of share 200 * (i // 200): runs of
    200 shares that span two to three rows; run 40 crosses the boundary of rows 63 and 64."""
    if not _run:
        k = 128
        ods = pyref.random_namespaced_square(k)
        for i in range(k * k):
            ods[i, :29] = ods[200 * (i // 200), :29]
        sq = ref.RefSquare(ods)
        starts = [bytes(ods[s, :29]) for s in range(0, k * k, 200)]
        assert len(starts) == 82 and starts == sorted(set(starts))
        assert (40 * 200) // k == 62 and (41 * 200 - 1) // k == 64
        present = [starts[0], starts[-1], starts[40]] + starts[1:30]
        absent = [(int.from_bytes(ns, "big") + 1).to_bytes(29, "big") for ns in starts[30:62]]
        assert len(present) == 32 and len(absent) == 32 and not set(absent) & set(starts)
        _run["sq"], _run["queries"] = sq, present + absent
    return _run["sq"], _run["queries"]


@pytest.mark.gpu
def test_runs_of_200_shares_at_k128(resident):
    ref_sq, nss = run_square()
    answers = [ref.get_shares_by_namespace(ref_sq, ns) for ns in nss]
    assert [r for r, _, _ in answers[2]] == [62, 63, 64]                   # run 40: both 64-row blocks
    assert all(2 <= len(a) <= 3 and all(not p.leaf_hash for _, p, _ in a) for a in answers[:32])
    assert all(len(a) <= 1 and all(p.leaf_hash for _, p, _ in a) for a in answers[32:])
    assert sum(len(a) for a in answers[32:]) >= 16 and any(r >= 64 for a in answers[32:] for r, _, _ in a)
    sq = resident(ref_sq)
    want = assert_batch_equals(sq.namespace_proofs(nss), sq.k, nss, answers)
    assert_plan_equals(namespace_plan(sq, nss), want)
    assert len(want.shares) == 32 * 200 - (200 - (128 * 128 - 81 * 200))


# ------------------------------------------------------------ 5. errors
@pytest.mark.gpu
def test_parity_namespace_query_is_invalid(ctx, resident):
    name = "small4"
    sq = resident(ref.squares()[name])
    nss = [ns for ns, _ in ref.honest(name)]
    plan = namespace_plan(sq, nss)
    bad = nss[:3] + [ref.PARITY] + nss[3:]
    out = NamespaceProofsBatch.empty(sq.k, bad, {k: v + 8 for k, v in plan.items()}, fill=0xAA)
    with pytest.raises(CdaError) as e:
        sq.namespace_proofs(bad, out=out)
    assert e.value.code == _lib.CDA_ERR_INVALID and str(e.value) == "query 3: namespace is the parity shares namespace"
    for a in out.arrays():
        assert (a.view(np.uint8) == 0xAA).all()
    p = _lib.NamespacePlanT(0xAAAA, 0xAAAA, 0xAAAA)
    arr = out.namespaces
    assert ctx.lib.cda_square_namespace_plan(sq.h, ptr(arr), len(bad), C.byref(p)) == _lib.CDA_ERR_INVALID
    assert ctx.lib.cda_last_error(ctx.h).decode().startswith("query 3: ")
    assert (p.n_segments, p.n_nodes, p.n_shares) == (0xAAAA, 0xAAAA, 0xAAAA)
    assert ctx.lib.cda_square_namespace_plan(sq.h, None, 1, C.byref(p)) == _lib.CDA_ERR_INVALID
    assert ctx.lib.cda_square_namespace_plan(sq.h, ptr(arr), 1, None) == _lib.CDA_ERR_INVALID


@pytest.mark.gpu
def test_unordered_square_answers_push_order(ctx):
    """nmt could not have built the trees of a square whose rows are not ordered: both calls say so and write
    nothing."""
    from celestia_da import proof as gpr
    k = 4
    ods = testfactory.random_square(k, 5).reshape(k, k, 512).copy()
    ods[1, [0, 3]] = ods[1, [3, 0]]                # row 1 and columns 0 / 3 out of order, as tests/test_malicious.py
    sq = gpr.ResidentSquare(ods, ctx)
    try:
        assert sq.push_order_error
        nss = [ods[0, 0, :29].tobytes(), ods[1, 3, :29].tobytes()]
        out = NamespaceProofsBatch.empty(k, nss, {"n_segments": 8, "n_nodes": 32, "n_shares": 8}, fill=0xAA)
        with pytest.raises(PushOrderError) as e:
            sq.namespace_proofs(nss, out=out)
        assert e.value.code == _lib.CDA_ERR_PUSH_ORDER and "row 1" in str(e.value)
        for a in out.arrays():
            assert (a.view(np.uint8) == 0xAA).all()
        with pytest.raises(PushOrderError):
            namespace_plan(sq, nss)
        assert len(sq.share_proofs_batch([(0, 3)])) == 1   # share proofs are served as before
    finally:
        sq.close()
