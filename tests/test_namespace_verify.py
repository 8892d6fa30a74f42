"""cda_namespace_proofs_verify (csrc/verify.hip): nmt Proof.VerifyNamespace per row and GetSharesByNamespace's
row selection per query, against the CPU restatement (tests/nmt_namespace_ref.py).  The batches come from the
restatement, so the verifier is tested without the GPU prover; one more comes straight from namespace_proofs.
"""
import ctypes as C

import numpy as np
import pytest

import nmt_namespace_ref as ref
from celestia_da import _lib
from celestia_da._lib import ptr
from celestia_da.namespace import NamespaceProofsBatch

NAMES = ("small1", "small2", "small4", "small8", "hand")


def mixed(name):
    """(labels, namespaces, answers, verdicts): every honest answer of the square, then every tamper."""
    honest = [("honest", ns, a, 0) for ns, a in ref.honest(name)]
    return tuple(zip(*(honest + ref.tampers(name))))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_mixed_batch_gets_the_restatements_verdicts(ctx, name):
    """One batch of every honest answer and every tamper: each query exactly its verdict, which is the
    restatement's, every honest query 0."""
    sq = ref.squares()[name]
    labels, nss, answers, want = mixed(name)
    if name in ("small4", "small8"):
        assert set(labels) == set(ref.TAMPER_LABELS) | {"honest"}
    assert [ref.answer_verdict(sq.row_roots, ns, a) for ns, a in zip(nss, answers)] == list(want)
    got = NamespaceProofsBatch.from_answers(sq.k, nss, answers).verify(sq.row_roots, ctx)
    assert got.tolist() == list(want), [(lb, g, w) for lb, g, w in zip(labels, got.tolist(), want) if g != w]


@pytest.mark.gpu
def test_precedence(ctx):
    """A dropped row and a flipped share: 1.  A flipped share and an incomplete neighbouring segment: 2."""
    name = "small8"
    sq = ref.squares()[name]
    two = {lb: (ns, a) for lb, ns, a, _ in ref.tampers(name) if lb in ("drop_and_flip", "flip_and_incomplete")}
    nss, answers = zip(*(two[lb] for lb in ("drop_and_flip", "flip_and_incomplete")))
    assert NamespaceProofsBatch.from_answers(sq.k, nss, answers).verify(sq.row_roots, ctx).tolist() == [1, 2]


@pytest.mark.gpu
def test_the_provers_batch_verifies(ctx):
    from celestia_da import proof as gpr
    name = "small8"
    sq = ref.squares()[name]
    res = gpr.ResidentSquare(sq.ods, ctx)
    try:
        batch = res.namespace_proofs([ns for ns, _ in ref.honest(name)])
        rows, _, _ = res.dah()
        assert rows == sq.row_roots
        b = batch.batch()
        assert C.addressof(b.nodes.contents) == batch.nodes.ctypes.data      # pointer assignment, no copies
        assert C.addressof(b.shares.contents) == batch.shares.ctypes.data
        v = batch.verify(rows, ctx)
        assert len(v) == len(batch) and not v.any()
        # against another DAH (the rows reversed: the parity rows first) no answer with a row holds
        other = sq.row_roots[::-1]
        want = [ref.answer_verdict(other, ns, a) for ns, a in ref.honest(name)]
        assert set(want) == {0, 1} and batch.verify(other, ctx).tolist() == want
    finally:
        res.close()


# ------------------------------------------------------------ errors
def _set(field, index, value):
    def change(b, st):
        getattr(b, field)[index] = value
    return change


def _count(field, value):
    def change(b, st):
        st[field] = value
    return change


def _null(field):
    def change(b, st):
        st[field] = None
    return change


# name -> (change, what the message must hold).  The batch is the hand-made square's honest answers: query 5 is
# B, segments 3 (absence, row 0, [1, 2)) and 4 (inclusion, row 1, [0, 1)).
INVALID = {
    "null_namespaces": (_null("namespaces"), "null"),
    "null_seg_off": (_null("seg_off"), "null"),
    "null_row": (_null("row"), "null"),
    "null_kind": (_null("kind"), "null"),
    "null_nmt_start": (_null("nmt_start"), "null"),
    "null_nmt_end": (_null("nmt_end"), "null"),
    "null_node_off": (_null("node_off"), "null"),
    "null_nodes": (_null("nodes"), "null"),
    "null_share_off": (_null("share_off"), "null"),
    "null_shares": (_null("shares"), "null"),
    "null_absence_leaf": (_null("absence_leaf"), "absence_leaf"),
    "null_row_roots": (_null("row_roots"), "null"),
    "parity_query": (lambda b, st: b.namespaces.__setitem__(2, 0xFF), "query 2: namespace"),
    "seg_off_start": (_set("seg_off", 0, 1), "query 0: seg_off"),
    "seg_off_decreases": (_set("seg_off", 4, 0), "query 3: seg_off decreases"),
    "node_off_start": (_set("node_off", 0, 1), "node_off must start at 0"),
    "node_off_decreases": (_set("node_off", 2, 0), "segment 1: node_off decreases"),
    "node_off_end": (_count("n_nodes", 1), "node_off ends at"),
    "share_off_start": (_set("share_off", 0, 1), "share_off must start at 0"),
    "share_off_decreases": (_set("share_off", 1, 5), "segment 1: share_off"),
    "share_off_end": (_set("share_off", -1, 99), "share_off ends at"),
    "kind_0": (_set("kind", 3, 0), "segment 3: kind 0"),
    "kind_3": (_set("kind", 4, 3), "segment 4: kind 3"),
    "start_negative": (_set("nmt_start", 4, -1), "segment 4: nmt_start -1"),
    "end_not_above_start": (_set("nmt_end", 4, 0), "segment 4: nmt_end 0"),
    "end_beyond_2k": (_set("nmt_end", 4, 5), "segment 4: nmt_end 5"),
    "absence_of_two": (_set("nmt_end", 3, 3), "segment 3: an absence segment's nmt_end 3"),
    "row_2k": (_set("row", 4, 4), "segment 4: row 4"),
    "n_shares": (_count("n_shares", 1), "n_shares is 1"),
    "k_3": (_count("k", 3), "square width"),
    "k_2048": (_count("k", 2048), "square width"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_batches_leave_the_verdicts_untouched(ctx, case):
    sq = ref.squares()["hand"]
    nss, answers = zip(*ref.honest("hand"))
    b_ns = sq.ods[2, :29].tobytes()
    assert nss[5] == b_ns and [len(a) for a in answers[:6]] == [0, 0, 1, 1, 1, 2]
    batch = NamespaceProofsBatch.from_answers(sq.k, nss, answers)
    assert batch.kind.tolist()[3:5] == [2, 1] and len(batch.shares) == 4
    roots = np.frombuffer(b"".join(sq.row_roots), dtype=np.uint8).copy()
    change, text = INVALID[case]
    st = {"k": sq.k, "row_roots": roots}
    change(batch, st)
    b = batch.batch()
    for field, value in st.items():
        if field in ("k", "row_roots"):
            continue
        setattr(b, field, value)
    verdict = np.full(len(nss), 0xAA, dtype=np.uint8)
    rc = ctx.lib.cda_namespace_proofs_verify(ctx.h, st["k"], ptr(st["row_roots"]), C.byref(b), ptr(verdict))
    msg = ctx.lib.cda_last_error(ctx.h).decode()
    assert rc == _lib.CDA_ERR_INVALID, (case, rc, msg)
    assert text in msg, (case, msg)
    assert (verdict == 0xAA).all()
    # and the batch as it was verifies
    assert not NamespaceProofsBatch.from_answers(sq.k, nss, answers).verify(sq.row_roots, ctx).any()


@pytest.mark.gpu
def test_no_query_and_null_batch(ctx):
    sq = ref.squares()["hand"]
    assert len(NamespaceProofsBatch.from_answers(sq.k, [], []).verify(sq.row_roots, ctx)) == 0
    assert ctx.lib.cda_namespace_proofs_verify(ctx.h, sq.k, None, None, None) == _lib.CDA_ERR_INVALID
