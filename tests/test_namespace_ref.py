"""The CPU restatement of the namespace query (tests/nmt_namespace_ref.py) against itself and against the
oracle: the squares hold every kind of answer, every honest answer verifies, and every tampered answer gets
the verdict it must.  No GPU.  Completeness and absence are pinned by this restatement only; inclusion
segments also pass the oracle's nmt_verify_inclusion.
"""
import pytest

import coracle
import nmt_namespace_ref as ref
import proofs as opr

NAMES = ("small1", "small2", "small4", "small8", "hand")


def test_hand_made_square_answers_b_with_absence_and_inclusion():
    sq = ref.squares()["hand"]
    a, c, b, d = (x[:29].tobytes() for x in sq.ods)
    assert a < b < c < d and sq.k == 2
    ans = ref.get_shares_by_namespace(sq, b)
    assert [(r, p.start, p.end, bool(p.leaf_hash), len(sh)) for r, p, sh in ans] == [(0, 1, 2, True, 0),
                                                                                    (1, 0, 1, False, 1)]
    assert ans[0][1].leaf_hash == sq.leaves[0][1] and ans[1][2] == [sq.ods[2].tobytes()]


def test_inventory_holds_every_kind():
    found = {}
    for name in NAMES:
        sq = ref.squares()[name]
        for ns, ans in ref.honest(name):
            for kind in ref.kinds_of(sq, ns, ans):
                found.setdefault(kind, (name, ns.hex()))
    assert set(found) == set(ref.KINDS), sorted(set(ref.KINDS) - set(found))


@pytest.mark.parametrize("name", NAMES)
def test_honest_answers_verify(name):
    sq = ref.squares()[name]
    assert sq.row_roots == [bytes(r) for r in coracle.extend_dah(sq.ods)[1]]   # the C oracle's roots
    for ns, ans in ref.honest(name):
        assert ref.answer_verdict(sq.row_roots, ns, ans) == 0, ns.hex()
        assert [r for r, _, _ in ans] == sorted(r for r, _, _ in ans) and all(r < sq.k for r, _, _ in ans)
        for r, p, shares in ans:
            if p.leaf_hash:
                assert not shares and p.end == p.start + 1 < sq.k + 1 and p.leaf_hash[:29] > ns
                assert opr.nmt_verify_range(sq.row_roots[r], p.nodes, p.start, p.end, 2 * sq.k, [p.leaf_hash])
            else:
                assert all(s[:29] == ns for s in shares) and len(shares) == p.end - p.start
                assert opr.nmt_verify_inclusion(sq.row_roots[r], p.nodes, p.start, p.end, ns, shares)
        # all the shares of the namespace, and no others
        assert [s for _, _, sh in ans for s in sh] == [x.tobytes() for x in sq.ods if x[:29].tobytes() == ns]


def test_every_tamper_is_made_and_rejected_with_its_verdict():
    seen = set()
    for name in NAMES:
        sq = ref.squares()[name]
        for label, ns, ans, want in ref.tampers(name):
            assert ref.answer_verdict(sq.row_roots, ns, ans) == want, (name, label, ns.hex())
            seen.add(label)
    assert seen == set(ref.TAMPER_LABELS), sorted(set(ref.TAMPER_LABELS) - seen)


def test_precedence():
    """The lower verdict wins: a dropped row beside a flipped share is 1, a flipped share beside an incomplete
    segment 2."""
    got = {label: want for name in NAMES for label, _, _, want in ref.tampers(name)}
    assert got["drop_and_flip"] == 1 and got["flip_and_incomplete"] == 2
