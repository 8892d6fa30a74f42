"""The CPU yardstick of the bad-encoding fraud proofs (tests/befp_ref.py) on the test squares: the verdicts the
protocol text demands, before anything is compared with the GPU (tests/test_befp.py)."""
import numpy as np
import pytest

import befp_ref as ref
import pyref

K = 2   # every index of every axis below; the GPU file replays the cases at k = 2 and 8


def test_honest_square_every_vector_matches_its_root():
    sq = ref.honest_square(K)
    W = 2 * K
    for axis in (ref.ROW, ref.COL):
        for index in range(W):
            full = ref.prove(sq, axis, index, range(W))
            v, root = ref.validate(full, sq.rows, sq.cols)
            assert v == ref.ROOT_MATCHES and root == (sq.rows if axis == ref.ROW else sq.cols)[index]
            for half in (range(K), range(K, W)):
                v, root = ref.validate(full.at(half), sq.rows, sq.cols)
                assert v == ref.ROOT_MATCHES and root == (sq.rows if axis == ref.ROW else sq.cols)[index]


def test_malicious_square_commits_two_non_codewords():
    k = 4
    sq = ref.malicious_square(k)
    r, c = ref.flipped_cell(k)
    assert r < k <= c
    for axis in (ref.ROW, ref.COL):
        for i in range(2 * k):
            v = sq.vector(axis, i)
            sound = np.array_equal(pyref.leopard_encode(v[:k]), v[k:])
            assert sound == ((axis, i) not in ((ref.ROW, r), (ref.COL, c)))
            assert pyref.axis_root(v, k, i) == (sq.rows if axis == ref.ROW else sq.cols)[i]


@pytest.mark.parametrize("k", [2, 4])
def test_cases_give_the_stated_verdicts(k):
    seen = set()
    for name, proof, rows, cols, want in ref.cases(k):
        v, root = ref.validate(proof, rows, cols)
        assert v == want, name
        assert (root == bytes(90)) == (v in (ref.TOO_FEW, ref.NOT_INCLUDED)), name
        seen.add(v)
    assert seen == {0, 1, 2, 3}
    assert len(ref.cases(k)) >= 9


def test_rebuilt_root_of_an_unordered_vector_is_the_blind_one():
    k = 4
    sq, row = ref.unordered_square(k)
    with pytest.raises(pyref.PushOrderError):
        pyref.axis_root(sq.eds[row], k, row)
    v, root = ref.validate(ref.prove(sq, ref.ROW, row, range(2 * k)), sq.rows, sq.cols)
    assert v == ref.VALID and root == sq.rows[row]   # equal roots, and still a fraud: the push order


def test_builder_emits_every_cell_of_a_whole_square_and_skips_holes():
    k = 2
    sq = ref.malicious_square(k)
    r, _ = ref.flipped_cell(k)
    p = ref.build(sq.eds, sq.rows, sq.cols, ref.ROW, r)
    assert p.positions.tolist() == list(range(2 * k)) and (p.proof_axes == ref.COL).all()
    assert ref.validate(p, sq.rows, sq.cols)[0] == ref.VALID
    eds = sq.eds.copy()
    eds[0, 2] = 0   # a hole in column 2, off the accused row
    assert r != 0
    p = ref.build(eds, sq.rows, sq.cols, ref.ROW, r)
    assert p.positions.tolist() == [0, 1, 3]
    assert ref.validate(p, sq.rows, sq.cols)[0] == ref.VALID
