"""The CPU restatement of the blob commitment proof (tests/commitment_proof_ref.py)
pinned by construction, its verdicts on every tampering the GPU tests use, and
the Python model of the fold kernel's tiling at the tile's boundary.  CPU only.

Pins: the Merkle root of the subtree roots `prove` emits equals the oracle's
get_commitment (inclusion.GetCommitment, itself pinned by block 408's PFB), and
every row of every proof folds to the oracle's row root.
"""
import pytest

import commitment_proof_ref as ref
import coracle
import proofs as opr
import square as osq


@pytest.fixture(scope="module")
def trees():
    return {k: ref.RefTrees(coracle.random_square(k, 3)) for k in (2, 4, 8)}


def aligned_blobs(k, thr):
    for share_len in range(1, k * k + 1):
        w = osq.subtree_width(share_len, thr)
        for start in range(0, k * k - share_len + 1, w):
            yield start, share_len


@pytest.mark.parametrize("k,step", [(2, 1), (4, 1), (8, 5)])
@pytest.mark.parametrize("thr", [1, 2, 64])
def test_restatement_pinned_by_commitment_and_row_roots(trees, k, thr, step):
    """Every aligned blob of k = 2 and 4, every fifth of k = 8 (and its first and last)."""
    t = trees[k]
    blobs = list(aligned_blobs(k, thr))
    for start, share_len in blobs[::step] + blobs[-1:]:
        p = ref.prove(t.eds, k, start, share_len, thr, trees=t)
        w = osq.subtree_width(share_len, thr)
        assert ref.commitment(p) == opr.get_commitment(t.eds, k, start, share_len, thr), (start, share_len)
        assert p.norm_start == start and [r.index for r in p.rows] == list(range(p.start_row, p.end_row + 1))
        for r in p.rows:
            assert r.row_root == t.row_roots[r.index]
            assert ref.fold_row(r, k, w), (start, share_len, r.index)
            assert opr.rfc_verify(t.data_root, 4 * k, r.index, r.leaf_hash, r.aunts)
        assert ref.verdict(p, t.data_root, ref.commitment(p), thr) == ref.VALID


def test_start_is_normalised(trees):
    t = trees[4]
    assert osq.subtree_width(3, 1) == 2
    p = ref.prove(t.eds, 4, 1, 3, 1, trees=t)
    assert p.norm_start == 2 and [(r.start, r.end) for r in p.rows] == [(2, 4), (0, 1)]
    assert ref.commitment(p) == opr.get_commitment(t.eds, 4, 1, 3, 1)


def test_verdict_on_every_tampering(trees):
    t, thr = trees[8], 8
    assert osq.subtree_width(22, thr) == 4 and osq.subtree_width(11, thr) == 2
    p = ref.prove(t.eds, 8, 24, 22, thr, trees=t)        # rows 3, 4, 5: [0, 8) [0, 8) [0, 6)
    other = ref.prove(t.eds, 8, 0, 5, thr, trees=t)
    good = ref.commitment(p)
    assert [r.index for r in p.rows] == [3, 4, 5] and ref.verdict(p, t.data_root, good, thr) == ref.VALID
    v = lambda q, root=t.data_root, c=good: ref.verdict(q, root, c, thr)  # noqa: E731
    assert v(p, root=bytes(32)) == ref.ROW_PROOF
    assert v(ref.flip_root_byte(p, row=1)) == ref.SUBTREE_ROOTS
    assert v(ref.swap_equal_roots(p, row=0)) == ref.SUBTREE_ROOTS
    split = ref.split_root(p, t, row=2)
    assert len(split.rows[2].roots) == len(p.rows[2].roots) + 1 and v(split) == ref.SUBTREE_ROOTS
    assert v(ref.drop_node(p, row=1)) == ref.SUBTREE_ROOTS
    assert v(ref.extra_node(p, row=2)) == ref.SUBTREE_ROOTS
    assert v(p, c=ref.commitment(other)) == ref.COMMITMENT
    assert v(ref.drop_row(p, 1)) == ref.NOT_A_BLOB                  # rows 3 and 5 without 4
    shifted = ref.prove(t.eds, 8, 8, 11, thr, trees=t)
    assert v(ref.shift_start(shifted), c=ref.commitment(shifted)) == ref.NOT_A_BLOB
    assert v(ref.change_total(p)) == ref.NOT_A_BLOB
    # the lowest number wins, but for 4
    both = ref.flip_root_byte(p)
    assert v(both, root=bytes(32)) == ref.ROW_PROOF and v(both, c=bytes(32)) == ref.SUBTREE_ROOTS
    assert v(ref.change_total(both), root=bytes(32)) == ref.NOT_A_BLOB
    # the split pair hashes to the root it replaced: only the count catches it
    import pyref
    i = next(i for i, (a, b) in enumerate(zip(split.rows[2].roots, p.rows[2].roots)) if a != b)
    assert pyref.nmt_hash_node(*split.rows[2].roots[i:i + 2]) == p.rows[2].roots[i]


def test_flat_arrays_round_trip(trees):
    t = trees[4]
    proofs = [ref.prove(t.eds, 4, s, n, 1, trees=t) for s, n in ((0, 1), (4, 7), (15, 1))]
    a = ref.flat_arrays(proofs)
    assert a["seg_off"].tolist() == [0, 1, 3, 4] and a["root_off"][-1] == len(a["subtree_roots"])
    assert a["node_off"][-1] == len(a["nodes"]) and a["aunt_off"].tolist() == [0, 4, 8, 12, 16]
    assert a["norm_start"].tolist() == [0, 4, 15] and a["rfc_total"].tolist() == [16] * 4


# ------------------------------------------------------------------ the fold kernel's tiling
def _sym_hash(left, right):
    """Nodes as (level, index): only the two children of one parent hash."""
    assert left[0] == right[0] and left[1] % 2 == 0 and right[1] == left[1] + 1, (left, right)
    return (left[0] + 1, left[1] // 2)


def _sym_proof(k, s0, e0, w):
    D = (2 * k).bit_length() - 1
    roots = ref.cover(k, s0, e0, w)
    nodes = []
    for L in range(D - 1, -1, -1):          # tree_index.h range_proof_node: left top down, right bottom up
        if (s0 >> L) & 1:
            nodes.append((L, (s0 >> L) - 1))
    for L in range(D):
        if not ((e0 - 1) >> L) & 1:
            nodes.append((L, ((e0 - 1) >> L) + 1))
    return roots, nodes, D


def _model(k, s0, e0, w, trace=None, roots=None, nodes=None):
    r, n, D = _sym_proof(k, s0, e0, w)
    return ref.fold_model(r if roots is None else roots, n if nodes is None else nodes, s0, e0,
                          w.bit_length() - 1, D, _sym_hash, trace)


def test_fold_model_every_aligned_range_of_small_rows():
    for k in (1, 2, 4, 8, 16, 32):
        D = (2 * k).bit_length() - 1
        w = 1
        while w <= k:
            for s0 in range(0, k, w):
                for e0 in range(s0 + 1, k + 1):
                    assert _model(k, s0, e0, w) == (D, 0), (k, w, s0, e0)
            w *= 2


TILE = ref.FOLD_TILE


@pytest.mark.parametrize("k,w,s0,e0,tiles", [
    (1024, 1, 0, TILE, 0), (1024, 1, 0, TILE + 1, 2), (1024, 1, 1, TILE + 1, 0), (1024, 1, 1, TILE + 2, 2),
    (1024, 1, TILE - 1, 2 * TILE - 1, 0), (1024, 1, TILE - 1, 2 * TILE, 2), (1024, 1, TILE, 2 * TILE + 1, 2),
    (1024, 1, 0, 1024, 16), (1024, 1, 1, 1024, 16), (1024, 1, 63, 1023, 16), (1024, 1, 0, 1023, 16),
    (1024, 2, 0, 2 * TILE, 0), (1024, 2, 0, 2 * TILE + 1, 2),      # the carry is the tile's 65th node
    (1024, 2, 2, 2 * TILE + 1, 0), (1024, 2, 2, 2 * TILE + 3, 2), (1024, 4, 4, 1023, 4), (1024, 8, 8, 529, 2),
    (128, 1, 0, 128, 2), (128, 1, 5, 70, 2), (128, 1, 5, 69, 0), (512, 1, 130, 200, 2), (512, 1, 127, 193, 3),
])
def test_fold_model_at_the_tile_boundary(k, w, s0, e0, tiles):
    """A run of at most FOLD_TILE nodes folds in one piece; one node more and it folds in aligned tiles, whose
    nodes are the final fold's run.  The counts of every stage are asserted inside the model."""
    trace = []
    D = (2 * k).bit_length() - 1
    assert _model(k, s0, e0, w, trace) == (D, 0)
    assert [t[0] for t in trace] == ["tile"] * tiles + ["final"]
    for kind, first, count in trace[:-1]:
        assert 1 <= count <= TILE and (first + count - 1) // TILE == first // TILE   # inside one aligned tile
    if tiles:
        assert sum(t[2] for t in trace[:-1]) == (e0 - s0) // w + (1 if (e0 - s0) % w else 0)
        assert trace[-1][2] == tiles
    # what the kernel fails without reading: a count that is not the cover's or the range's
    roots, nodes, _ = _sym_proof(k, s0, e0, w)
    assert _model(k, s0, e0, w, roots=roots + roots[-1:]) is None
    assert _model(k, s0, e0, w, roots=roots[:-1]) is None
    assert _model(k, s0, e0, w, nodes=nodes[:-1]) is None
    assert _model(k, s0, e0, w, nodes=nodes + nodes[-1:]) is None


def test_fold_model_on_real_nodes(trees):
    """The model with the oracle's hash rebuilds the oracle's row roots."""
    import pyref
    t, k = trees[8], 8
    for thr, start, share_len in ((1, 8, 13), (2, 24, 22), (64, 3, 40), (1, 0, 64)):
        p = ref.prove(t.eds, k, start, share_len, thr, trees=t)
        w = osq.subtree_width(share_len, thr)
        for r in p.rows:
            got = ref.fold_model(r.roots, r.nodes, r.start, r.end, w.bit_length() - 1, 4, pyref.nmt_hash_node)
            assert got == r.row_root, (thr, start, share_len, r.index)
