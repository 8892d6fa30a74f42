"""Blob inclusion by share commitment on the GPU: cda_square_commitment_proofs
(csrc/share_proofs.hip), cda_commitment_proofs_verify (csrc/verify.hip) and
their Python surface (ResidentSquare.commitment_proofs, CommitmentProof,
validate_commitment_proofs, new_blob_commitment_proofs).

The yardstick is the CPU restatement tests/commitment_proof_ref.py, pinned in
tests/test_commitment_proof_ref.py by the oracle's GetCommitment and row roots;
block 408's proof is pinned by the ShareCommitment of the PFB in the reference's
fixture and by the block's DataHash.
"""
import ctypes as C

import numpy as np
import pytest

import commitment_proof_ref as ref
import coracle
import inclusion as oinc
import proofs as opr
import square as osq
from celestia_da import CdaError, PushOrderError, _lib, blobfactory
from celestia_da import proof as gpr
from celestia_da import square as gsquare

pytestmark = pytest.mark.gpu
# blob txs and blob sizes whose square.Construct is exactly k x k (seed 1)
BLOCKS = {1: (0, 1), 2: (1, 400), 4: (3, 1400), 8: (8, 3000), 16: (20, 6000), 32: (40, 12000)}
FIELDS = gpr.CommitmentProofsBatch.FIELDS


def block_txs(k):
    n, mx = BLOCKS[k]
    return blobfactory.random_block(1, 0 if k < 4 else 1, n, (1, 2), (1, mx)) if n else []


class Made:
    """One square per k for the whole module: the constructor's ODS, its blobs (start, share count) in PFB
    order, the resident square and the restatement's trees."""

    def __init__(self, ctx, k, ods=None):
        self.k = k
        if ods is None:
            txs = block_txs(k)
            sq = gsquare.construct(txs, k, 64, ctx=ctx)
            assert sq.size() == k
            ods = np.frombuffer(sq.to_bytes(), dtype=np.uint8)
            starts = gsquare.layout(txs, k, 64)[2]
            lens = [n for tx in txs for n, _ in (gpr.blob_tx_blobs(tx) or [])]
            assert len(starts) == len(lens)
            self.blobs = list(zip(starts, lens))
        self.ods = np.ascontiguousarray(ods).reshape(k * k, 512)
        self.sq = gpr.ResidentSquare(self.ods, ctx)
        self._trees = None

    @property
    def trees(self):
        if self._trees is None:
            self._trees = ref.RefTrees(self.ods)
        return self._trees


@pytest.fixture(scope="module")
def made(ctx):
    cache = {}

    def get(k, ods=None):
        if k not in cache:
            cache[k] = Made(ctx, k, ods() if ods else None)
        return cache[k]
    yield get
    for m in cache.values():
        m.sq.close()


def fits(k, start, share_len, thr):
    return share_len >= 1 and osq.next_share_index(start, share_len, thr) + share_len <= k * k


def cases(k, thr, blobs):
    """The blobs the issue names, where the square holds them, then the square's own blobs."""
    c = [(0, 1), (k * k - 1, 1),
         (k // 2, k // 2),              # ends exactly at a row end
         (k, 3 * k),                    # whole middle rows
         (k + k // 2, 2 * k + 1),       # three rows, both ends inside a row
         (0, 11), (16, 11),             # w = 4 at thresholds 1 and 2: 4, 4, 2, 1
         (0, k * k),                    # the whole square
         (1, 3), (1, 2), (k + 1, 5)]    # starts NextShareIndex moves
    return [b for b in c + list(blobs) if fits(k, *b, thr)]


def from_batch(batch):
    """The restatement's view of a batch the library filled."""
    out = []
    cut = lambda a, lo, hi: [a[i].tobytes() for i in range(lo, hi)]  # noqa: E731
    for i in range(len(batch)):
        rows = []
        for g in range(batch.seg_off[i], batch.seg_off[i + 1]):
            rows.append(ref.RefRow(int(batch.nmt_start[g]), int(batch.nmt_end[g]),
                                   cut(batch.nodes, batch.node_off[g], batch.node_off[g + 1]),
                                   cut(batch.subtree_roots, batch.root_off[g], batch.root_off[g + 1]),
                                   batch.row_roots[g].tobytes(), int(batch.rfc_total[g]), int(batch.rfc_index[g]),
                                   batch.rfc_leaf_hash[g].tobytes(),
                                   cut(batch.aunts, batch.aunt_off[g], batch.aunt_off[g + 1])))
        out.append(ref.RefProof(rows, batch.namespaces[i].tobytes(), int(batch.start_row[i]), int(batch.end_row[i]),
                                int(batch.norm_start[i])))
    return out


def assert_equals_restatement(batch, want, what):
    a = ref.flat_arrays(want)
    for name in FIELDS:
        got = getattr(batch, name)
        assert got.shape == a[name].shape and got.dtype == a[name].dtype, (what, name, got.shape, a[name].shape)
        assert np.array_equal(got, a[name]), (what, name)


# ------------------------------------------------------------------ 1. build parity
@pytest.mark.parametrize("thr", [1, 2, 64])
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16])
def test_build_equals_the_restatement(made, k, thr):
    m = made(k)
    blobs = cases(k, thr, m.blobs)
    if k >= 4 and thr in (1, 2):
        assert (0, 11) in blobs and osq.subtree_width(11, thr) == 4
    if (k >= 4 and thr in (1, 2)) or (k == 2 and thr == 1):
        assert any(osq.next_share_index(s, n, thr) != s for s, n in blobs)   # a start NextShareIndex moves
    starts, lens = [b[0] for b in blobs], [b[1] for b in blobs]
    out = gpr.CommitmentProofsBatch.empty(k, starts, lens, thr, fill=0xAA)
    batch = m.sq.commitment_proofs(starts, lens, thr, out=out)
    want = [ref.prove(m.trees.eds, k, s, n, thr, trees=m.trees) for s, n in blobs]
    assert_equals_restatement(batch, want, (k, thr))
    assert batch.commitments.tobytes() == b"".join(m.sq.blob_commitments(starts, lens, thr))
    assert batch.verify(m.trees.data_root).tolist() == [0] * len(blobs)
    # the objects carry the same bytes, and validate through the flat batch built from them
    objs = batch.proofs()
    for o, w in zip(objs, want):
        assert o.subtree_roots == w.subtree_roots() and o.namespace == w.namespace
        assert o.share_len == sum(r.end - r.start for r in w.rows)
    assert gpr.validate_commitment_proofs(objs, [m.trees.data_root] * len(objs), [ref.commitment(w) for w in want],
                                          thr) == [None] * len(objs)


def test_every_height_in_one_row(made):
    """11 shares with w = 4 in one row of k = 16: roots of 4, 4, 2 and 1 leaves."""
    m = made(16)
    batch = m.sq.commitment_proofs([32], [11], 2)
    assert batch.root_off.tolist() == [0, 4] and batch.seg_off.tolist() == [0, 1]
    w = ref.prove(m.trees.eds, 16, 32, 11, 2, trees=m.trees)
    assert [lv for lv, _ in w.rows[0].coords] == [2, 2, 1, 0]
    assert_equals_restatement(batch, [w], "11 of 16")


def test_empty_batch_and_null_outputs(made):
    m = made(4)
    batch = m.sq.commitment_proofs([], [], 64, out=gpr.CommitmentProofsBatch.empty(4, [], [], 64, fill=0xAA))
    assert batch.seg_off.tolist() == [0] and batch.root_off.tolist() == [0] and batch.node_off.tolist() == [0]
    assert batch.verify(m.trees.data_root).tolist() == []
    # any output may be NULL: the others are the same bytes
    starts, lens = [4, 0], [7, 16]
    full = m.sq.commitment_proofs(starts, lens, 2)
    for skip in (("commitments",), ("subtree_roots", "root_off"), ("nodes", "aunts", "rfc_leaf_hash", "namespaces"),
                 tuple(n for n in FIELDS if n != "commitments")):
        out = gpr.CommitmentProofsBatch.empty(4, starts, lens, 2, fill=0xAA)
        o = out.out_struct(skip=skip)
        u32p = C.POINTER(C.c_uint32)
        st, ln = np.array(starts, dtype=np.uint32), np.array(lens, dtype=np.uint32)
        m.sq.ctx.check(m.sq.ctx.lib.cda_square_commitment_proofs(m.sq.h, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p),
                                                                 2, 2, C.byref(o)))
        for name in FIELDS:
            got = getattr(out, name)
            if name in skip:
                assert (got.view(np.uint8) == 0xAA).all(), (skip, name)
            else:
                assert np.array_equal(got, getattr(full, name)), (skip, name)


def test_invalid_blobs_leave_the_outputs_untouched(made):
    m = made(4)
    out = gpr.CommitmentProofsBatch.empty(4, [0, 4], [1, 7], 64, fill=0xAA)
    for starts, lens, thr, text in (([0, 14], [1, 3], 64, "blob 1: start 14 (normalised 14) with share_len 3 ends beyond "
                                     "the 16 shares of the original square"),
                                    ([0, 3], [0, 1], 64, "blob 0: share_len is 0"),
                                    ([0, 3], [1, 1], 0, "subtree root threshold must be positive")):
        with pytest.raises(CdaError) as e:
            m.sq.commitment_proofs(starts, lens, thr, out=out)
        assert str(e.value) == text and e.value.code == _lib.CDA_ERR_INVALID
        assert all((a.view(np.uint8) == 0xAA).all() for a in out.arrays())


def test_push_order_square_answers_push_order(ctx, made):
    ods = made(4).ods[[5, 1, 9, 13]].copy()
    if bytes(ods[0, :29]) <= bytes(ods[1, :29]):
        ods = ods[[1, 0, 2, 3]].copy()
    assert bytes(ods[0, :29]) > bytes(ods[1, :29])
    sq = gpr.ResidentSquare(ods, ctx)
    try:
        assert sq.push_order_error
        out = gpr.CommitmentProofsBatch.empty(2, [0], [2], 64, fill=0xAA)
        with pytest.raises(PushOrderError) as e:
            sq.commitment_proofs([0], [2], 64, out=out)
        assert "no commitment proof" in str(e.value)
        assert all((a.view(np.uint8) == 0xAA).all() for a in out.arrays())
    finally:
        sq.close()


# ------------------------------------------------------------------ 2. block 408
def test_block408_blob_is_proven_by_its_pfb_commitment(ctx):
    from test_square import block408
    txs, _, data_hash = block408()
    # the ShareCommitment the reference's fixture carries, decoded by the oracle
    pfb = [c for t in txs if osq.unmarshal_blob_tx(t) for c in oinc.pfb_share_commitments(osq.unmarshal_blob_tx(t)[0])[0]]
    assert len(pfb) == 1
    got = gpr.new_blob_commitment_proofs(txs, ctx=ctx)
    assert len(got) == 1
    proof, claimed = got[0]
    assert claimed == pfb[0] and proof.share_len == 352
    assert proof.validate(data_hash, pfb[0], ctx=ctx) is None
    assert len(proof.subtree_roots) * 90 < 4096
    assert proof.validate(bytes(32), pfb[0], ctx=ctx) == gpr.ERR_ROW_PROOF
    assert proof.validate(data_hash, bytes(32), ctx=ctx) == gpr.ERR_COMMITMENT
    # the restatement agrees, from the proof's own bytes
    rows, at = [], 0
    w = osq.subtree_width(352, 64)
    for q, root, mp in zip(proof.subtree_root_proofs, proof.row_proof.row_roots, proof.row_proof.proofs):
        n = len(ref.cover(mp.total // 4, q.start, q.end, w))
        rows.append(ref.RefRow(q.start, q.end, q.nodes, proof.subtree_roots[at:at + n], root, mp.total, mp.index,
                               mp.leaf_hash, mp.aunts))
        at += n
    assert at == len(proof.subtree_roots)
    assert ref.verdict(ref.RefProof(rows, proof.namespace, 0, 0, 0), data_hash, pfb[0], 64) == ref.VALID


# ------------------------------------------------------------------ 3. the widest trees
@pytest.mark.parametrize("k,start,share_len", [(128, 3 * 128 + 50, 300), (512, 3 * 512 + 100, 1500)])
def test_wide_squares(made, k, start, share_len):
    """One multi-row blob of a k = 128 and of a k = 512 square (GF(2^16) rows, the deepest trees a block has),
    built and verified; the k = 128 one equals the restatement byte for byte, the k = 512 one is checked by the
    restatement's verdict on its own bytes, the square's DAH, its commitment and its cached subtree roots."""
    m = made(k, ods=lambda: coracle.random_square(k, 7 if k <= 128 else 0))
    batch = m.sq.commitment_proofs([start], [share_len], 64)
    rows, _, data_root = m.sq.dah()
    assert batch.seg_off[1] >= 3
    assert batch.commitments.tobytes() == m.sq.blob_commitments([start], [share_len], 64)[0]
    assert batch.verify(data_root).tolist() == [0]
    got = from_batch(batch)[0]
    assert [r.row_root for r in got.rows] == rows[got.start_row:got.end_row + 1]
    assert ref.verdict(got, data_root, batch.commitments.tobytes(), 64) == ref.VALID
    w = osq.subtree_width(share_len, 64)
    for r in (got.rows[0], got.rows[-1]):
        for (lv, ix), root in zip(ref.cover(k, r.start, r.end, w), r.roots):
            depth = (2 * k).bit_length() - 1 - lv
            assert m.sq.subtree_root(r.index, opr.subtree_root_path(depth, ix)) == root
    if k == 128:
        assert m.trees.data_root == data_root
        assert_equals_restatement(batch, [ref.prove(m.trees.eds, k, start, share_len, 64, trees=m.trees)], k)
    # a tampered copy fails where the restatement says
    bad = ref.flip_root_byte(got, row=1)
    assert gpu_verdicts(m.sq.ctx, [bad], [data_root], [ref.commitment(got)], 64) == [ref.SUBTREE_ROOTS]


def test_run_longer_than_a_fold_tile(made):
    """k = 128 with w = 1 (a threshold above the blob's share count): whole rows of 128 subtree roots, more
    than CDA_COMMITMENT_FOLD_TILE, with unaligned ends in the first and the last row."""
    m = made(128, ods=lambda: coracle.random_square(128, 7))
    start, share_len, thr = 128 + 63, 2 * 128 + 10, 1 << 20
    assert osq.subtree_width(share_len, thr) == 1
    batch = m.sq.commitment_proofs([start], [share_len], thr)
    assert np.diff(batch.root_off).tolist() == [65, 128, 73]
    assert_equals_restatement(batch, [ref.prove(m.trees.eds, 128, start, share_len, thr, trees=m.trees)], "w = 1")
    assert batch.verify(m.trees.data_root).tolist() == [0]
    got = from_batch(batch)[0]
    tampered = [ref.flip_root_byte(got, row=1, i=64), ref.flip_root_byte(got, row=1, i=127),
                ref.flip_root_byte(got, row=0, i=0), ref.flip_root_byte(got, row=2, i=72)]
    assert gpu_verdicts(m.sq.ctx, tampered, [m.trees.data_root] * 4, [ref.commitment(got)] * 4, thr) == [2] * 4


# ------------------------------------------------------------------ 4. verdicts
def c_batch(proofs, data_roots, commitments, thr, edit=None):
    """The cda_commitment_proof_batch of the restatement's proofs; edit(arrays) changes the arrays first."""
    a = ref.flat_arrays(proofs)
    a["data_roots"] = np.frombuffer(b"".join(data_roots), dtype=np.uint8).copy()
    a["claimed"] = np.frombuffer(b"".join(commitments), dtype=np.uint8).copy()
    counts = {"n_nodes": len(a["nodes"]), "n_roots": len(a["subtree_roots"]), "n_aunts": len(a["aunts"])}
    if edit:
        edit(a, counts)
    b = _lib.CommitmentProofBatch()
    b.n_proofs, b.ns_len, b.threshold = len(proofs), 29, thr
    for name, t in _lib.CommitmentProofBatch._fields_:
        src = {"commitments": "claimed"}.get(name, name)
        if src in a:
            arr = a[src] if a[src].size else np.zeros(1, dtype=a[src].dtype)
            a[src] = arr
            setattr(b, name, arr.ctypes.data_as(t))
    b.n_nodes, b.n_roots, b.n_aunts = counts["n_nodes"], counts["n_roots"], counts["n_aunts"]
    b._keep = a
    return b


def gpu_verdicts(ctx, proofs, data_roots, commitments, thr, edit=None):
    b = c_batch(proofs, data_roots, commitments, thr, edit)
    verdict = np.full(max(1, len(proofs)), 0xAA, dtype=np.uint8)
    ctx.check(ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), verdict.ctypes.data_as(C.POINTER(C.c_uint8))))
    return verdict[:len(proofs)].tolist()


def verdict_entries(made):
    """(proof, data root, claimed commitment) of one batch at threshold 8: valid proofs of three widths and
    every tampering, and what each is expected to be."""
    thr = 8
    t2, t8, t32 = made(2).trees, made(8).trees, made(32).trees
    p2 = ref.prove(t2.eds, 2, 1, 3, thr, trees=t2)
    p8 = ref.prove(t8.eds, 8, 24, 22, thr, trees=t8)          # rows 3, 4, 5 with w = 4
    p8b = ref.prove(t8.eds, 8, 8, 11, thr, trees=t8)          # w = 2
    p32 = ref.prove(t32.eds, 32, 32 * 5 + 16, 100, thr, trees=t32)
    assert osq.subtree_width(22, thr) == 4 and [r.index for r in p8.rows] == [3, 4, 5]
    c2, c8, c8b, c32 = (ref.commitment(p) for p in (p2, p8, p8b, p32))
    e = [(p2, t2.data_root, c2, 0), (p8, t8.data_root, c8, 0), (p32, t32.data_root, c32, 0), (p8b, t8.data_root, c8b, 0),
         (p8, t32.data_root, c8, 1),                                          # wrong data root
         (ref.flip_root_byte(p8, row=1), t8.data_root, c8, 2),
         (ref.flip_root_byte(p32, row=len(p32.rows) - 1, i=-1), t32.data_root, c32, 2),
         (ref.swap_equal_roots(p8, row=0), t8.data_root, c8, 2),
         (ref.split_root(p8, t8, row=2), t8.data_root, c8, 2),                # count only
         (ref.split_root(p32, t32, row=0), t32.data_root, c32, 2),
         (ref.drop_node(p8, row=1), t8.data_root, c8, 2),
         (ref.extra_node(p8, row=2), t8.data_root, c8, 2),
         (p8, t8.data_root, c8b, 3),                                          # a right commitment, another blob's
         (ref.drop_row(p8, 1), t8.data_root, c8, 4),                          # rows 3 and 5 without 4
         (ref.shift_start(p8b), t8.data_root, c8b, 4),                        # first nmt_start no multiple of w
         (ref.change_total(p8), t8.data_root, c8, 4),                         # rfc_total differs inside the proof
         (ref.change_total(ref.flip_root_byte(p8)), t32.data_root, c8b, 4),   # 4 wins over all
         (ref.flip_root_byte(p8), t32.data_root, c8b, 1),                     # then the lowest number
         (ref.flip_root_byte(p8), t8.data_root, c8b, 2),
         (p2, t2.data_root, c2, 0)]
    return thr, e


def test_verdicts_of_a_mixed_batch(ctx, made):
    thr, entries = verdict_entries(made)
    want = [ref.verdict(p, root, c, thr) for p, root, c, _ in entries]
    assert want == [x[3] for x in entries]
    got = gpu_verdicts(ctx, [x[0] for x in entries], [x[1] for x in entries], [x[2] for x in entries], thr)
    assert got == want
    # each alone too: no entry leans on its neighbours
    for p, root, c, v in entries[4:16]:
        assert gpu_verdicts(ctx, [p], [root], [c], thr) == [v]


def test_objects_validate_like_the_batch(ctx, made):
    """validate_commitment_proofs deals the flat subtree roots to the rows by the cover's counts: every entry
    whose rows still say where its roots belong gets the batch's verdict."""
    thr, entries = verdict_entries(made)
    objs = []
    for p, _, _, _ in entries:
        objs.append(gpr.CommitmentProof(
            p.subtree_roots(), [gpr.NMTProof(r.start, r.end, r.nodes) for r in p.rows], p.namespace,
            gpr.RowProof([r.row_root for r in p.rows], [gpr.Proof(r.total, r.index, r.leaf_hash, r.aunts) for r in p.rows],
                         p.start_row, p.end_row)))
    got = gpr.validate_commitment_proofs(objs, [x[1] for x in entries], [x[2] for x in entries], thr, ctx)
    assert got == [gpr.COMMITMENT_VERDICT_TEXT[x[3]] for x in entries]


def test_malformed_offsets_are_errors_not_verdicts(ctx, made):
    thr, entries = verdict_entries(made)
    proofs, roots, claimed = ([x[i] for x in entries[:4]] for i in range(3))

    def setter(name, i, v):
        def edit(a, counts):
            a[name][i] = v
        return edit

    def count(name, d):
        def edit(a, counts):
            counts[name] += d
        return edit
    bad = [(setter("seg_off", 0, 1), "seg_off must start at 0"), (setter("seg_off", 2, 0), "seg_off decreases"),
           (setter("root_off", 0, 1), "root_off must start at 0"), (setter("root_off", 2, 0), "root_off decreases"),
           (setter("node_off", 0, 1), "node_off must start at 0"), (setter("node_off", 3, 0), "node_off decreases"),
           (setter("aunt_off", 0, 1), "aunt_off must start at 0"), (setter("aunt_off", 3, 1), "aunt_off decreases"),
           (count("n_roots", 1), "root_off ends at"), (count("n_nodes", -1), "node_off ends at"),
           (count("n_aunts", 1), "aunt_off ends at"),
           (setter("nmt_start", 1, -1), "nmt_start -1 is negative"), (setter("nmt_end", 1, 0), "is not above nmt_start"),
           (setter("nmt_end", 2, 2049), "nmt_end 2049 exceeds 2048")]
    for edit, text in bad:
        b = c_batch(proofs, roots, claimed, thr, edit)
        verdict = np.full(len(proofs), 0xAA, dtype=np.uint8)
        rc = ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), verdict.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == _lib.CDA_ERR_INVALID, text
        assert text in ctx.lib.cda_last_error(ctx.h).decode(), text
        assert (verdict == 0xAA).all(), text
    for field, value, text in (("ns_len", 33, "ns_len 33 is not 29"), ("threshold", 0, "threshold must be positive")):
        b = c_batch(proofs, roots, claimed, thr)
        setattr(b, field, value)
        verdict = np.full(len(proofs), 0xAA, dtype=np.uint8)
        rc = ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), verdict.ctypes.data_as(C.POINTER(C.c_uint8)))
        assert rc == _lib.CDA_ERR_INVALID and text in ctx.lib.cda_last_error(ctx.h).decode()
        assert (verdict == 0xAA).all()
    assert gpu_verdicts(ctx, proofs, roots, claimed, thr) == [0] * 4


# ------------------------------------------------------------------ 5. launch counts
def test_launch_counts_do_not_grow_with_the_batch(ctx, made):
    m = made(16)
    blobs = [(s, 4) for s in range(0, 256, 4)]
    assert len(blobs) == 64
    ctx.set_profiling(True)
    try:
        ctx.stage_times()
        counts = {}
        for n in (1, 64):
            batch = m.sq.commitment_proofs([b[0] for b in blobs[:n]], [b[1] for b in blobs[:n]], 64)
            built = ctx.stage_times()
            assert batch.verify(m.trees.data_root).tolist() == [0] * n
            verified = ctx.stage_times()
            counts[n] = (built["commitment_proofs"][1], built["commitment_proofs_verify"][1],
                         verified["commitment_proofs"][1], verified["commitment_proofs_verify"][1])
            # without the commitments: the one launch of the proof kernel
            out = gpr.CommitmentProofsBatch.empty(16, [b[0] for b in blobs[:n]], [b[1] for b in blobs[:n]], 64)
            o = out.out_struct(skip=("commitments",))
            st = np.array([b[0] for b in blobs[:n]], dtype=np.uint32)
            ln = np.array([b[1] for b in blobs[:n]], dtype=np.uint32)
            u32p = C.POINTER(C.c_uint32)
            ctx.check(ctx.lib.cda_square_commitment_proofs(m.sq.h, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p), n, 64,
                                                           C.byref(o)))
            assert ctx.stage_times()["commitment_proofs"][1] == 1
        assert counts[1] == counts[64] == (2, 0, 0, 4)
    finally:
        ctx.set_profiling(False)
