"""CPU restatement of the blob commitment proof -- TEST INFRASTRUCTURE ONLY.

Restates, from their published algorithms and on top of the oracle's own
pieces only (proofs.subtree_root_coords / walk_subtree_root / nmt_range_proof /
rfc_aunts / rfc_verify / merkle_proof_verify, pyref.nmt_hash_node /
merkle_root):
  * celestia-node's blob.CommitmentProof of a blob (start, share_len): per row
    the subtree roots the share commitment is the Merkle root of, the nodes of
    nmt ProveRange over the row's range, the row roots and their proofs
                                                        -> prove
  * nmt v0.22.0 Proof.VerifySubtreeRootInclusion per row (the subtree roots
    and the nodes rebuild the row root: the usual recursion over [0, 2k), a
    span equal to the next cover element pops a subtree root, a span outside
    the range pops a node), RowProof.Validate and the commitment, as the four
    verdicts of cda_commitment_proofs_verify in its order
                                                        -> verdict
and the tamperings, the flat arrays and the Python model of the fold kernel's
tiling that the commitment proof tests share.  No vector of celestia-node or
nmt pins this file; what pins it is proofs.get_commitment (pinned by block
408's PFB) and the oracle's row roots (tests/test_commitment_proof_ref.py).
"""
import copy
from dataclasses import dataclass, field

import numpy as np

import coracle
import proofs as opr
import pyref
import square as osq

NS = 29


def log2(x: int) -> int:
    assert x > 0 and x & (x - 1) == 0, x
    return x.bit_length() - 1


@dataclass
class RefRow:
    start: int
    end: int
    nodes: list
    roots: list          # the row's subtree roots, left to right
    row_root: bytes
    total: int
    index: int
    leaf_hash: bytes
    aunts: list
    coords: list = field(default_factory=list)   # (level, index) of every root: not part of the proof


@dataclass
class RefProof:
    rows: list
    namespace: bytes
    start_row: int
    end_row: int
    norm_start: int

    def subtree_roots(self):
        return [r for row in self.rows for r in row.roots]


class RefTrees:
    """One square as the restatement sees it: the oracle's EDS and DAH, the leaf nodes of its row trees on demand."""

    def __init__(self, ods):
        ods = np.ascontiguousarray(ods, dtype=np.uint8).reshape(-1, 512)
        self.k = int(round(len(ods) ** 0.5))
        assert self.k * self.k == len(ods)
        W = 2 * self.k
        eds, rows, cols, root = coracle.extend_dah(ods)
        self.eds = np.asarray(eds).reshape(W, W, 512)
        self.row_roots = [bytes(r) for r in rows]
        self.col_roots = [bytes(c) for c in cols]
        self.data_root = bytes(root)
        self._leaves = {}

    def leaves(self, r):
        if r not in self._leaves:
            self._leaves[r] = pyref.erasured_leaves([x.tobytes() for x in self.eds[r]], self.k, r)
        return self._leaves[r]

    def node(self, r, level, index):
        """Node `index` of level `level` of row tree r."""
        return pyref.nmt_root_from_nodes(self.leaves(r)[index << level:(index + 1) << level])


def cover(k: int, s0: int, e0: int, w: int):
    """The subtree roots of the leaf range [s0, e0) of a row as (level, index) of the row tree, from the
    oracle's subtree_root_coords (depths count down from the k leaves of the ODS half)."""
    max_depth = log2(k)
    return [(max_depth - d, pos) for d, pos in opr.subtree_root_coords(max_depth, max_depth - log2(w), s0, e0)]


def blob_rows(k: int, start: int, share_len: int, threshold: int):
    """(normalised start, w, [(row, s0, e0)]) of a blob."""
    w = osq.subtree_width(share_len, threshold)
    start = osq.next_share_index(start, share_len, threshold)
    end = start + share_len
    assert end <= k * k
    r0, r1 = start // k, (end - 1) // k
    return start, w, [(r, start % k if r == r0 else 0, (end - 1) % k + 1 if r == r1 else k) for r in range(r0, r1 + 1)]


def prove(eds, k: int, start: int, share_len: int, threshold: int = 64, trees: RefTrees = None) -> RefProof:
    """The commitment proof of blob (start, share_len).  eds: the (2k, 2k, 512) square; trees: a RefTrees of
    the same square to share its hashing among calls."""
    if trees is None:
        trees = RefTrees(np.asarray(eds).reshape(2 * k, 2 * k, 512)[:k, :k])
    assert trees.k == k
    start, w, rows = blob_rows(k, start, share_len, threshold)
    all_roots = trees.row_roots + trees.col_roots
    out = []
    for r, s0, e0 in rows:
        leaves = trees.leaves(r)
        coords = cover(k, s0, e0, w)
        # the oracle's own walk from the row root, WalkLeft first (the ODS half), as get_commitment does
        roots = [opr.walk_subtree_root(leaves, [opr.WALK_LEFT] + opr.subtree_root_path(log2(k) - lv, ix))
                 for lv, ix in coords]
        leaf_hash, aunts = opr.rfc_aunts(all_roots, r)
        out.append(RefRow(s0, e0, opr.nmt_range_proof(leaves, s0, e0), roots, trees.row_roots[r], 4 * k, r,
                          leaf_hash, aunts, coords))
    return RefProof(out, trees.eds[rows[0][0], rows[0][1], :NS].tobytes(), rows[0][0], rows[-1][0], start)


def commitment(proof: RefProof) -> bytes:
    return pyref.merkle_root(proof.subtree_roots())


def fold_row(row: RefRow, k: int, w: int) -> bool:
    """The subtree roots and the nodes rebuild the row root."""
    if row.start % w or row.end > k:
        return False
    spans = [(ix << lv, (ix + 1) << lv) for lv, ix in cover(k, row.start, row.end, w)]
    if len(row.roots) != len(spans):
        return False
    roots, nodes = list(row.roots), list(row.nodes)

    def rec(lo, hi):
        if hi <= row.start or lo >= row.end:
            return nodes.pop(0)
        if spans and (lo, hi) == spans[0]:
            spans.pop(0)
            return roots.pop(0)
        assert hi - lo > 1
        mid = lo + opr.split_point(hi - lo)
        left = rec(lo, mid)
        return pyref.nmt_hash_node(left, rec(mid, hi))

    try:
        got = rec(0, 2 * k)
    except IndexError:      # too few nodes
        return False
    return not nodes and not roots and got == row.row_root


VALID, ROW_PROOF, SUBTREE_ROOTS, COMMITMENT, NOT_A_BLOB = 0, 1, 2, 3, 4


def verdict(proof: RefProof, data_root: bytes, claimed: bytes, threshold: int = 64) -> int:
    """cda_commitment_proofs_verify's verdict: 4 is decided first, then the lowest number wins."""
    rows = proof.rows
    if not rows:
        return NOT_A_BLOB
    total = rows[0].total
    k = total // 4
    if total <= 0 or total % 4 or k & (k - 1) or k > 1024:
        return NOT_A_BLOB
    for j, r in enumerate(rows):
        if r.total != total or not 0 <= r.index < k or r.index != rows[0].index + j:
            return NOT_A_BLOB
        if (j > 0 and r.start != 0) or (j + 1 < len(rows) and r.end != k) or r.end > k:
            return NOT_A_BLOB
    w = osq.subtree_width(sum(r.end - r.start for r in rows), threshold)
    if rows[0].start % w:
        return NOT_A_BLOB
    for r in rows:
        if not opr.merkle_proof_verify(data_root, r.total, r.index, r.leaf_hash, r.aunts, r.row_root):
            return ROW_PROOF
    for r in rows:
        if not fold_row(r, k, w):
            return SUBTREE_ROOTS
    if commitment(proof) != claimed:
        return COMMITMENT
    return VALID


# ------------------------------------------------------------------ tamperings
def _edit(proof: RefProof) -> RefProof:
    return copy.deepcopy(proof)


def flip_root_byte(proof, row=0, i=0, byte=40):
    p = _edit(proof)
    r = bytearray(p.rows[row].roots[i])
    r[byte] ^= 1
    p.rows[row].roots[i] = bytes(r)
    return p


def swap_equal_roots(proof, row=0):
    """Two neighbouring subtree roots of equal height change places."""
    p = _edit(proof)
    c = p.rows[row].coords
    i = next(i for i in range(len(c) - 1) if c[i][0] == c[i + 1][0])
    rt = p.rows[row].roots
    assert rt[i] != rt[i + 1]
    rt[i], rt[i + 1] = rt[i + 1], rt[i]
    return p


def split_root(proof, trees: RefTrees, row=0):
    """A subtree root of height >= 1 is replaced by its two children: the row root still rebuilds, the count
    is not the cover's."""
    p = _edit(proof)
    rw = p.rows[row]
    i = next(i for i, (lv, _) in enumerate(rw.coords) if lv >= 1)
    lv, ix = rw.coords[i]
    kids = [trees.node(rw.index, lv - 1, 2 * ix), trees.node(rw.index, lv - 1, 2 * ix + 1)]
    assert pyref.nmt_hash_node(*kids) == rw.roots[i]
    rw.roots[i:i + 1] = kids
    rw.coords[i:i + 1] = [(lv - 1, 2 * ix), (lv - 1, 2 * ix + 1)]
    return p


def drop_node(proof, row=0):
    p = _edit(proof)
    assert p.rows[row].nodes
    p.rows[row].nodes.pop()
    return p


def extra_node(proof, row=0):
    p = _edit(proof)
    p.rows[row].nodes.append(p.rows[row].row_root)
    return p


def drop_row(proof, j):
    """The proof without its j-th row (rows 3 and 5 without 4)."""
    p = _edit(proof)
    del p.rows[j]
    return p


def shift_start(proof, by=1):
    """The first row's range starts `by` later: no multiple of w."""
    p = _edit(proof)
    p.rows[0].start += by
    assert p.rows[0].start < p.rows[0].end
    return p


def change_total(proof, row=-1):
    p = _edit(proof)
    p.rows[row].total *= 2
    return p


# ------------------------------------------------------------------ flat arrays
def offsets(counts):
    return np.cumsum([0] + list(counts), dtype=np.int64).astype(np.uint32)


def _bytes(parts, width):
    a = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return a.reshape(-1, width).copy() if a.size else np.zeros((0, width), dtype=np.uint8)


def flat_arrays(proofs) -> dict:
    """The arrays of cda_commitment_proofs_out / cda_commitment_proof_batch for `proofs`, by field name."""
    rows = [r for p in proofs for r in p.rows]
    return {
        "seg_off": offsets(len(p.rows) for p in proofs),
        "nmt_start": np.array([r.start for r in rows], dtype=np.int32),
        "nmt_end": np.array([r.end for r in rows], dtype=np.int32),
        "node_off": offsets(len(r.nodes) for r in rows),
        "nodes": _bytes([x for r in rows for x in r.nodes], 90),
        "row_roots": _bytes([r.row_root for r in rows], 90),
        "rfc_total": np.array([r.total for r in rows], dtype=np.int64),
        "rfc_index": np.array([r.index for r in rows], dtype=np.int64),
        "rfc_leaf_hash": _bytes([r.leaf_hash for r in rows], 32),
        "aunt_off": offsets(len(r.aunts) for r in rows),
        "aunts": _bytes([a for r in rows for a in r.aunts], 32),
        "namespaces": _bytes([p.namespace for p in proofs], 29),
        "start_row": np.array([p.start_row for p in proofs], dtype=np.uint32),
        "end_row": np.array([p.end_row for p in proofs], dtype=np.uint32),
        "root_off": offsets(len(r.roots) for r in rows),
        "subtree_roots": _bytes([x for r in rows for x in r.roots], 90),
        "norm_start": np.array([p.norm_start for p in proofs], dtype=np.uint32),
        "commitments": _bytes([commitment(p) for p in proofs], 32),
    }


# ------------------------------------------------------------------ the fold kernel's tiling
FOLD_TILE, FOLD_TILE_LOG = 64, 6      # CDA_COMMITMENT_FOLD_TILE
FOLD_STAGE = {"nodes": 22, "low": 10, "tile": FOLD_TILE, "half": FOLD_TILE // 2 + 1, "next": 1025 // FOLD_TILE + 2}


def fold_model(roots, nodes, s0, e0, L, D, hash_node, trace=None):
    """vc_fold_kernel (csrc/verify.hip) step by step, on any node type: the chain below level L, the aligned
    tiles of FOLD_TILE nodes, the final fold.  Returns the root, or None where the kernel fails the segment.
    Asserts every staged count against the kernel's LDS arrays (FOLD_STAGE).  trace: a list that receives
    ("tile", first index, count) / ("final", first index, count)."""
    n_w, rem = (e0 - s0) >> L, (e0 - s0) & ((1 << L) - 1)
    n_low = bin(rem).count("1")
    popc = lambda x: bin(x).count("1")  # noqa: E731
    m = len(nodes)
    if len(roots) != n_w + n_low or m != popc(s0) + D - popc(e0 - 1):
        return None
    assert m <= FOLD_STAGE["nodes"] and n_low <= FOLD_STAGE["low"]
    low = roots[n_w:]
    state = {"li": popc(s0), "ri": popc(s0), "bad": False}
    carry, lx = None, n_low
    for lv in range(L):
        bit = (rem >> lv) & 1
        if not bit and carry is None:
            continue
        if bit:
            lx -= 1
            left = low[lx]
        else:
            left = carry
        if bit and carry is not None:
            right = carry
        else:
            if state["ri"] >= m:
                state["bad"] = True
            right = nodes[state["ri"] if state["ri"] < m else 0]
            state["ri"] += 1
        carry = hash_node(left, right)

    def fold_levels(src, a, b, levels):
        for _ in range(levels):
            need_l, need_r = a & 1, b & 1
            if (need_l and state["li"] == 0) or (need_r and state["ri"] >= m):
                state["bad"] = True
            lxx = state["li"] - 1 if state["li"] else 0
            rxx = state["ri"] if state["ri"] < m else 0
            na, nb = a >> 1, (b + 1) >> 1
            assert nb - na <= FOLD_STAGE["half"] and b - a <= FOLD_STAGE["tile"]
            dst = []
            for t in range(nb - na):
                p0 = 2 * (na + t)
                p1 = p0 + 1
                left = nodes[lxx] if p0 < a else src[p0 - a]
                right = nodes[rxx] if p1 >= b else src[p1 - a]
                dst.append(hash_node(left, right))
            if need_l and state["li"]:
                state["li"] -= 1
            if need_r:
                state["ri"] += 1
            a, b, src = na, nb, dst
        return src[0]

    run = roots[:n_w] + ([carry] if carry is not None else [])
    lo, level = s0 >> L, L
    hi = lo + len(run)
    if hi - lo > FOLD_TILE:
        t0, t1 = lo >> FOLD_TILE_LOG, (hi - 1) >> FOLD_TILE_LOG
        assert t1 - t0 < FOLD_STAGE["next"]
        nxt = []
        for t in range(t0, t1 + 1):
            a, e = max(lo, t << FOLD_TILE_LOG), min(hi, (t + 1) << FOLD_TILE_LOG)
            if trace is not None:
                trace.append(("tile", a, e - a))
            nxt.append(fold_levels(run[a - lo:e - lo], a, e, FOLD_TILE_LOG))
        run, lo, hi, level = nxt, t0, t1 + 1, level + FOLD_TILE_LOG
    assert hi - lo <= FOLD_TILE
    if trace is not None:
        trace.append(("final", lo, hi - lo))
    top = fold_levels(run, lo, hi, D - level)
    if state["bad"] or state["li"] != 0 or state["ri"] != m:
        return None
    return top
