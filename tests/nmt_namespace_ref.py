"""CPU restatement of the namespace query -- TEST INFRASTRUCTURE ONLY.

Restates, from the published algorithms of nmt v0.22.0 and on top of the
oracle's own pieces only (pyref.erasured_leaves / nmt_hash_node /
nmt_root_from_nodes, proofs.nmt_range_proof / nmt_verify_inclusion):
  * NamespacedMerkleTree.ProveNamespace: the inclusion proof of the whole run
    of the namespace (foundInRange -> ProveRange), or the absence proof, the
    ProveRange of the first leaf above it (calculateAbsentIndex) with that
    leaf's node as Proof.leafHash            -> prove_namespace
  * Proof.VerifyNamespace = VerifyLeafHashes(verifyCompleteness = true): the
    root from the leaves (or the absence leaf, whose min namespace must be above
    the queried one) and the nodes, then no node left of the range may reach the
    namespace (max >= ns) and none right of it either (min <= ns)
                                             -> segment_verdict
  * the row selection GetSharesByNamespace makes on the DAH: the rows with
    min(rowRoot) <= ns <= max(rowRoot)       -> selected_rows
and, on top of them, the answer and the verdict of the library's batch calls
(get_shares_by_namespace, answer_verdict) and the squares, queries, inventory
and tampered answers the namespace tests share.
"""
from dataclasses import dataclass, replace

import numpy as np

import coracle
import proofs as opr
import pyref

NS = 29
PARITY = b"\xff" * NS


@dataclass
class NsProof:          # celestia_da.proof.NMTProof's fields
    start: int
    end: int
    nodes: list
    leaf_hash: bytes = b""


class RefSquare:
    """One square as the restatement sees it: the oracle's EDS, the leaf nodes of its row trees and their roots."""

    def __init__(self, ods):
        ods = np.ascontiguousarray(ods, dtype=np.uint8).reshape(-1, 512)
        self.k = int(round(len(ods) ** 0.5))
        assert self.k * self.k == len(ods)
        self.ods = ods
        W = 2 * self.k
        self.eds = np.asarray(coracle.extend(ods)).reshape(W, W, 512)
        self.leaves = [pyref.erasured_leaves([x.tobytes() for x in self.eds[r]], self.k, r) for r in range(W)]
        self.row_roots = [pyref.nmt_root_from_nodes(lv) for lv in self.leaves]

    def namespaces(self):
        return sorted({x[:NS].tobytes() for x in self.ods})


def selected_rows(row_roots, ns):
    return [r for r, root in enumerate(row_roots) if root[:NS] <= ns <= root[NS:2 * NS]]


def prove_namespace(leaves, ns):
    """ProveNamespace of a tree that holds a leaf >= ns (the caller selected the row): an NsProof."""
    less = sum(1 for x in leaves if x[:NS] < ns)
    equal = sum(1 for x in leaves if x[:NS] == ns)
    if equal:
        return NsProof(less, less + equal, opr.nmt_range_proof(leaves, less, less + equal))
    return NsProof(less, less + 1, opr.nmt_range_proof(leaves, less, less + 1), leaves[less])


def get_shares_by_namespace(sq, ns):
    """[(row, NsProof, shares)] in row order: what cda_square_namespace_proofs answers to one query."""
    out = []
    for r in selected_rows(sq.row_roots, ns):
        p = prove_namespace(sq.leaves[r], ns)
        shares = [] if p.leaf_hash else [sq.eds[r, c].tobytes() for c in range(p.start, p.end)]
        out.append((r, p, shares))
    return out


def _root_from_leaf_nodes(nodes, start, end, leaf_nodes):
    """VerifyLeafHashes' computeRoot over leaf nodes (None if the nodes run out): the subtree of pow2ceil(end)
    leaves, then the nodes that remain folded in on the right."""
    rest, hs = list(nodes), list(leaf_nodes)
    pop = lambda a: a.pop(0) if a else None   # noqa: E731

    def compute(lo, hi):
        if hi - lo == 1:
            return pop(hs) if start <= lo < end else pop(rest)
        if hi <= start or lo >= end:
            return pop(rest)
        half = (hi - lo) // 2
        left, right = compute(lo, lo + half), compute(lo + half, hi)
        if left is None:
            return None
        return left if right is None else pyref.nmt_hash_node(left, right)

    size = 1
    while size < end:
        size *= 2
    h = compute(0, size)
    while rest and h is not None:
        h = pyref.nmt_hash_node(h, rest.pop(0))
    return h


def segment_verdict(root, ns, p, shares):
    """VerifyNamespace of one row's proof: 0, 2 (the root, or the absence leaf) or 3 (completeness)."""
    if p.leaf_hash:
        ok = not shares and p.end == p.start + 1 and p.leaf_hash[:NS] > ns \
            and _root_from_leaf_nodes(p.nodes, p.start, p.end, [p.leaf_hash]) == root
    else:
        ok = len(shares) == p.end - p.start and opr.nmt_verify_inclusion(root, p.nodes, p.start, p.end, ns, shares)
    if not ok:
        return 2
    n_left = bin(p.start).count("1")
    if any(x[NS:2 * NS] >= ns for x in p.nodes[:n_left]) or any(x[:NS] <= ns for x in p.nodes[n_left:]):
        return 3
    return 0


def answer_verdict(row_roots, ns, answer):
    """The verdict of cda_namespace_proofs_verify for one query; the lower number wins."""
    if [r for r, _, _ in answer] != selected_rows(row_roots, ns):
        return 1
    v = [segment_verdict(row_roots[r], ns, p, shares) for r, p, shares in answer]
    return 2 if 2 in v else 3 if 3 in v else 0


# ------------------------------------------------------------------ squares and queries
def hand_made_square():
    """[[A, C], [B, D]] with A < B < C < D: rows and columns ordered, the square not row-major."""
    a, b, c, d = (bytes(NS - 1) + bytes([v]) + bytes([v + 1]) * (512 - NS) for v in (0x10, 0x20, 0x30, 0x40))
    return np.frombuffer(a + c + b + d, dtype=np.uint8).reshape(4, 512).copy()


_squares = {}


def squares():
    """name -> RefSquare: SMALL k = 1, 2, 4, 8 of test_share_proofs_batch and the hand-made 2 x 2; made once."""
    if not _squares:
        from test_share_proofs_batch import SMALL, square_of
        for k in SMALL:
            _squares[f"small{k}"] = RefSquare(square_of(k))
        _squares["hand"] = RefSquare(hand_made_square())
    return _squares


def queries(sq):
    """Every present namespace, its neighbours as 232-bit integers where those are not present themselves (and
    are namespaces one can ask for: not below zero, not the parity namespace or beyond), and the all-zero one."""
    present = sq.namespaces()
    out = set(present) | {bytes(NS)}
    for ns in present:
        v = int.from_bytes(ns, "big")
        for w in (v - 1, v + 1):
            if 0 <= w < (1 << (8 * NS)) - 1:
                out.add(w.to_bytes(NS, "big"))
    assert PARITY not in out
    return sorted(out)


KINDS = ("single_row_inclusion", "multi_row_whole_row", "run_from_leaf_0", "run_to_last_leaf", "absence", "mixed",
         "empty_below", "empty_between", "empty_above")


def kinds_of(sq, ns, answer):
    k = sq.k
    inc = [(r, p) for r, p, _ in answer if not p.leaf_hash]
    out = set()
    if not answer:
        lo, hi = min(x[:NS] for x in sq.row_roots[:k]), max(x[NS:2 * NS] for x in sq.row_roots[:k])
        out.add("empty_below" if ns < lo else "empty_above" if ns > hi else "empty_between")
    if len(answer) == 1 and len(inc) == 1:
        out.add("single_row_inclusion")
    if len(inc) >= 2 and any((p.start, p.end, len(p.nodes)) == (0, k, 1) for _, p in inc):
        out.add("multi_row_whole_row")
    if any(p.start == 0 for _, p in inc):
        out.add("run_from_leaf_0")
    if any(p.end == k for _, p in inc):
        out.add("run_to_last_leaf")
    if len(inc) < len(answer):
        out.add("absence")
        if inc:
            out.add("mixed")
    return out


_honest = {}


def honest(name):
    """[(ns, answer)] for every query of the named square; computed once, never changed."""
    if name not in _honest:
        sq = squares()[name]
        _honest[name] = [(ns, get_shares_by_namespace(sq, ns)) for ns in queries(sq)]
    return _honest[name]


# ------------------------------------------------------------------ tampered answers
def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def flip_share(answer, g=None):
    g = next(i for i, (_, _, sh) in enumerate(answer) if sh) if g is None else g
    r, p, sh = answer[g]
    return answer[:g] + [(r, p, [_flip(sh[0], 100)] + sh[1:])] + answer[g + 1:]


def shorten(sq, answer, g, first):
    """Segment g as the honest ProveRange of its run without the first or the last share."""
    r, p, sh = answer[g]
    s, e = (p.start + 1, p.end) if first else (p.start, p.end - 1)
    q = NsProof(s, e, opr.nmt_range_proof(sq.leaves[r], s, e))
    return answer[:g] + [(r, q, sh[1:] if first else sh[:-1])] + answer[g + 1:]


def tampers(name):
    """[(label, ns, answer, verdict)]: every tamper of the issue's table, each made of the first honest answer
    of the named square it applies to; the labels present depend on the square."""
    sq = squares()[name]
    k, out, seen = sq.k, [], set()

    def add(label, ns, answer, verdict):
        if label not in seen:
            seen.add(label)
            out.append((label, ns, answer, verdict))

    for ns, ans in honest(name):
        inc = [g for g, (_, p, _) in enumerate(ans) if not p.leaf_hash]
        absent = [g for g, (_, p, _) in enumerate(ans) if p.leaf_hash]
        long_runs = [g for g in inc if ans[g][1].end - ans[g][1].start >= 2]
        if ans:
            add("row_dropped", ns, ans[1:], 1)
            extra = ans[-1][0] + 1
            add("row_appended", ns, ans + [(extra, ans[-1][1], ans[-1][2])], 1)
        if len(ans) >= 2:
            add("rows_swapped", ns, [ans[1], ans[0]] + ans[2:], 1)
        if inc:
            add("share_flipped", ns, flip_share(ans), 2)
        if len(ans) >= 2 and inc:   # two faults: a flipped share in one row, another row dropped
            drop = 1 if inc[0] == 0 else 0
            flipped = flip_share(ans, inc[0])
            add("drop_and_flip", ns, flipped[:drop] + flipped[drop + 1:], 1)
        if ans:
            r, p, sh = ans[0]
            add("node_flipped", ns, [(r, replace(p, nodes=[_flip(p.nodes[0], 70)] + p.nodes[1:]), sh)] + ans[1:], 2)
        if absent:
            g = absent[0]
            r, p, sh = ans[g]
            add("absence_leaf_not_above", ns, ans[:g] + [(r, replace(p, leaf_hash=ns + ns + p.leaf_hash[2 * NS:]), sh)]
                + ans[g + 1:], 2)
        if long_runs:
            add("without_last", ns, shorten(sq, ans, long_runs[0], False), 3)
            add("without_first", ns, shorten(sq, ans, long_runs[0], True), 3)
        if len(inc) >= 2 and long_runs:
            other = next(g for g in inc if g != long_runs[0])
            add("flip_and_incomplete", ns, flip_share(shorten(sq, ans, long_runs[0], False), other), 2)
        if len(ans) == 1 and inc:
            r, p, _ = ans[0]
            q = NsProof(p.end, p.end + 1, opr.nmt_range_proof(sq.leaves[r], p.end, p.end + 1), sq.leaves[r][p.end])
            add("absence_after_run", ns, [(r, q, [])], 3)
    return out


TAMPER_LABELS = ("row_dropped", "row_appended", "rows_swapped", "share_flipped", "node_flipped",
                 "absence_leaf_not_above", "without_last", "without_first", "absence_after_run",
                 "drop_and_flip", "flip_and_incomplete")
