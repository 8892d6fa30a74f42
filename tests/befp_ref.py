"""CPU yardstick for bad-encoding fraud proofs -- TEST INFRASTRUCTURE ONLY.

A restatement of the builder and of the four validation steps (include/cda.h,
"Bad-encoding fraud proofs") composed from the oracle: leopard_reconstruct
(oracle/repair.py), leopard_encode, erasured_leaves and axis_root
(oracle/pyref.py), nmt_range_proof and nmt_verify_inclusion (oracle/proofs.py).
The reference holds the protocol text only (specs/src/specs/fraud_proofs.md,
networking.md "BadEncodingFraudProof", proto/types.proto:247-259), no vector, so
this file is what the GPU answers are compared with.

Also the test squares and the proof cases that tests/test_befp_ref.py pins on
the CPU and tests/test_befp.py replays on the GPU.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import proofs as oproofs
import pyref
import repair as orepair

ROW, COL = 0, 1
VALID, TOO_FEW, NOT_INCLUDED, ROOT_MATCHES = 0, 1, 2, 3
NODE = pyref.NMT_NODE_SIZE


def log2(x: int) -> int:
    return x.bit_length() - 1


@dataclass
class RefProof:
    """Field for field celestia_da.byzantine.BadEncodingProof (numpy arrays)."""
    k: int
    axis: int
    index: int
    positions: np.ndarray    # (m,) uint32
    proof_axes: np.ndarray   # (m,) uint8
    shares: np.ndarray       # (m, 512)
    nmt_nodes: np.ndarray    # (m, D, 90)

    def __len__(self):
        return int(self.positions.shape[0])

    def copy(self):
        return RefProof(self.k, self.axis, self.index, self.positions.copy(), self.proof_axes.copy(),
                        self.shares.copy(), self.nmt_nodes.copy())

    def take(self, sel):
        """The proof with only the entries `sel` (indexes into the arrays)."""
        sel = np.asarray(sel, dtype=np.int64)
        return RefProof(self.k, self.axis, self.index, self.positions[sel].copy(), self.proof_axes[sel].copy(),
                        self.shares[sel].copy(), self.nmt_nodes[sel].copy())

    def at(self, positions):
        """The proof with only the given positions of the vector."""
        want = set(int(p) for p in positions)
        return self.take([i for i, p in enumerate(self.positions.tolist()) if p in want])


@dataclass
class Square:
    """An EDS with the roots committed for it (the DAH a verifier holds)."""
    eds: np.ndarray   # (W, W, 512)
    rows: list        # W x 90 bytes
    cols: list
    _leaves: dict = field(default_factory=dict)

    @property
    def k(self) -> int:
        return self.eds.shape[0] // 2

    def vector(self, axis: int, i: int) -> np.ndarray:
        return self.eds[i] if axis == ROW else self.eds[:, i]

    def leaves(self, axis: int, i: int):
        """Blind erasured leaves of row / column i (no push-order check, as the builder hashes)."""
        if (axis, i) not in self._leaves:
            self._leaves[(axis, i)] = pyref.erasured_leaves(self.vector(axis, i), self.k, i, blind=True)
        return self._leaves[(axis, i)]

    def dah(self):
        return self.rows, self.cols

    def rows_array(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.rows), dtype=np.uint8).reshape(-1, NODE).copy()

    def cols_array(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.cols), dtype=np.uint8).reshape(-1, NODE).copy()


def committed(eds: np.ndarray, blind: bool = False) -> Square:
    rows, cols, _ = pyref.dah_from_eds(eds, blind)
    return Square(eds, rows, cols)


@functools.lru_cache(maxsize=None)
def honest_square(k: int) -> Square:
    ods = pyref.ods_from_shares(pyref.random_namespaced_square(k))
    return committed(pyref.extend_square(ods))


def flipped_cell(k: int):
    """The Q1 cell (r, c), r < k <= c, that the malicious square corrupts."""
    return (k - 1, k) if k > 1 else (0, 1)


def flipped_cells(k: int):
    """Two cells per quadrant, Q0..Q3: the corners of the square and the cells about its centre."""
    W = 2 * k
    return [(0, 0), (k - 1, k - 1), (0, W - 1), (k - 1, k), (W - 1, 0), (k, k - 1), (k, k), (W - 1, W - 1)]


@functools.lru_cache(maxsize=None)
def malicious_square(k: int, cell=None) -> Square:
    """The honest EDS with a few payload bytes of one cell flipped (`cell`, default the Q1 cell flipped_cell(k))
    and all 4k roots recomputed from the corrupted cells: row r and column c are committed non-codewords."""
    r, c = flipped_cell(k) if cell is None else cell
    eds = honest_square(k).eds.copy()
    eds[r, c, 100:104] ^= 0x5A
    return committed(eds)


@functools.lru_cache(maxsize=None)
def unordered_square(k: int):
    """(square, row): an ODS with two cells of one row swapped so that its namespaces descend, extended properly
    and committed over blind trees (test/util/malicious): every vector is a codeword, row `row` breaks push order."""
    ods = pyref.ods_from_shares(pyref.random_namespaced_square(k)).copy()
    row = 0
    assert bytes(ods[row, 0, :29]) < bytes(ods[row, k - 1, :29])
    ods[row, [0, k - 1]] = ods[row, [k - 1, 0]]
    return committed(pyref.extend_square(ods), blind=True), row


# ------------------------------------------------------------------ the builder
def cell_of(axis: int, index: int, pos: int):
    return (index, pos) if axis == ROW else (pos, index)


def prove(sq: Square, axis: int, index: int, positions, proof_axes=None) -> RefProof:
    """Shares `positions` of vector (axis, index), each proven against the orthogonal root (or the axis that
    proof_axes names), whatever the square commits to."""
    k, W = sq.k, 2 * sq.k
    D = log2(W)
    positions = [int(p) for p in positions]
    pax = [1 - axis] * len(positions) if proof_axes is None else [int(a) for a in proof_axes]
    shares = np.zeros((len(positions), 512), dtype=np.uint8)
    nodes = np.zeros((len(positions), D, NODE), dtype=np.uint8)
    for j, (p, a) in enumerate(zip(positions, pax)):
        r, c = cell_of(axis, index, p)
        shares[j] = sq.eds[r, c]
        tree, leaf = (index, p) if a == axis else (p, index)
        got = oproofs.nmt_range_proof(sq.leaves(a, tree), leaf, leaf + 1)
        assert len(got) == D
        nodes[j] = np.frombuffer(b"".join(got), dtype=np.uint8).reshape(D, NODE)
    return RefProof(k, axis, index, np.array(positions, dtype=np.uint32), np.array(pax, dtype=np.uint8), shares, nodes)


def build(eds: np.ndarray, rows, cols, axis: int, index: int) -> RefProof:
    """cda_befp_build: cell p of the vector is emitted iff the orthogonal vector through it hashes (blind) to its
    DAH root; positions ascend."""
    sq = Square(np.asarray(eds), [bytes(r) for r in rows], [bytes(c) for c in cols])
    W = 2 * sq.k
    orth = sq.cols if axis == ROW else sq.rows
    ok = [p for p in range(W) if pyref.nmt_root_from_nodes(sq.leaves(1 - axis, p)) == orth[p]]
    return prove(sq, axis, index, ok)


# ---------------------------------------------------------------- the verifier
def validate(proof, rows, cols):
    """(verdict, rebuilt root): steps 1-4.  The rebuilt root is the blind one; 90 zero bytes when step 3 is
    never reached."""
    k = int(proof.k)
    W = 2 * k
    axis, index = int(proof.axis), int(proof.index)
    zero = bytes(NODE)
    m = len(proof)
    if m < k:                                                        # step 1
        return TOO_FEW, zero
    for j in range(m):                                               # step 2
        p, a = int(proof.positions[j]), int(proof.proof_axes[j])
        r, c = cell_of(axis, index, p)
        share = bytes(proof.shares[j])
        ns = share[:29] if (r < k and c < k) else pyref.PARITY_NS
        tree, leaf = (index, p) if a == axis else (p, index)
        root = bytes((rows if a == ROW else cols)[tree])
        nodes = [bytes(proof.nmt_nodes[j, q]) for q in range(proof.nmt_nodes.shape[1])]
        if not oproofs.nmt_verify_inclusion(root, nodes, leaf, leaf + 1, ns, [share]):
            return NOT_INCLUDED, zero
    vec = np.zeros((W, 512), dtype=np.uint8)                         # step 3
    present = np.zeros(W, dtype=bool)
    for j in range(m):
        vec[int(proof.positions[j])] = proof.shares[j]
        present[int(proof.positions[j])] = True
    data = orepair.leopard_reconstruct(vec, present)[:k]
    full = np.concatenate([data, pyref.leopard_encode(data)])
    rebuilt = pyref.axis_root(full, k, index, blind=True)
    try:
        pyref.erasured_leaves(full, k, index)
        ordered = True
    except pyref.PushOrderError:
        ordered = False
    want = bytes((rows if axis == ROW else cols)[index])            # step 4
    return (ROOT_MATCHES if ordered and rebuilt == want else VALID), rebuilt


# -------------------------------------------------------------------- the cases
def parity_namespace_case(k: int):
    """A parity cell sent with its own first 29 bytes as namespace: the DAH's root of the orthogonal tree was
    computed with that leaf hashed under the cell's prefix, so a verifier that took the namespace from the share
    would accept; the derived namespace (ParitySharesNamespace) does not fold to that root."""
    sq = honest_square(k)
    axis, index, p = ROW, 0, 2 * k - 1          # cell (0, W - 1) is in Q1
    proof = prove(sq, axis, index, range(2 * k))
    share = bytes(sq.eds[0, p])
    leaves = list(sq.leaves(COL, p))
    leaves[index] = pyref.nmt_hash_leaf(share[:29] + share)
    cols = list(sq.cols)
    cols[p] = pyref.nmt_root_from_nodes(leaves)
    nodes = [bytes(proof.nmt_nodes[p, q]) for q in range(proof.nmt_nodes.shape[1])]
    assert oproofs.nmt_verify_inclusion(cols[p], nodes, index, index + 1, share[:29], [share])
    return proof, sq.rows, cols


@functools.lru_cache(maxsize=None)
def cases(k: int):
    """[(name, proof, rows, cols, verdict the issue states)]: every verifier case, at one ODS width."""
    W = 2 * k
    H, M = honest_square(k), malicious_square(k)
    r, c = flipped_cell(k)
    out = []

    def add(name, proof, sq_or_roots, want):
        rows, cols = sq_or_roots.dah() if isinstance(sq_or_roots, Square) else sq_or_roots
        out.append((name, proof, rows, cols, want))

    add("honest row 0, all shares", prove(H, ROW, 0, range(W)), H, ROOT_MATCHES)
    add("honest col k, exactly k shares", prove(H, COL, k, range(k, W)), H, ROOT_MATCHES)
    row_all = prove(M, ROW, r, range(W))
    add("bad row, all shares", row_all, M, VALID)
    add("bad row, k shares without the flipped cell", row_all.at(range(k)), M, VALID)
    add("bad row, k shares with the flipped cell", row_all.at(list(range(1, k)) + [c]), M, VALID)
    col_all = prove(M, COL, c, range(W))
    add("bad col, all shares", col_all, M, VALID)
    add("bad col, k shares without the flipped cell", col_all.at(range(k, W)), M, VALID)
    add("bad col, k shares with the flipped cell", col_all.at(range(k)), M, VALID)
    add("k - 1 shares", row_all.at(range(k - 1)), M, TOO_FEW)
    bad = row_all.copy()
    bad.shares[1, 300] ^= 1
    add("flipped share byte", bad, M, NOT_INCLUDED)
    bad = row_all.copy()
    bad.nmt_nodes[W - 1, 0, 70] ^= 1
    add("flipped node byte", bad, M, NOT_INCLUDED)
    bad = row_all.copy()   # the content of two positions swapped (the positions themselves must ascend)
    bad.shares[[0, 1]] = bad.shares[[1, 0]]
    bad.nmt_nodes[[0, 1]] = bad.nmt_nodes[[1, 0]]
    add("two positions swapped", bad, M, NOT_INCLUDED)
    proof, rows, cols = parity_namespace_case(k)
    add("parity cell under its own namespace", proof, (rows, cols), NOT_INCLUDED)
    sound = 0 if r != 0 else 1
    add("sound row of the malicious square", prove(M, ROW, sound, row_all.positions), M, ROOT_MATCHES)
    add("own-axis proofs", prove(M, ROW, r, range(W), [ROW] * W), M, VALID)
    add("mixed proof axes", prove(M, COL, c, range(W), [q % 2 for q in range(W)]), M, VALID)
    U, urow = unordered_square(k)
    add("descending namespaces in the rebuilt data half", prove(U, ROW, urow, range(W)), U, VALID)
    return out
