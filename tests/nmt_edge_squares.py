"""Squares whose namespaces sit on the edges of the NMT rules -- TEST
INFRASTRUCTURE ONLY.

Every family is a deterministic function (k, seed) -> (k, k, 512) ODS with
random share bodies and namespaces from one ladder of ten 29-byte values
(ladder_values, ascending): the all-zero namespace and its byte-28 successor, a
random v0 namespace A and A with only byte 28 raised, a namespace that differs
from zero in byte 0 only, one with a first byte below 0xFF, one that differs
from the parity namespace in the middle (byte 14), FF*28 00, tail padding
(FF*28 FE) and the parity namespace FF*29 itself, which da.ExtendShares and
nmt Push accept on a Q0 share and which makes IgnoreMaxNamespace fire inside
the Q0 half of a tree.

Ordered families (non-decreasing along every row and column): ladder, uniform,
last_p, byte29_trap.  Unordered: p_left, byte28_descent.  ORDERED / UNORDERED
name the squares of each kind the tests run, batch_names the order a device
batch holds them in.

ns_tree_levels restates computeNsRange (test/util/malicious/hasher.go: min
from the left child, max from the right one unless the right min is the parity
namespace) on ladder ranks alone, so the preconditions of the GPU tests -- how
many left children a square has with min = FF*29 and max below it -- are cheap
at every k.
"""
import functools

import numpy as np

NS = 29
PARITY = b"\xff" * NS
TAIL_PADDING = b"\xff" * 28 + b"\xfe"
ZERO = b"\x00" * NS


def ns_a(seed: int) -> bytes:
    """A = 00*19 followed by 10 random bytes (first one non-zero, last one
    below 0xFF so that byte 28 can be raised)."""
    r = np.random.default_rng([0xA5, seed]).integers(0, 256, 10, dtype=np.uint8)
    r[0] |= 1
    r[9] &= 0x7F
    return b"\x00" * 19 + r.tobytes()


def ladder_values(seed: int) -> list:
    a = ns_a(seed)
    out = [ZERO,
           b"\x00" * 28 + b"\x01",
           a,
           a[:28] + bytes([a[28] + 1]),          # A with only byte 28 changed
           b"\x01" + b"\x00" * 28,                # differs from 00*29 in byte 0 only
           b"\xfe" + b"\xff" * 28,
           b"\xff" * 14 + b"\x00" + b"\xff" * 14,  # differs from parity at a word boundary
           b"\xff" * 28 + b"\x00",
           TAIL_PADDING,
           PARITY]
    assert out == sorted(out) and len(set(out)) == 10
    return out


def _bodies(k: int, seed: int, family: int) -> np.ndarray:
    return np.random.default_rng([family, k, seed]).integers(0, 256, (k, k, 512), dtype=np.uint8)


def _put(q0: np.ndarray, values: list, rank: np.ndarray) -> np.ndarray:
    """q0 with cell (r, c) given the namespace values[rank[r, c]]."""
    table = np.frombuffer(b"".join(values), dtype=np.uint8).reshape(len(values), NS)
    q0[:, :, :NS] = table[rank]
    return q0


def _antidiagonal_order(k: int) -> np.ndarray:
    """(k, k) position of every cell in the order by (r + c, r): a linear
    extension of the row / column order, so any non-decreasing assignment
    along it is non-decreasing along every row and every column."""
    r, c = np.divmod(np.arange(k * k), k)
    order = np.lexsort((r, r + c))
    pos = np.empty(k * k, dtype=np.int64)
    pos[order] = np.arange(k * k)
    return pos.reshape(k, k)


def ladder_ranks(k: int) -> np.ndarray:
    """Ladder rank of every cell of the ladder square: the last fifth of the
    antidiagonal order (the bottom-right corner) is FF*29, the cells before
    it take the other nine rungs in equal runs (all nine from k = 4 on)."""
    n = k * k
    n_par = max(1, n // 5)
    pos = _antidiagonal_order(k)
    return np.where(pos >= n - n_par, 9, pos * 9 // (n - n_par))


def ladder(k: int, seed: int = 0) -> np.ndarray:
    return _put(_bodies(k, seed, 1), ladder_values(seed), ladder_ranks(k))


def uniform(k: int, seed: int = 0, ns: bytes = ZERO) -> np.ndarray:
    return _put(_bodies(k, seed, 2), [ns], np.zeros((k, k), dtype=np.int64))


def last_p(k: int, seed: int = 0, what: str = "cell") -> np.ndarray:
    """A sorted square of random v0 namespaces whose last cell ("cell"), last
    row ("row") or last column ("col") carries FF*29."""
    q0 = _bodies(k, seed, 3)
    q0[:, :, :19] = 0
    q0[:, :, 19] |= 1
    flat = q0.reshape(k * k, 512)
    q0 = flat[np.lexsort(flat[:, NS - 1::-1].T)].reshape(k, k, 512).copy()
    if what == "cell":
        q0[k - 1, k - 1, :NS] = 0xFF
    elif what == "row":
        q0[k - 1, :, :NS] = 0xFF
    else:
        assert what == "col"
        q0[:, k - 1, :NS] = 0xFF
    return q0


def byte29_trap(k: int, seed: int = 0) -> np.ndarray:
    """Four runs of equal namespaces, neighbours differing only in byte 28
    (A with byte 28 + 0 .. 3), while share bytes 29..31 -- the rest of the
    32-bit word that holds byte 28 -- strictly decrease along every row and
    column: a namespace comparison that does not mask that word reports a
    violation inside every run."""
    a = ns_a(seed)
    a = a[:28] + bytes([a[28] & 0x7C])
    values = [a[:28] + bytes([a[28] + i]) for i in range(4)]
    q0 = _put(_bodies(k, seed, 4), values, _antidiagonal_order(k) * 4 // (k * k))
    r, c = np.indices((k, k))
    v = 0xFFFFFF - (r + c) * 0x4001          # < 2^24 up to k = 512; every step lowers byte 31, every 4th byte 29
    assert v.min() >= 0
    q0[:, :, 29] = v >> 16
    q0[:, :, 30] = (v >> 8) & 0xFF
    q0[:, :, 31] = v & 0xFF
    return q0


def p_left(k: int, seed: int = 0) -> np.ndarray:
    """A seeded shuffle of a ladder multiset, half of it FF*29 and the rest
    the other nine rungs in turn: pairs [FF*29, X] whose parent has min =
    FF*29 and max = X, at every level of the blind trees."""
    n = k * k
    rank = np.where(np.arange(n) % 2 == 0, 9, (np.arange(n) // 2) % 9)
    rng = np.random.default_rng([0x9E, k, seed])
    q0 = _bodies(k, seed, 5)
    while True:   # (a shuffle of four cells can come out ordered)
        rng.shuffle(rank)
        _put(q0, ladder_values(seed), rank.reshape(k, k))
        if first_violation(q0) is not None:
            return q0


def _ns(q0, r, c) -> bytes:
    return q0[r, c, :NS].tobytes()


def byte28_descent(k: int, seed: int = 0, axis: int = 0, last: bool = False) -> np.ndarray:
    """The ladder square with exactly one adjacent pair out of order, and that
    only in byte 28: the first cell (row-major; of the last Q0 column if
    `last`) that can take its left neighbour's namespace with byte 28 lowered
    by one without falling below the cell above it.  axis = 1: the transpose,
    so the pair descends along a column (and, with `last`, ends on the last Q0
    row)."""
    q0 = ladder(k, seed)
    for r in range(k):
        for c in ([k - 1] if last else range(1, k)):
            left = _ns(q0, r, c - 1)
            if left[28] == 0:
                continue
            new = left[:28] + bytes([left[28] - 1])
            if r > 0 and _ns(q0, r - 1, c) > new:
                continue
            q0[r, c, :NS] = np.frombuffer(new, dtype=np.uint8)
            return np.ascontiguousarray(q0.transpose(1, 0, 2)) if axis else q0
    raise AssertionError(f"no byte-28 descent fits the ladder square of width {k}")


def descents(q0: np.ndarray) -> list:
    """Every adjacent pair of one Q0 that descends: (axis, index, position,
    first differing byte)."""
    k = q0.shape[0]
    out = []
    for axis in (0, 1):
        g = q0 if axis == 0 else q0.transpose(1, 0, 2)
        for i in range(k):
            for p in range(1, k):
                a, b = g[i, p - 1, :NS].tobytes(), g[i, p, :NS].tobytes()
                if b < a:
                    out.append((axis, i, p, next(j for j in range(NS) if a[j] != b[j])))
    return out


def first_violation(q0: np.ndarray):
    """Brute-force nmt push-order check of one Q0: the smallest (axis, index,
    position) whose namespace is below its predecessor's, rows before
    columns, as cda_push_order_detail_at reports it; None if ordered."""
    k = q0.shape[0]
    for axis in (0, 1):
        ns = np.ascontiguousarray((q0 if axis == 0 else q0.transpose(1, 0, 2))[:, :, :NS])
        for i in range(k):
            row = [x.tobytes() for x in ns[i]]
            for p in range(1, k):
                if row[p] < row[p - 1]:
                    return (axis, i, p)
    return None


# name -> (builder, ordered)
SQUARES = {
    "p_left": (p_left, False),
    "ladder": (ladder, True),
    "descent_row": (functools.partial(byte28_descent, axis=0), False),
    "byte29_trap": (byte29_trap, True),
    "descent_col": (functools.partial(byte28_descent, axis=1), False),
    "last_p_cell": (functools.partial(last_p, what="cell"), True),
    "descent_row_last": (functools.partial(byte28_descent, axis=0, last=True), False),
    "last_p_row": (functools.partial(last_p, what="row"), True),
    "descent_col_last": (functools.partial(byte28_descent, axis=1, last=True), False),
    "last_p_col": (functools.partial(last_p, what="col"), True),
    "uniform_zero": (functools.partial(uniform, ns=ZERO), True),
    "uniform_a": (lambda k, seed=0: uniform(k, seed, ns_a(seed)), True),
    "uniform_tail_padding": (functools.partial(uniform, ns=TAIL_PADDING), True),
    "uniform_parity": (functools.partial(uniform, ns=PARITY), True),
}
ORDERED = [name for name, (_, ordered) in SQUARES.items() if ordered]
UNORDERED = [name for name, (_, ordered) in SQUARES.items() if not ordered]

# The seed every test uses: chosen so that the P-left square of every width
# the GPU tests run has, among its row trees and among its column trees, at
# least k left children with min = FF*29 > max, some at every level from 1 to
# log2(k) - 1 (test_namespace_edges.py::test_p_left_reaches_the_parity_min_left_children).
SEED = 3


def square(name: str, k: int, seed: int = SEED) -> np.ndarray:
    return SQUARES[name][0](k, seed)


def batch_names(k: int) -> list:
    """The distinct squares of a device batch of width k, in order: edge
    squares with the oracle's random squares ("random:<index>") in between,
    an odd number of them, the two that matter most first.  From k = 256 on
    only P-left and the ladder."""
    if k >= 256:
        return ["p_left", "ladder", "random:0"]
    out = []
    for i, name in enumerate(SQUARES):
        out.append(name)
        if i % 2 == 1:
            out.append(f"random:{i // 2}")
    assert len(out) % 2 == 1
    return out


def ladder_rank_of(q0: np.ndarray, seed: int = SEED) -> np.ndarray:
    """(k, k) ladder rank of every cell of a square built from the ladder."""
    values = ladder_values(seed)
    k = q0.shape[0]
    flat = q0[:, :, :NS].reshape(k * k, NS)
    rank = np.full(k * k, -1, dtype=np.int64)
    for i, v in enumerate(values):
        rank[(flat == np.frombuffer(v, dtype=np.uint8)).all(axis=1)] = i
    assert (rank >= 0).all()
    return rank.reshape(k, k)


def ns_tree_levels(rank: np.ndarray, parity_rank: int = 9):
    """Namespace ranges of the Q0-half subtrees of k blind trees at once.
    rank: (trees, k) ladder ranks of the Q0 leaves (row trees: the ODS rows,
    column trees: its transpose).  Yields (level, mins, maxs) for level = 1 ..
    log2(k), each (trees, k >> level): min from the left child, max from the
    right one unless the right min is the parity namespace (computeNsRange
    with IgnoreMaxNamespace, no order check)."""
    mins = maxs = np.asarray(rank)
    level = 0
    while mins.shape[1] > 1:
        lmin, rmin = mins[:, 0::2], mins[:, 1::2]
        lmax, rmax = maxs[:, 0::2], maxs[:, 1::2]
        mins, maxs = lmin, np.where(rmin == parity_rank, lmax, rmax)
        level += 1
        yield level, mins, maxs


def parity_min_left_children(rank: np.ndarray, parity_rank: int = 9) -> dict:
    """{level: count} of the inner nodes of the trees over `rank` that are
    left children, lie at level >= 1 and have min = FF*29 and max != FF*29:
    the nodes whose 55-byte head is not the constant one although their min
    namespace is the parity namespace.  (The root of a Q0 half is the left
    child of its tree's root: level log2(k).)"""
    out = {}
    for level, mins, maxs in ns_tree_levels(rank, parity_rank):
        hit = (mins == parity_rank) & (maxs != parity_rank)
        out[level] = int(hit[:, 0::2].sum())   # a lone node is node 0: a left child
    return out
