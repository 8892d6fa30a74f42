"""Repair against maliciously committed and unordered squares (cda_repair, cda_repair_device).

A byzantine producer commits roots computed over the badly encoded square: every root matches and only the
parity check, or a rebuild, can expose the row or column.  The squares are tests/befp_ref.py's: the honest EDS with
one cell flipped and all 4k roots recomputed (two cells per quadrant), and the properly encoded square with one
descending row committed over blind trees.  Every outcome, axis and index included, is compared with
oracle/repair.py, and every byzantine outcome that leaves enough provable shares is carried on to a fraud proof
that must validate against the committed DAH.

Masks per (k, flipped cell), seeds SEED + 100 k + cell number:
  * random at densities DENSITIES;
  * each quadrant withheld;
  * the flipped cell held, and withheld, with its row and column both incomplete;
  * the two holes (k - 1, 0) and (k, k) alone: with the default cell (k - 1, k) column 0 is rebuilt first and
    completes row k - 1, whose root matches while its parity does not.
Honest squares run under the same masks (each distinct mask once per k).

One outcome is the project's choice, not rsmt2d's pinned one: a vector complete in the input
whose namespaces descend is ErrByzantineData from the pre-repair check.
"""
import functools

import numpy as np
import pytest

import befp_ref as ref
import repair as orp
from test_repair import device_repair, gpu_repair, run_oracle

SEED = 7000
DENSITIES = (0.3, 0.45, 0.6, 0.75, 0.9)
# k = 16, reduced: one cell per quadrant, one random mask, the opposite quadrant withheld, the two holes
REDUCED_CELLS = (0, 3, 5, 7)


def quadrant_withheld(k, q):
    p = np.ones((2 * k, 2 * k), dtype=bool)
    r0, c0 = (q // 2) * k, (q % 2) * k
    p[r0:r0 + k, c0:c0 + k] = False
    return p


def two_holes(k):
    p = np.ones((2 * k, 2 * k), dtype=bool)
    p[k - 1, 0] = False
    p[k, k] = False
    return p


def masks_for(k, n, cell):
    """[(name, present)] for flipped cell number n = `cell` of an ODS width k."""
    W = 2 * k
    r, c = cell
    rng = np.random.default_rng(SEED + 100 * k + n)
    reduced = k >= 16
    out = []
    for d in (DENSITIES[2:3] if reduced else DENSITIES):
        out.append((f"random {d}", rng.random((W, W)) < d))
    for q in ((3 - n // 2,) if reduced else range(4)):
        out.append((f"Q{q} withheld", quadrant_withheld(k, q)))
    if not reduced:
        for held in (True, False):
            p = rng.random((W, W)) < 0.75
            p[r, (c + 1 + rng.integers(0, W - 1)) % W] = False
            p[(r + 1 + rng.integers(0, W - 1)) % W, c] = False
            p[r, c] = held
            out.append((f"cell {'held' if held else 'withheld'}, row and column incomplete", p))
    out.append(("two holes", two_holes(k)))
    return out


@functools.lru_cache(maxsize=None)
def matrix(k):
    """The cases of one ODS width with the oracle's outcome of each, computed once:
    [(label, square, present, outcome, how, named vector complete in the input)], malicious and honest interleaved."""
    H = ref.honest_square(k)
    cells = ref.flipped_cells(k)
    out, seen = [], set()
    for n, cell in enumerate(cells):
        if k >= 16 and n not in REDUCED_CELLS:
            continue
        M = ref.malicious_square(k, cell)
        for name, p in masks_for(k, n, cell):
            todo = [(f"malicious {cell}, {name}", M)]
            if p.tobytes() not in seen:
                seen.add(p.tobytes())
                todo.append((f"honest, {name} (as for {cell})", H))
            for label, sq in todo:
                info = {}
                want, rep = run_oracle(sq.eds, p, sq.rows, sq.cols, info)
                if want == "ok":
                    assert np.array_equal(rep, sq.eds), label
                complete = None
                if isinstance(want, tuple):
                    complete = bool((p[want[2]] if want[1] == orp.ROW else p[:, want[2]]).all())
                out.append((label, sq, p, want, info.get("how"), complete))
    return out


def histogram(k):
    h = {}
    for label, _sq, _p, want, _how, _c in matrix(k):
        key = (label.split(",")[0].split(" ")[0], want if isinstance(want, str) else "byz")
        h[key] = h.get(key, 0) + 1
    return h


def check_coverage(k, outcomes):
    """The conditions the matrix is chosen to meet, on `outcomes` (one per case of matrix(k), the oracle's or a
    GPU entry point's)."""
    cases = matrix(k)
    assert len(outcomes) == len(cases)
    named = [(o, c) for o, c in zip(outcomes, cases) if isinstance(o, tuple)]
    assert {o[1] for o, _ in named} == {orp.ROW, orp.COL}, "named vectors on one axis only"
    assert any(c[5] and c[4] == "check-parity" for _, c in named), "no parity-only pre-check case"
    assert any(c[5] is False for _, c in named), "no named vector that was incomplete in the input"
    assert any(c[4] == "orth-parity" for _, c in named), "no orthogonal parity-only case"
    assert "unrep" in outcomes and "ok" in outcomes
    for o, c in zip(outcomes, cases):
        if c[0].startswith("malicious"):
            assert o != "ok" and o != "badroot", c[0]
        else:
            assert o in ("ok", "unrep"), c[0]


# ------------------------------------------------------------------ CPU: the oracle
@pytest.mark.parametrize("k", [2, 4, 8])
def test_oracle_unordered_square_outcomes(k):
    """The pre-repair check must not leak PushOrderError: the first complete unordered vector is byzantine, as the
    rebuilt one is."""
    for name, sq, p, want, how in unordered_cases(k):
        info = {}
        assert run_oracle(sq.eds, p, sq.rows, sq.cols, info)[0] == want, name
        assert info["how"] == how, name


@pytest.mark.parametrize("k", [2, 4, 8])
def test_oracle_matrix_meets_the_coverage_conditions(k):
    check_coverage(k, [c[3] for c in matrix(k)])
    # the two-hole mask on the default cell is the orthogonal parity-only case, named through column 0's rebuild
    hit = [c for c in matrix(k) if c[0] == f"malicious {ref.flipped_cell(k)}, two holes"]
    assert len(hit) == 1 and hit[0][3] == ("byz", orp.ROW, k - 1) and hit[0][4] == "orth-parity"


def test_generalised_malicious_square_keeps_its_default():
    k = 4
    assert ref.malicious_square(k) is not None and ref.flipped_cell(k) in ref.flipped_cells(k)
    assert np.array_equal(ref.malicious_square(k).eds, ref.malicious_square(k, ref.flipped_cell(k)).eds)
    assert ref.malicious_square(k).rows == ref.malicious_square(k, ref.flipped_cell(k)).rows
    for r, c in ref.flipped_cells(k):
        sq = ref.malicious_square(k, (r, c))
        H = ref.honest_square(k)
        diff = np.argwhere((sq.eds != H.eds).any(axis=2))
        assert diff.tolist() == [[r, c]]
        assert [i for i in range(2 * k) if sq.rows[i] != H.rows[i]] == [r]
        assert [j for j in range(2 * k) if sq.cols[j] != H.cols[j]] == [c]


# ------------------------------------------------------------------ GPU: the matrix
def fraud_proof_chain(ctx, label, sq, p, want, square):
    """Where the held cells alone prove at least k shares of the named vector, the proof built from the square the
    GPU returned confirms the fraud against the committed DAH, on the GPU and on the CPU yardstick."""
    from celestia_da import byzantine
    _, axis, index = want
    k = sq.k
    held = np.where(p[..., None], sq.eds, 0).astype(np.uint8)
    if len(ref.build(held, sq.rows, sq.cols, axis, index)) < k:
        return False
    proof = byzantine.build_bad_encoding_proof(square, sq.rows, sq.cols, axis, index, ctx=ctx)
    assert byzantine.validate_bad_encoding_proofs([proof], [sq.dah()], ctx) == [None], label
    assert ref.validate(proof, sq.rows, sq.cols)[0] == ref.VALID, label
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_malicious_commitment_matrix(ctx, k):
    cases = matrix(k)
    got = {"host": [], "device": []}
    chained = 0
    for label, sq, p, want, _how, _complete in cases:
        for entry, fn in (("host", gpu_repair), ("device", device_repair)):
            info = {}
            o, rep = fn(ctx, sq.eds, p, sq.rows, sq.cols, info)
            assert o == want, (entry, label, o, want)
            got[entry].append(o)
            if o == "ok":
                assert np.array_equal(rep, sq.eds), (entry, label)
            elif isinstance(o, tuple):
                chained += fraud_proof_chain(ctx, f"{entry}: {label}", sq, p, want, info["square"])
    if k < 16:
        check_coverage(k, got["host"])
        check_coverage(k, got["device"])
    assert chained > 0


# ------------------------------------------------------------------ GPU: unordered squares
def unordered_cases(k):
    """[(name, square, present, outcome, the oracle's check that gives it)].  The square with row 0 descending, and
    its transpose (column 0 descending, the roots of the two axes exchanged: extension and trees are symmetric in
    the axes), which reaches the one branch the first cannot: row 0 is visited before column 0, so its rebuild
    completes the unordered column."""
    W = 2 * k
    sq, row = ref.unordered_square(k)
    assert row == 0
    tr = ref.Square(np.ascontiguousarray(sq.eds.transpose(1, 0, 2)), sq.cols, sq.rows)
    full = np.ones((W, W), dtype=bool)
    hole = full.copy()
    hole[0, k] = False
    corner = full.copy()
    corner[0, 0] = False
    r0, c0 = ("byz", orp.ROW, 0), ("byz", orp.COL, 0)
    return [("every cell present", sq, full, r0, "check-order"),
            ("one hole in row 0", sq, hole, r0, "rebuilt-order"),
            ("Q0 withheld", sq, quadrant_withheld(k, 0), r0, "rebuilt-order"),
            ("transposed, every cell present", tr, full, c0, "check-order"),
            ("transposed, hole at (0, 0)", tr, corner, c0, "orth-order"),
            ("transposed, Q0 withheld", tr, quadrant_withheld(k, 0), c0, "rebuilt-order")]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4, 8])
def test_unordered_square_is_byzantine(ctx, k):
    """A properly encoded square with a descending row 0, committed over blind trees: every root and every parity
    check passes, and row 0 is byzantine all the same, complete in the input or rebuilt; likewise column 0 of the
    transposed square, complete in the input or completed by row 0's rebuild."""
    wrong = []
    for name, sq, p, want, _how in unordered_cases(k):
        assert run_oracle(sq.eds, p, sq.rows, sq.cols)[0] == want
        for entry, fn in (("host", gpu_repair), ("device", device_repair)):
            got, _ = fn(ctx, sq.eds, p, sq.rows, sq.cols)
            print(f"unordered k={k} {name}: {entry} -> {got}")
            if got != want:
                wrong.append((entry, name, got))
    assert not wrong, wrong


# ------------------------------------------------------------------ GPU: GF(2^16)
@functools.lru_cache(maxsize=None)
def gf16_square():
    import coracle
    k = 256
    W = 2 * k
    r, c = ref.flipped_cell(k)
    eds = coracle.extend(coracle.random_square(k, 3)).reshape(W, W, 512).copy()
    eds[r, c, 100:104] ^= 0x5A
    rows, cols, _ = coracle.blind_dah(eds, k)
    return eds, [bytes(x) for x in rows], [bytes(x) for x in cols]


@pytest.mark.gpu
@pytest.mark.parametrize("q", [3, 1])
def test_gf16_malicious_square(ctx, q):
    """k = 256, cell (k - 1, k) flipped under recomputed roots.  Q3 withheld: rows and columns 0..k-1 are complete
    and the pre-repair check reaches row k - 1 first (root equal, parity not).  Q1 withheld: the replay rebuilds rows
    0..k-1, and the honest rebuild of row k - 1 misses the committed root.  Both follow from the visiting order, as
    the oracle's runs at k = 2..8 show (test_oracle_gf16_expectations_at_small_k)."""
    k = 256
    eds, rows, cols = gf16_square()
    assert gpu_repair(ctx, eds, quadrant_withheld(k, q), rows, cols)[0] == ("byz", orp.ROW, k - 1)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_oracle_gf16_expectations_at_small_k(k):
    sq = ref.malicious_square(k)
    for q, how in ((3, "check-parity"), (1, "rebuilt-root")):
        info = {}
        assert run_oracle(sq.eds, quadrant_withheld(k, q), sq.rows, sq.cols, info)[0] == ("byz", orp.ROW, k - 1)
        assert info["how"] == how


# ------------------------------------------------------------------ GPU: the bad-root text
@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 8])
def test_bad_root_error_text_is_the_oracles(ctx, k):
    """A held cell corrupted under the honest DAH, its row or column complete: the whole error text, expected and
    computed root in hex included, equals the oracle's ErrBadRoot."""
    H = ref.honest_square(k)
    W = 2 * k
    full = np.ones((W, W), dtype=bool)
    for r, c, hole in ((1, 0, None), (k, W - 1, (k, 0)), (W - 1, k - 1, (0, k - 1))):
        bad = H.eds.copy()
        bad[r, c, 200] ^= 0x11
        p = full.copy()
        if hole:
            p[hole] = False   # row r, or column c, incomplete: the other one is named
        oi = {}
        assert run_oracle(bad, p, H.rows, H.cols, oi)[0] == "badroot"
        assert oi["error"].startswith("bad root input: ") and len(oi["error"]) > 2 * 180
        for entry, fn in (("host", gpu_repair), ("device", device_repair)):
            gi = {}
            assert fn(ctx, bad, p, H.rows, H.cols, gi)[0] == "badroot", (entry, r, c)
            assert gi["error"] == oi["error"], (entry, r, c)
