"""cda_befp_batch_check: the structural checks of a fraud-proof batch.  Host only (no context, no device work), so
it runs without a GPU; the same batches through cda_befp_verify are in tests/test_befp.py."""
import ctypes as C

import numpy as np
import pytest

import befp_ref as ref
from celestia_da import _lib, byzantine

K = 2


def good_proofs():
    sq = ref.malicious_square(K)
    r, c = ref.flipped_cell(K)
    return [ref.prove(sq, ref.ROW, r, range(2 * K)), ref.prove(sq, ref.COL, c, range(K))], [sq.dah(), sq.dah()]


def packed():
    proofs, dahs = good_proofs()
    return byzantine.pack_batch(proofs, dahs)


# (what to break in the packed arrays, the text cda_last_error then gives)
MALFORMED = [
    ("k3", "k 3 is not a power of two <= 512"),
    ("k1024", "k 1024 is not a power of two <= 512"),
    ("axis", "proof 1: axis 2 is neither 0 (row) nor 1 (column)"),
    ("index", "proof 0: index 4 is not below the EDS width 4"),
    ("position", "proof 1: share 1: position 4 is not below the EDS width 4"),
    ("ascending", "proof 0: share 2: position 1 is not above the one before it, 1: positions must be strictly "
                  "ascending"),
    ("descending", "proof 0: share 1: position 0 is not above the one before it, 1: positions must be strictly "
                   "ascending"),
    ("off_start", "proof 0: share_off must start at 0"),
    ("off_decreases", "proof 1: share_off decreases"),
]


def break_batch(what, b, keep):
    axes, indexes, rows, cols, off, positions, proof_axes, shares, nodes = keep
    if what == "k3":
        b.k = 3
    elif what == "k1024":
        b.k = 1024
    elif what == "axis":
        axes[1] = 2
    elif what == "index":
        indexes[0] = 2 * K
    elif what == "position":
        positions[off[1] + 1] = 2 * K
    elif what == "ascending":
        positions[2] = positions[1]
    elif what == "descending":
        positions[0], positions[1] = 1, 0
    elif what == "off_start":
        off[0] = 1
    elif what == "off_decreases":
        off[2] = off[1] - 1


def test_well_formed_batch_passes():
    b, keep = packed()
    assert byzantine.batch_check(b) is None
    assert _lib.load().cda_last_error(None) == b""
    del keep


def test_empty_batch_passes():
    assert byzantine.batch_check(_lib.BefpBatch()) is None


def test_null_batch():
    lib = _lib.load()
    assert lib.cda_befp_batch_check(None) == _lib.CDA_ERR_INVALID
    assert lib.cda_last_error(None) == b"null batch"


@pytest.mark.parametrize("what,text", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_field_is_named(what, text):
    b, keep = packed()
    break_batch(what, b, keep)
    lib = _lib.load()
    assert lib.cda_befp_batch_check(C.byref(b)) == _lib.CDA_ERR_INVALID
    assert lib.cda_last_error(None).decode() == text


def test_null_proof_axes_means_orthogonal():
    b, keep = packed()
    b.proof_axes = None
    assert byzantine.batch_check(b) is None
    del keep


def test_python_structural_checks_have_their_own_texts():
    proofs, dahs = good_proofs()
    p = proofs[0].copy()
    p.positions[1] = p.positions[0]
    assert byzantine.structural_error(p) == "positions are not strictly ascending"
    p = proofs[0].copy()
    p.k = 3
    assert byzantine.structural_error(p) == "square width 3 is not a power of two <= 512"
    p = proofs[0].copy()
    p.index = 4
    assert byzantine.structural_error(p) == "index 4 is outside the EDS width 4"
    p = proofs[0].copy()
    p.axis = 2
    assert byzantine.structural_error(p) == "axis 2 is neither 0 (row) nor 1 (column)"
    p = proofs[0].copy()
    p.positions[3] = 9
    assert byzantine.structural_error(p) == "a position is outside the EDS width 4"
    assert byzantine.structural_error(proofs[0]) is None and byzantine.structural_error(proofs[1]) is None
    # a malformed proof gets its text without any library call (there is no GPU here)
    p = proofs[0].copy()
    p.axis = 2
    assert byzantine.validate_bad_encoding_proofs([p], [dahs[0]]) == ["axis 2 is neither 0 (row) nor 1 (column)"]
