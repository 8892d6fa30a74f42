"""The closed-form range proof of csrc/tree_index.h (range_proof_count /
range_proof_node) and the host-only plan of a batch of share proofs
(csrc/share_proofs_plan.h, cda_square_share_proofs_plan).  No GPU.

tools/range_proof_host_test.cpp prints range_proof_node for every range of
the perfect trees of 1 .. 64 leaves and for spot checks at 2 048 leaves, and
compares each with prove_nodes itself; here the lines are compared with a
recursion over oracle.proofs.split_point.  The plan's sizes are compared with
batches sized by hand, through the program and through the library's call.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

from celestia_da import CdaError, _lib
from test_tree_index import _prove_nodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

SPOT = [(s, e) for s in (0, 1, 1023, 1024, 2047) for e in (s + 1, 1024, 2048) if e > s]

# (k, ranges) -> (n_segments, n_nodes, n_aunts, aunts_per_segment, n_shares), sized by hand:
#   k = 1 (W = 2, D = 1, 2 aunts): [0, 1) has the one sibling.
#   k = 2 (D = 2, 3 aunts): [0, 2) ends at a row end: 1 node (the parity half).  [1, 3) crosses a
#     row end: (1, 2) has the leaf on its left and the parity half, (0, 1) of row 1 the leaf on its
#     right and the parity half: 4 nodes.  [0, 4) is both whole rows: 1 node each.  [3, 4) = (1, 2)
#     of row 1: 2 nodes.  6 segments, 9 nodes, 18 aunts, 9 shares.
#   k = 4 (D = 3, 4 aunts): [2, 4) ends exactly at the end of row 0: leaves [0, 2) and the parity
#     half, 2 nodes.  [4, 6) starts at the start of row 1: leaves [2, 4) and the parity half, 2.
#     [3, 11) spans three rows: (3, 4) of row 0 has [0, 2), leaf 2 and the parity half (3), the whole
#     row 1 the parity half (1), (0, 3) of row 2 leaf 3 and the parity half (2): 6 nodes, 8 shares.
#     [0, 16): four whole rows, 4 nodes.  [5, 6) = (1, 2) of row 1: leaf 0, [2, 4), parity: 3.
#     10 segments, 17 nodes, 40 aunts, 29 shares.
#   k = 128 (D = 8, 9 aunts): the whole square is 128 whole rows of 1 node; [0, 1) has 8 siblings.
PLANS = [
    (1, [(0, 1)], (1, 1, 2, 2, 1)),
    (2, [(0, 2), (1, 3), (0, 4), (3, 4)], (6, 9, 18, 3, 9)),
    (4, [(2, 4), (4, 6), (3, 11), (0, 16), (5, 6)], (10, 17, 40, 4, 29)),
    (4, [], (0, 0, 0, 4, 0)),
    (128, [(0, 128 * 128), (0, 1)], (129, 136, 1161, 9, 16385)),
]
ERRORS = [
    (4, [(0, 1), (5, 5), (3, 4)], "range 1: start 5 is not below end 5"),
    (4, [(0, 1), (7, 6)], "range 1: start 7 is not below end 6"),
    (8, [(0, 1), (1, 2), (2, 3), (3, 70)], "range 3: end 70 is beyond the 64 shares of the original square"),
    (3, [(0, 1)], "square width 3 is not a power of two <= 1024"),
    (2048, [(0, 1)], "square width 2048 is not a power of two <= 1024"),
    (0, [(0, 1)], "square width 0 is not a power of two <= 1024"),
]
# 349 526 whole k = 1024 squares: 12 aunts for each of 357 914 624 segments pass 2^32 at the last range
OVERFLOW = (1024, 349526, "range 349525: aunt offset 4294975488 does not fit the batch's 32-bit offsets")


@pytest.fixture(scope="module")
def host_program_output():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "range_proof_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "range_proof_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_closed_form_equals_the_recursion(host_program_output):
    proved = {}
    for line in host_program_output:
        if line.startswith("R "):
            v = [int(x) for x in line[2:].replace(":", " ").split()]
            proved[tuple(v[:3])] = list(zip(v[3::2], v[4::2]))
    widths = [1, 2, 4, 8, 16, 32, 64]
    assert len(proved) == sum(W * (W + 1) // 2 for W in widths) + len(set(SPOT))
    for W in widths:
        D = W.bit_length() - 1
        for s in range(W):
            for e in range(s + 1, W + 1):
                got = proved[(W, s, e)]
                assert got == _prove_nodes(W, s, e), (W, s, e)
                assert len(got) == bin(s).count("1") + D - bin(e - 1).count("1")
                assert len(got) <= (2 * (D - 1) if D >= 2 else D)
    for s, e in SPOT:
        assert proved[(2048, s, e)] == _prove_nodes(2048, s, e), (s, e)
    # one share: the sibling rule of the sampling kernel
    for p in range(64):
        assert sorted(proved[(64, p, p + 1)]) == [(L, (p >> L) ^ 1) for L in range(6)]


def test_plan_in_the_host_program(host_program_output):
    lines = [x for x in host_program_output if x[:2] in ("P ", "E ")]
    want = [f"P {k} {len(r)} : " + " ".join(str(x) for x in sizes) for k, r, sizes in PLANS]
    want += [f"E {k} : {msg}" for k, _, msg in ERRORS]
    want.append(f"E {OVERFLOW[0]} : {OVERFLOW[2]}")
    assert sorted(lines) == sorted(want)


@pytest.mark.parametrize("k,ranges,sizes", PLANS)
def test_plan_sizes(k, ranges, sizes):
    from celestia_da import proof as gpr
    p = gpr.share_proofs_plan(k, ranges)
    assert tuple(p[n] for n in ("n_segments", "n_nodes", "n_aunts", "aunts_per_segment", "n_shares")) == sizes
    # the sum of end_row - start_row + 1, and log2(4k) aunts per segment
    assert p["n_segments"] == sum((e - 1) // k - s // k + 1 for s, e in ranges)
    assert p["n_aunts"] == p["n_segments"] * ((4 * k).bit_length() - 1)
    assert p["n_shares"] == sum(e - s for s, e in ranges)


@pytest.mark.parametrize("k,ranges,msg", ERRORS)
def test_plan_errors(k, ranges, msg):
    from celestia_da import proof as gpr
    with pytest.raises(CdaError) as e:
        gpr.share_proofs_plan(k, ranges)
    assert e.value.code == _lib.CDA_ERR_INVALID and str(e.value) == msg


def test_plan_offset_overflow_and_untouched_output():
    import ctypes as C

    import numpy as np
    from celestia_da import proof as gpr
    k, n, msg = OVERFLOW
    ranges = np.zeros((n, 2), dtype=np.int64)
    ranges[:, 1] = k * k
    with pytest.raises(CdaError) as e:
        gpr.share_proofs_plan(k, ranges)
    assert e.value.code == _lib.CDA_ERR_INVALID and str(e.value) == msg
    assert gpr.share_proofs_plan(k, ranges[:-1])["n_aunts"] == (n - 1) * 1024 * 12
    # an error leaves *out as it was; a NULL out is an error too
    L = _lib.load()
    p = _lib.ShareProofsPlanT(7, 7, 7, 7, 7)
    one = (C.c_uint32 * 1)(5)
    assert L.cda_square_share_proofs_plan(4, one, one, 1, C.byref(p)) == _lib.CDA_ERR_INVALID
    assert (p.n_segments, p.n_nodes, p.n_aunts, p.aunts_per_segment, p.n_shares) == (7, 7, 7, 7, 7)
    assert L.cda_square_share_proofs_plan(4, one, one, 1, None) == _lib.CDA_ERR_INVALID
    assert L.cda_square_share_proofs_plan(4, None, None, 1, C.byref(p)) == _lib.CDA_ERR_INVALID
    assert L.cda_square_share_proofs_plan(4, None, None, 0, C.byref(p)) == _lib.CDA_OK and p.n_segments == 0


def test_symbols_and_python_surface():
    from celestia_da import proof as gpr
    assert {"cda_square_share_proofs_plan", "cda_square_share_proofs"} <= set(_lib.EXPORTED)
    assert hasattr(gpr.ResidentSquare, "share_proofs_batch")
    for name in ("ShareProofsBatch", "share_proofs_plan", "new_share_inclusion_proofs", "new_tx_inclusion_proofs"):
        assert hasattr(gpr, name), name
    # the output struct carries the batch struct's names, so filling one from the other is assignment
    batch = {n for n, _ in _lib.ShareProofBatch._fields_}
    out = {n for n, _ in _lib.ShareProofsOut._fields_}
    assert out - batch == {"start_row", "end_row", "one_namespace"}
    assert {n: t for n, t in _lib.ShareProofsOut._fields_ if n in batch} == \
        {n: t for n, t in _lib.ShareProofBatch._fields_ if n in out}


def test_tx_inclusion_proofs_index_errors():
    """new_tx_inclusion_proofs checks its indexes as new_tx_inclusion_proof does, before any GPU work."""
    from celestia_da import proof as gpr
    with pytest.raises(CdaError, match="txIndex 0 out of bounds"):
        gpr.new_tx_inclusion_proofs([], [0])
    with pytest.raises(CdaError, match="txIndex 2 out of bounds"):
        gpr.new_tx_inclusion_proofs([b"x", b"y"], [0, 2])
    with pytest.raises(CdaError, match="txIndex -1 is negative"):
        gpr.new_tx_inclusion_proofs([b"x"], [-1])
    assert gpr.new_tx_inclusion_proofs([], None) == []
