"""csrc/tree_index.h (the proof paths' index arithmetic) against the oracle.

tools/tree_index_host_test.cpp prints prove_nodes for every range of every
tree of 1..33 leaves, level_counts, and level_offset for the resident-square
widths 2, 4, 16 and 2048 (rows and columns); compared here with a recursion
over oracle.proofs.split_point and with the plain sums W * (W >> l) * 96.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

import proofs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")


def _prove_nodes(n, start, end):
    """Maximal subtrees outside [start, end), depth first, left to right: the
    subtree [lo, hi) of size 2^L is node (L, lo >> L); a last subtree cut short
    by n is the promoted node of the level of its full size."""
    out = []

    def rec(lo, hi):
        if hi <= start or lo >= end:
            level = (hi - lo - 1).bit_length()
            out.append((level, lo >> level))
            return
        if hi - lo == 1:
            return
        k = proofs.split_point(hi - lo)
        rec(lo, lo + k)
        rec(lo + k, hi)

    rec(0, n)
    return out


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
def test_tree_index_host():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tree_index_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "tree_index_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    proved, counts, offsets = {}, {}, {}
    for line in r.stdout.splitlines():
        kind, *f = line.replace(":", " ").split()
        v = [int(x) for x in f]
        if kind == "P":
            proved[tuple(v[:3])] = list(zip(v[3::2], v[4::2]))
        elif kind == "C":
            counts[v[0]] = v[1:]
        else:
            assert kind == "O", line
            offsets[tuple(v[:3])] = v[3]

    assert sorted(counts) == list(range(1, 34))
    assert len(proved) == sum(n * (n + 1) // 2 for n in range(1, 34))
    for n in range(1, 34):
        want, m = [n], n
        while m > 1:
            m = (m + 1) // 2
            want.append(m)
        assert counts[n] == want, n
        for start in range(n):
            for end in range(start + 1, n + 1):
                got = proved[(n, start, end)]
                assert got == _prove_nodes(n, start, end), (n, start, end)
                # every node exists in its level
                assert all(i < counts[n][lv] for lv, i in got), (n, start, end, got)

    for W in (2, 4, 16, 2048):
        log_w = W.bit_length() - 1
        for first in (0, 1):
            for L in range(first, log_w + 2):
                want = sum(W * (W >> l) * 96 for l in range(first, L))
                assert offsets[(W, first, L)] == want, (W, first, L)
    assert len(offsets) == sum(2 * (W.bit_length() + 1) - 1 for W in (2, 4, 16, 2048))
