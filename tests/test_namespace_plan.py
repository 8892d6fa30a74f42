"""The host half of the namespace query (csrc/namespace_proofs_plan.h): the search's words to segments,
offsets and sizes, and the queries' check.  No GPU: tools/namespace_plan_host_test.cpp is compiled by the host
compiler and its lines are compared with values worked out by hand for a k = 4 square (row trees of 8 leaves,
D = 3: a proof of [s, e) has popcount(s) + 3 - popcount(e - 1) nodes).
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

EXPECTED = {
    "P none": "0 0 0 | 0 |",
    "P unselected": "0 0 0 | 0 0 |",
    # [1, 4): 1 + 3 - 2 = 2 nodes; [0, 4): 0 + 3 - 2 = 1; [0, 1): 3; absence of leaf 2, [2, 3): 1 + 3 - 1 = 3; [0, 1): 3
    "P mixed": "5 12 9 | 0 3 3 5 | 0 1 1 4 1 0 2 0 4 1 0 3 0 1 1 2 0 2 3 2 2 1 0 1 1",
    "E absence_at_k": "query 0: row 0: search word 2147483652 is not one of a square of width 4",
    "E too_many": "query 1: row 1: search word 2147491843 is not one of a square of width 4",
    "E check_ok": "",
    "E check_parity": "query 1: namespace is the parity shares namespace",
    "E check_null": "null buffer",
    "E check_width": "square width 3 is not a power of two <= 1024",
}


@pytest.fixture(scope="module")
def lines():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "namespace_plan_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "namespace_plan_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict((x.split(" :", 1)[0], x.split(" :", 1)[1].strip()) for x in r.stdout.splitlines())


def test_plan_equals_the_values_worked_out_by_hand(lines):
    assert lines == EXPECTED
