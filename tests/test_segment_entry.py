"""The `row` word of a segment table entry (csrc/segment_table.h): the row in the low sixteen bits, the square of
a set above it.  No GPU: tools/segment_entry_host_test.cpp is compiled by the host compiler and its lines are
compared with values worked out by hand: word = row + 65536 * square (65534 * 65536 = 2^32 - 131072 =
4294836224), the range word 5 | 9 << 16 = 589829 with the absence flag 2^31 or the subtree flag 2^30 added, the
64-bit share offset 0x123456789 as the words 0x23456789 = 591751049 and 1.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

EXPECTED = {
    "S size": "32 8",
    "W 0 0": "0 0 0",
    "W 0 1": "65536 0 1",
    "W 0 65534": "4294836224 0 65534",
    "W 1 0": "1 1 0",
    "W 1 1": "65537 1 1",
    "W 1 65534": "4294836225 1 65534",
    "W 2047 0": "2047 2047 0",
    "W 2047 1": "67583 2047 1",
    "W 2047 65534": "4294838271 2047 65534",
    "E 0": "4294838271 589829 7 11 591751049 1 13 4294967295 | 2047 65534 5 9 0 0",
    "E 2": "4294838271 2148073477 7 11 591751049 1 13 4294967295 | 2047 65534 5 9 1 0",
    "E 1": "4294838271 1074331653 7 11 591751049 1 13 4294967295 | 2047 65534 5 9 0 1",
    "Z single": "77 2047",
    "M max": "65535 65534",
}


@pytest.fixture(scope="module")
def lines():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "segment_entry_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "segment_entry_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict((x.split(" :", 1)[0], x.split(" :", 1)[1].strip()) for x in r.stdout.splitlines())


def test_row_word_equals_the_values_worked_out_by_hand(lines):
    assert lines == EXPECTED


def test_the_set_limit_fits_the_word():
    """CDA_SET_MAX_SQUARES of include/cda.h is what the high half of the word can name."""
    with open(os.path.join(ROOT, "include", "cda.h")) as f:
        assert "#define CDA_SET_MAX_SQUARES 65535" in f.read()
