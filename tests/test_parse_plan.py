"""The host half of the share parser (csrc/parse_plan.h): digests, the sequence
table and its checks, the share-count rules, the unit walk with the
reserved-bytes check and every error text.  No GPU:
tools/parse_plan_host_test.cpp is compiled by the host compiler and its lines
are compared with values worked out by hand on squares of at most 16 shares.

The "simple" square: 0 tx {abc, de} (stream 03 abc 02 de, L = 7); 1 pfb {wxyz} (L = 5); 2 reserved padding;
3 a blob of 1 byte; 4-5 a blob of 479 bytes; 6 a namespace-padding share in that blob's namespace; 7 tail padding.
Digest word 0 = info | class << 8 | same-namespace << 16 with class 1 TX, 2 PFB, 4 padding namespace.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

EXPECTED = {
    # share 5 is a continuation (info 0) in share 4's namespace: 1 << 16; its bytes [30, 34) are 66 00 00 00;
    # share 6 is a start share in the same namespace: 1 | 1 << 16; the last two: share 0's reserved bytes, share 5's
    "D simple": "257 7 | 513 5 | 1025 0 | 1 1 | 1 479 | 65536 1711276032 | 65537 0 | 1025 0 | 38 1711276032",
    "T simple": "2 3 480 12 | 0 1 7 1 | 1 1 5 2 | 3 1 1 0 | 4 2 479 0",
    # offsets in the packed compact streams (the PFB's follows the 7 bytes of the TX one), lengths, share ranges
    "U simple": "2 1 9 | 1 3 0 1 | 5 2 0 1 | 8 4 1 2",
    "T ranges": "2 1 480 0 | 3 1 1 0 | 4 2 479 0",
    "E range_at_continuation": "share 5: the first share of range 1 is a continuation share",
    "E range_cuts_sequence": "sequence at share 4: length 479 needs 2 shares, found 1",
    "T none": "0 0 0 0",
    "N sparse": "1 1 2 2 3",        # 1, 478, 479, 960, 961 bytes
    "N compact": "1 1 2 2 3",       # 1, 474, 475, 952, 953 bytes
    # stream bytes 473, 474, 951, 952 lie in shares 0, 1, 1, 2; bytes 0, 473, 474, 952 at share offsets 38, 511, 34, 34
    "C stream": "0 1 1 2 | 38 511 34 34",
    "E parity": "share 6: parity-namespace share",
    "E version": "share 3: unsupported share version 1",
    "E first_continuation": "share 0: the first share of the input is a continuation share",
    "E namespace_differs": "share 5: continuation share's namespace differs from that of its sequence's start share 4",
    "E too_few": "sequence at share 4: length 479 needs 2 shares, found 1",
    "E too_many": "sequence at share 4: length 479 needs 2 shares, found 3",
    "E padding_continued": "sequence at share 6: length 0 needs 1 shares, found 2",
    "E compact_count": "sequence at share 0: length 475 needs 2 shares, found 1",
    # L = 600 at shares 2-3: d7 03 = 471 bytes at 2; prefix 100 at stream 473 = byte 511 of share 2, its bytes
    # 474..573 all in share 3; prefix 25 at stream 574 = byte 34 + 100 of share 3
    "U straddle": "3 0 596 | 2 471 2 3 | 474 100 2 4 | 575 25 3 4",
    "E reserved_bytes": "share 3: reserved bytes 34, expected 134",
    "U zero_ends_the_walk": "1 0 2 | 1 2 0 1",
    "E malformed_prefix": "share 2: malformed unit length prefix",
    "E prefix_cut_by_length": "share 0: malformed unit length prefix",
    "E unit_past_length": "share 0: unit of 80 bytes runs past the sequence length 61",
    "E reserved_zero": "share 0: reserved bytes 0, expected 38",
    "E ranges_ok": "",
    "E ranges_order": "range 2: start 4 is below the end 12 of the range before it",
    "E ranges_beyond": "range 1: end 12 is beyond the 10 shares of the original square",
    "E ranges_empty": "range 0: start 4 is not below end 0",
    "E ranges_null": "null buffer",
}


@pytest.fixture(scope="module")
def lines():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "parse_plan_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "parse_plan_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return dict((x.split(" :", 1)[0], x.split(" :", 1)[1].strip()) for x in r.stdout.splitlines())


def test_parse_plan_equals_the_values_worked_out_by_hand(lines):
    assert lines == EXPECTED
