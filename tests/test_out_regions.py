"""The layout of a resident-square call's outputs in its scratch buffer
(csrc/out_regions.h), which the sampling and the share-proof calls share.
No GPU.

tools/out_regions_host_test.cpp lays out a few calls, prints every region and
checks each layout itself (alignment, no overlap, the covering span, and that
one copy of the span followed by memcpys delivers the bytes of one copy per
region); here the printed numbers are compared with layouts worked out by
hand.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

# name -> (total, (span offset, span bytes), [(offset, bytes, device offset or -1)], [(offset, bytes) to copy]).
# Every region starts at the next multiple of 16 behind the upload and the regions before it.
#   samples: 20 bytes of coordinates end at 32; 2560 -> 2592; 145 takes 160 -> 2752; 900 takes 912 -> 3664;
#     450 takes 464 -> 4128; 160 -> 4288; 480 -> 4768.  The span is [32, 4768).
#   null: the same without the second and the fourth: they take no room, have no device pointer and are not copied.
#   zero: a requested output of no bytes keeps its device pointer, takes no room and is not copied.
#   none / empty: nothing to copy, the span is empty; the upload alone is rounded up (33 -> 48).
#   flags: a 100-byte upload (-> 112) whose bytes [96, 99) are an output themselves: the span starts inside the
#     upload, [96, 384 + 29).  flags_only / no_flags: that output alone, and without it.
EXPECTED = {
    "samples": (4768, (32, 4736),
                [(32, 2560, 32), (2592, 145, 2592), (2752, 900, 2752), (3664, 450, 3664), (4128, 160, 4128),
                 (4288, 480, 4288)],
                [(32, 2560), (2592, 145), (2752, 900), (3664, 450), (4128, 160), (4288, 480)]),
    "null": (4144, (32, 4112),
             [(32, 2560, 32), (2592, 0, -1), (2592, 900, 2592), (3504, 0, -1), (3504, 160, 3504), (3664, 480, 3664)],
             [(32, 2560), (2592, 900), (3504, 160), (3664, 480)]),
    "zero": (48, (16, 29), [(16, 0, 16), (16, 29, 16), (48, 0, 48)], [(16, 29)]),
    "none": (48, (0, 0), [(48, 0, -1), (48, 0, -1)], []),
    "empty": (0, (0, 0), [], []),
    "flags": (416, (96, 317), [(112, 270, 112), (384, 0, -1), (384, 29, 384), (96, 3, 96)],
              [(112, 270), (384, 29), (96, 3)]),
    "flags_only": (112, (96, 3), [(112, 0, -1), (96, 3, 96)], [(96, 3)]),
    "no_flags": (208, (112, 90), [(112, 90, 112), (96, 0, -1)], [(112, 90)]),
}


@pytest.fixture(scope="module")
def host_program_output():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "out_regions_host_test")
        subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tools", "out_regions_host_test.cpp"), "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def _numbers(text, per):
    v = [int(x) for x in text.split()]
    assert len(v) % per == 0
    return [tuple(v[i:i + per]) for i in range(0, len(v), per)]


def test_layouts_equal_the_ones_worked_out_by_hand(host_program_output):
    layouts, copies = {}, {}
    for line in host_program_output:
        kind, name, rest = line[0], line[2:].split(" :", 1)[0], line.split(" :", 1)[1]
        if kind == "L":
            head, regions = rest.split("|")
            total, off, size = (int(x) for x in head.split())
            layouts[name] = (total, (off, size), _numbers(regions, 3))
        else:
            assert kind == "C"
            copies[name] = _numbers(rest, 2)
    assert set(layouts) == set(copies) == set(EXPECTED)
    for name, (total, span, regions, copy) in EXPECTED.items():
        assert layouts[name] == (total, span, regions), name
        assert copies[name] == copy, name


def test_expected_layouts_follow_the_rules():
    """The hand-made table itself: 16-byte boundaries, total behind the last region, the span around the copies."""
    for name, (total, span, regions, copy) in EXPECTED.items():
        assert total % 16 == 0, name
        assert copy == [(o, b) for o, b, _ in regions if b], name
        assert all((d == -1 and b == 0) or d == o for o, b, d in regions), name
        if copy:
            lo, hi = min(o for o, _ in copy), max(o + b for o, b in copy)
            assert span == (lo, hi - lo) and hi <= total, name
        else:
            assert span == (0, 0), name
