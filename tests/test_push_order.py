"""csrc/push_order.h (the push-order word) against the reference's order of
checks, on the CPU.

tools/push_order_host_test.cpp prints encode / decode / fill_status at the
corners of the layout and the minimum of a set of violation words.  The
reference pushes every row tree, then every column tree, each from its first
leaf, and stops at the first namespace below its predecessor's: the first
violation is the smallest (axis, index, position) tuple.  The device keeps the
minimum word per square, so the word order must be that tuple order.
"""
import functools
import os
import random
import shutil
import subprocess
import tempfile

import pytest

from celestia_da import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")
ORDERED = 0xFFFFFFFF

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@functools.lru_cache(maxsize=None)
def _exe():
    import atexit
    d = tempfile.mkdtemp(prefix="push_order_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "push_order_host_test")
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tools", "push_order_host_test.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _run(*args):
    r = subprocess.run([_exe(), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return [line.split() for line in r.stdout.splitlines()]


@functools.lru_cache(maxsize=None)
def _dump():
    enc, dec, status = {}, {}, {}
    for tag, *f in _run():
        v = [int(x) for x in f]
        if tag == "E":
            enc[tuple(v[:3])] = v[3]
        elif tag == "D":
            dec[v[0]] = tuple(v[1:])
        else:
            assert tag == "S", tag
            status[v[0]] = v[1]
    return enc, dec, status


def test_round_trip_at_the_corners():
    enc, dec, _ = _dump()
    corners = [(a, i, p) for a in (0, 1) for i in (0, 4095) for p in (1, 4095)]
    assert all(c in enc for c in corners)
    for v, w in enc.items():
        assert dec[w] == v, v
    assert len(set(enc.values())) == len(enc) and ORDERED not in enc.values()
    assert dec[ORDERED] == (-1, 0, 0)


def test_word_layout_is_the_documented_one():
    enc, _, _ = _dump()
    for (a, i, p), w in enc.items():
        assert w == a << 24 | i << 12 | p
    # the value tests/test_dist.py hard-codes for row 1, push position 3
    assert enc[(0, 1, 3)] == (0 << 24) | (1 << 12) | 3 == 4099


def test_rows_sort_below_columns():
    enc, _, _ = _dump()
    rows = [w for (a, _, _), w in enc.items() if a == 0]
    cols = [w for (a, _, _), w in enc.items() if a == 1]
    assert max(rows) < min(cols) and max(cols) < ORDERED
    assert sorted(enc, key=enc.get) == sorted(enc)   # word order == (axis, index, position) order


def test_minimum_is_the_reference_first_violation():
    rng = random.Random(7)
    sets = [[(1, 0, 1), (0, 4095, 4095)],                       # any row violation before any column violation
            [(0, 5, 2), (0, 4, 4095)],                          # then the lower tree
            [(1, 9, 7), (1, 9, 6), (1, 10, 1)],                 # then the earlier push
            [(0, 0, 1)], [(1, 4095, 4095)]]
    for _ in range(20):
        sets.append([(rng.randrange(2), rng.randrange(4096), rng.randrange(1, 4096))
                     for _ in range(rng.randrange(1, 12))])
    for s in sets:
        (tag, word, *got), = _run("min", *(f"{a},{i},{p}" for a, i, p in s))
        assert tag == "M" and tuple(int(x) for x in got) == min(s), s
    (tag, word, *got), = _run("min")                            # no violation: the word stays kOrdered
    assert int(word) == ORDERED and [int(x) for x in got] == [-1, 0, 0]


def test_fill_status():
    _, _, status = _dump()
    assert status.pop(ORDERED) == _lib.CDA_OK
    assert status and set(status.values()) == {_lib.CDA_ERR_PUSH_ORDER}
