"""tools/hash_plan_host_test.cpp (csrc/hash_plan.h printed by a host program)
built once per test session, and its output parsed into part plans and plan
classes.  Shared by test_hash_schedules.py, test_tree_top_schedule.py and
test_variants.py."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celestia-app_amd", "csrc")

HAVE_GXX = shutil.which("g++") is not None

Launch = namedtuple("Launch", "kernel n_in sub wide lv n_dig pair ragged pmax mode threads persistent scratch")
Part = namedtuple("Part", "k n parts p i0 m stop room launches")

# The A/B forms the test build still carries (tests/test_variants.py runs one
# child per entry; test_hash_schedules.py asserts on the CPU that each reaches
# a plan the default schedule does not).  CDA_HASH_WG_PER_CU=1: 256 persistent
# workgroups, fewer than the blocks of every k >= 32 case of VARIANT_CASES.
VARIANT_ENVS = [
    {"CDA_TOP_PAIR": "0"},
    {"CDA_DR_HELPERS": "0"},
    {"CDA_TOP_HELPERS": "0"},
    {"CDA_TOP_RFC": "0"},
    {"CDA_TOP_WIDE": "0"},
    {"CDA_SUBTREE": "0"},
    {"CDA_LEAF_PAIR_MAX": "0"},
    {"CDA_HASH_WG_PER_CU": "1"},
    {"CDA_TOP_FUSE": "0"},
    {"CDA_RS8_ONE": "1"},
    {"CDA_RS8_BYTEFORM": "1"},
]
VARIANT_CASES = [(8, 1), (32, 3), (64, 9), (128, 2), (128, 16), (256, 1)]


@functools.lru_cache(maxsize=None)
def _exe() -> str:
    d = tempfile.mkdtemp(prefix="hash_plan_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "hash_plan_host_test")
    subprocess.run(["g++", "-O2", "-std=c++20", "-Wall", "-I", CSRC,
                    os.path.join(ROOT, "tools", "hash_plan_host_test.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def _run(args) -> str:
    r = subprocess.run([_exe(), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@functools.lru_cache(maxsize=None)
def plans(knobs: tuple = ()) -> dict:
    """{(k, n): [Part, ...]} for every (k, n) the tool prints, under the
    knob settings `knobs` (a tuple of "NAME=VALUE")."""
    out = {}
    for line in _run(knobs).splitlines():
        head, tail = line.split(":")
        tag, *f = head.split()
        assert tag == "P", line
        k, n, parts, p, i0, m, stop, room = (int(x) for x in f)
        launches = []
        for tok in tail.split():
            name, *v = tok.split(",")
            launches.append(Launch(name, *(int(x) for x in v)))
        out.setdefault((k, n), []).append(Part(k, n, parts, p, i0, m, stop, room, tuple(launches)))
    return out


def env_knobs(env: dict) -> tuple:
    return tuple(f"{name}={value}" for name, value in sorted(env.items()))


def class_key(part: Part) -> tuple:
    """A plan class: k and the ordered launches with the parameters that pick
    a kernel form -- not n, and not the figures that only restate them
    (threads, scratch bytes)."""
    return (part.k,) + tuple((l.kernel, l.n_in, l.sub, l.wide, l.lv, l.n_dig, l.pair, l.ragged, l.pmax, l.mode,
                              l.persistent) for l in part.launches)


def describe(key: tuple) -> str:
    def one(l):
        kernel, n_in, sub, wide, lv, n_dig, pair, ragged, pmax, mode, persistent = l
        if kernel == "rs8":
            return f"rs8[{n_in} cw, {'bitsliced' if sub else 'byte form'}{', one per wg' if pair else ''}]"
        if kernel in ("leaf", "leaf_pair"):
            return kernel + ("[persistent]" if persistent else "")
        if kernel == "subtree":
            return f"subtree[{n_in}->{sub}]"
        if kernel == "level":
            return f"level[{n_in}]" + ("[persistent]" if persistent else "")
        if kernel == "tree_top":
            return (f"tree_top[n_in={n_in}{' wide' if wide else ''} tpw={sub} lv={lv} n_dig={n_dig} "
                    f"{'pair' if pair else 'no-pair'}{' helpers' if mode else ''}{' ragged' if ragged else ''}]")
        if kernel == "data_root":
            return f"data_root[n_dig={n_dig} pmax={pmax} mode={mode}]"
        return kernel
    return f"k={key[0]}: " + " ".join(one(l) for l in key[1:])


def top_fuse_table(knobs: tuple = ()) -> dict:
    """{(W, n, top_wide): (top, wide)} from hash_plan.h top_fuse_nodes."""
    out = {}
    for line in _run(("--top",) + tuple(knobs)).splitlines():
        tag, W, n, tw, top, wide = line.split()
        assert tag == "T", line
        out[(int(W), int(n), int(tw))] = (int(top), bool(int(wide)))
    return out
