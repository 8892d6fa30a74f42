"""The A/B-selectable encoder variants stay bit-exact.

The library picks one kernel per job shape and reads its A/B knobs once per
process, so the non-default forms are only reachable from a fresh process:
  * (round 3's CDA_RS16_HALF=0 full-width GF(2^16) kernel was removed in round 4
    with the byte-form encoders it belonged to; the bitsliced encoder has no
    variants)
  * CDA_RS8_SLICE=0 -- the k = 128 Q0 launch of a batch without the XCD-aware
    128-byte slices (mode 0, two codewords per workgroup);
  * CDA_RS8_BS=1 -- round 1's four-codeword k = 128 encoder.
Each child extends squares of the committed fixtures and compares data roots
and EDS / root digests (tests/golden/k512.json, config4_k128.json; generated
by oracle/gen_config4.py from the C oracle).  Reference: the Leopard encoders
behind pkg/appconsts/global_consts.go:92 (klauspost/reedsolomon v1.12.1)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hash_plan_tool
import knobs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_CHILD = r"""
import hashlib, json, os, sys
sys.path[:0] = [os.path.join(ROOT, "celestia-app_amd"), ROOT]
import numpy as np
import torch
from celestia_da import Context, testfactory
ctx = Context(0)
dev = torch.device("cuda", 0)
square = testfactory.random_square
if sys.argv[1] == "edges":   # P-left and the ladder square in turn (tests/nmt_edge_squares.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nmt_edge_squares
    square = lambda k, i: nmt_edge_squares.square(("p_left", "ladder")[i % 2], k).reshape(k * k, 512)
sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
for k, n in zip(map(int, sys.argv[2::2]), map(int, sys.argv[3::2])):
    W = 2 * k
    eds = torch.zeros(n, W * W * 512, dtype=torch.uint8, device=dev)
    for i in range(n):
        eds[i].view(W, W, 512)[:k, :k] = torch.from_numpy(square(k, i)).to(dev).view(k, k, 512)
    rows = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    cols = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    roots = torch.empty(n, 32, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.extend_dah_inplace_device(k, n, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                  status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = [{"status": int(status[i]), "data_root": roots[i].cpu().numpy().tobytes().hex(),
            "eds_sha256": sha(eds[i]), "row_roots_sha256": sha(rows[i]), "col_roots_sha256": sha(cols[i])}
           for i in range(n)]
    print(json.dumps(out))
    del eds
""".replace("ROOT", repr(ROOT))


def _run_cases(env_extra: dict, cases: list, squares: str = "x") -> list:
    """One fresh process on the test build with `env_extra` set: the squares
    0 .. n-1 of every (k, n) of `cases`, one in-place batch each.  squares =
    "edges": the edge-namespace squares of test_namespace_edges.py in place
    of the random ones."""
    env = dict(os.environ)
    env.update(env_extra)
    env["CDA_LIB"] = knobs.lib_path_for_tests()   # the A/B knobs are read only by the test build
    args = [str(x) for kn in cases for x in kn]
    r = subprocess.run([sys.executable, "-c", _CHILD, squares, *args], env=env, capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.strip().splitlines()[-len(cases):]]


def _run(env_extra: dict, k: int, n: int) -> list:
    return _run_cases(env_extra, [(k, n)])[0]


@pytest.mark.parametrize("env", [{"CDA_RS8_SLICE": "0"}, {"CDA_RS8_SLICE": "1"}, {"CDA_RS8_BS": "1"}],
                         ids=["mode0", "slices", "round1_kernel"])
def test_gf8_q0_modes_match_fixture(env):
    """16 squares in one submission (the batch path: slice mode 2 unless
    CDA_RS8_SLICE=0; CDA_RS8_BS=1 is round 1's four-codeword kernel) against
    config 4's fixture (squares 0..15)."""
    g = json.load(open(os.path.join(HERE, "golden", "config4_k128.json")))["squares"]
    got = _run(env, 128, 16)
    for i in range(16):
        want = g[str(i)]
        assert got[i]["status"] == 0
        assert got[i]["data_root"] == want["data_root"], i
        assert got[i]["row_roots_sha256"] == want["row_roots_sha256"], i
        assert got[i]["col_roots_sha256"] == want["col_roots_sha256"], i
        if "eds_sha256" in want:
            assert got[i]["eds_sha256"] == want["eds_sha256"], i


@functools.lru_cache(maxsize=None)
def _oracle_digests(k: int, n: int) -> list:
    """Squares 0 .. n-1 of width k as the children see them: the committed
    oracle digests at k = 128, the C oracle otherwise."""
    import coracle
    from celestia_da import testfactory
    if k == 128:
        g = json.load(open(os.path.join(HERE, "golden", "config4_k128.json")))["squares"]
        return [g[str(i)] for i in range(n)]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    out = []
    for i in range(n):
        ods = testfactory.random_square(k, i)
        eds, rows, cols, root = coracle.cpu_baseline(ods, 16) if k >= 64 else coracle.extend_dah(ods)
        out.append({"data_root": root.hex(), "eds_sha256": sha(eds), "row_roots_sha256": sha(rows),
                    "col_roots_sha256": sha(cols)})
    return out


@pytest.mark.parametrize("env", hash_plan_tool.VARIANT_ENVS,
                         ids=lambda e: "-".join(f"{a}={b}" for a, b in e.items()))
def test_ab_form_matches_oracle(env):
    """The A/B forms the test build still carries -- thread-per-parent tree
    tops and data root (CDA_TOP_PAIR=0), no schedule helpers, no RFC levels in
    the top, no wide first level, per-level launches only, one-lane leaves,
    the persistent leaf / level grids (CDA_HASH_WG_PER_CU=1), no tree top, and
    the k = 128 encoder's one-codeword and byte-form launches -- one child
    each over hash_plan_tool.VARIANT_CASES: every square's EDS digest, row and
    column root digests and data root against the oracle
    (test_hash_schedules.py asserts that each child reaches a plan the default
    schedule does not)."""
    got = _run_cases(env, hash_plan_tool.VARIANT_CASES)
    for (k, n), squares in zip(hash_plan_tool.VARIANT_CASES, got):
        want = _oracle_digests(k, n)
        assert len(squares) == n
        for i in range(n):
            assert squares[i]["status"] == 0, (env, k, n, i)
            for field in ("data_root", "row_roots_sha256", "col_roots_sha256", "eds_sha256"):
                assert squares[i][field] == want[i][field], (env, k, n, i, field)
