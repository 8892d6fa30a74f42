"""bench.py's plain run and --dump-outputs.

CPU: dump_outputs on host tensors (names, number formats, the fixed sample,
exact byte values), and the argument checks.  GPU: one small plain run
(4 squares, 2 steps) whose line carries the headline fields and none of the
--full ones, and whose dumped arrays equal the oracle's for the same squares.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = {"data_roots", "status", "row_roots", "col_roots", "eds_shares", "roots_index", "eds_shares_index"}
FULL_ONLY = ("parity", "stage_pass", "roofline", "rs_roofline", "traffic", "stages", "cpu_baseline", "extras")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def _load(d):
    return {os.path.splitext(f)[0]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_on_host_tensors(tmp_path):
    import torch
    k, batch = 2, 3
    W = 2 * k
    g = torch.Generator().manual_seed(1)
    eds = torch.randint(0, 256, (batch * W * W * 512,), dtype=torch.uint8, generator=g)
    rows = torch.randint(0, 256, (batch * W * 90,), dtype=torch.uint8, generator=g)
    cols = torch.randint(0, 256, (batch * W * 90,), dtype=torch.uint8, generator=g)
    roots = torch.randint(0, 256, (batch * 32,), dtype=torch.uint8, generator=g)
    status = torch.tensor([0, -3, 2 ** 31 - 1], dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "a"), k, batch, eds, rows, cols, roots, status)
    bench.dump_outputs(str(tmp_path / "b"), k, batch, eds, rows, cols, roots, status)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES == set(b)
    for name in NAMES:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name          # the sample is fixed
    assert np.array_equal(a["data_roots"], roots.view(batch, 32).numpy())
    assert np.array_equal(a["status"], status.numpy().astype(np.float64))   # exact, int32 extremes included
    assert list(a["roots_index"]) == [0, 1, 2]                 # batch <= sample size: every square
    assert np.array_equal(a["row_roots"], rows.view(batch, W, 90).numpy())
    assert np.array_equal(a["col_roots"], cols.view(batch, W, 90).numpy())
    idx = a["eds_shares_index"].astype(np.int64)
    assert idx.shape == (bench.DUMP_EDS_SHARES, 3) and a["eds_shares"].shape == (bench.DUMP_EDS_SHARES, 512)
    assert (idx >= 0).all() and (idx[:, 0] < batch).all() and (idx[:, 1:] < W).all()
    e = eds.view(batch, W, W, 512).numpy()
    assert np.array_equal(a["eds_shares"], e[idx[:, 0], idx[:, 1], idx[:, 2]])


def test_dump_sample_within_budget_at_config4_shape():
    """The files of a default run (1 024 squares, k = 128) stay far below 64 MB."""
    W = 256
    n = (1024 * 32 * 4 + 1024 * 8 + 2 * bench.DUMP_ROOT_SQUARES * W * 90 * 4 + bench.DUMP_EDS_SHARES * 512 * 4
         + bench.DUMP_ROOT_SQUARES * 8 + bench.DUMP_EDS_SHARES * 3 * 8)
    assert n < 32e6


@pytest.mark.parametrize("argv,msg", [(["--steps", "0"], "--steps"), (["--config5"], "--full")])
def test_argument_checks(argv, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=_env(), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr and r.stdout == ""


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    import coracle
    k, batch, steps = 128, 4, 2
    W = 2 * k
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(batch), "--dump-outputs", str(out)], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["metric"] == "EDS+DAH squares/sec (k=128)" and j["unit"] == "squares/s" and j["dtype"] == "u8/u32"
    assert j["higher_is_better"] is True and j["steps"] == steps and j["full"] is False
    assert j["ms_per_step"] > 0
    assert abs(j["value"] - batch / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    for name in FULL_ONLY:
        assert name not in j, name
    d = _load(out)
    assert set(d) == NAMES
    assert not d["status"].any()
    with open(os.path.join(ROOT, "tests", "golden", "config4_k128.json")) as f:
        g = json.load(f)["squares"]
    for i in range(batch):
        assert d["data_roots"][i].astype(np.uint8).tobytes().hex() == g[str(i)]["data_root"], i
    assert list(d["roots_index"]) == list(range(batch))
    eds, rows, cols, _ = coracle.cpu_baseline(coracle.random_square(k, 1), 8)
    assert np.array_equal(d["row_roots"][1], rows) and np.array_equal(d["col_roots"][1], cols)
    idx = d["eds_shares_index"].astype(np.int64)
    sel = idx[:, 0] == 1
    assert sel.sum() > 100
    assert np.array_equal(d["eds_shares"][sel], eds.reshape(W, W, 512)[idx[sel, 1], idx[sel, 2]])
