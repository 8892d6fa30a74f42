#!/usr/bin/env python3
"""Serving and checking data-availability samples from one k = 128 resident
square on one GPU.  A measurement, not a gate: the only requirement is that a
sample of (a) costs less than a sample of (b) in the same run.

4 096 samples per call:
  (a) cells of Q0 on the row axis, one cda_square_sample_proofs call;
  (b) the same 4 096 cells through 4 096 cda_square_share_proof calls (one
      single-share proof each): the only way to answer them without (a);
  (c) uniformly random cells of the whole EDS with random axes, one call;
  (d) cda_sample_proofs_verify of (c).
The timed region is the C call alone (for (b): the loop of C calls, buffers
allocated once, no Python objects built): host buffers in and out, the copies
and the stream synchronisation inside it.  Wall time, WARMUP calls first, then
REPS timed calls; median, min and max are reported.  Bytes returned: the six
output arrays of (a) / (c); for (b) the share, the proof nodes, the row root,
the leaf hash and the aunts; for (d) the bytes checked.

These are whole-call figures.  The kernels' own times come from a kernel
trace of this tool in a run of its own (rocprofv3 --kernel-trace --stats --
python3 tools/sample_proofs_bench.py OUT with WARMUP=2 REPS=5; the stats CSV
is profiles/sample_proofs_kernel_stats.csv).

Writes profiles/sample_proofs.txt (or argv[1]).
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

import numpy as np  # noqa: E402

from celestia_da import _lib, default_context, sampling, testfactory  # noqa: E402
from celestia_da import proof as gpr  # noqa: E402

K = 128
N = 4096
WARMUP = int(os.environ.get("WARMUP", "5"))
REPS = int(os.environ.get("REPS", "30"))
ptr = _lib.ptr


def timed(call):
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= WARMUP:
            times.append(dt)
    return times


def serve(ctx, sq, coords):
    rows, cols, axes = sampling.split_coords(coords)
    out = sampling.SampleBatch.empty(K, coords)
    u32p = C.POINTER(C.c_uint32)
    args = (sq.h, rows.ctypes.data_as(u32p), cols.ctypes.data_as(u32p), ptr(axes), rows.size,
            *(ptr(a) for a in out.arrays()))

    def call():
        ctx.check(ctx.lib.cda_square_sample_proofs(*args))
    return timed(call), out, sum(a.nbytes for a in out.arrays())


def serve_one_by_one(ctx, sq, coords):
    """One cda_square_share_proof call per cell (Q0, row axis)."""
    D, A = 8, 9
    share = np.empty(512, dtype=np.uint8)
    nodes = np.empty(2 * D * 90, dtype=np.uint8)
    root, leaf, aunts = np.empty(90, dtype=np.uint8), np.empty(32, dtype=np.uint8), np.empty(A * 32, dtype=np.uint8)
    ns, ne, cnt = (C.c_int32 * 1)(), (C.c_int32 * 1)(), (C.c_uint32 * 1)()
    r0, r1 = C.c_uint32(), C.c_uint32()
    starts = [int(r) * K + int(c) for r, c, _ in coords]
    fn, h = ctx.lib.cda_square_share_proof, sq.h
    tail = (ptr(share), C.byref(r0), C.byref(r1), ns, ne, cnt, ptr(nodes), ptr(root), ptr(leaf), ptr(aunts))
    n_nodes = 0

    def call():
        nonlocal n_nodes
        n_nodes = 0
        for s in starts:
            rc = fn(h, s, s + 1, *tail)
            if rc:
                ctx.check(rc)
            n_nodes += cnt[0]
    t = timed(call)
    return t, len(starts) * (512 + 90 + 32 + A * 32) + n_nodes * 90


def verify(ctx, batch, root):
    rows, cols, axes = sampling.split_coords(batch.coords)
    roots = np.tile(np.frombuffer(root, dtype=np.uint8), len(batch))
    verdict = np.full(len(batch), 255, dtype=np.uint8)
    u32p = C.POINTER(C.c_uint32)
    arrs = (batch.shares, batch.nmt_nodes, batch.axis_roots, batch.leaf_hash, batch.aunts)
    args = (ctx.h, K, len(batch), ptr(roots), rows.ctypes.data_as(u32p), cols.ctypes.data_as(u32p), ptr(axes),
            *(ptr(a) for a in arrs), ptr(verdict))

    def call():
        ctx.check(ctx.lib.cda_sample_proofs_verify(*args))
    t = timed(call)
    assert not verdict.any(), "a sample of the bench failed to verify"
    return t, sum(a.nbytes for a in arrs) + roots.nbytes


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sample_proofs.txt")
    ctx = default_context()
    sq = gpr.ResidentSquare(testfactory.random_square(K, 0), ctx)
    root = sq.dah()[2]
    step = K * K // N
    q0 = np.array([(s // K, s % K, 0) for s in range(0, K * K, step)], dtype=np.int64)
    rng = np.random.default_rng(0)
    anywhere = np.stack([rng.integers(0, 2 * K, N), rng.integers(0, 2 * K, N), rng.integers(0, 2, N)], axis=1)

    t_a, batch_a, bytes_a = serve(ctx, sq, q0)
    t_b, bytes_b = serve_one_by_one(ctx, sq, q0)
    t_c, batch_c, bytes_c = serve(ctx, sq, anywhere)
    assert not sampling.verify_samples(batch_a, root, ctx).any()
    t_d, bytes_d = verify(ctx, batch_c, root)
    sq.close()

    lines = [f"data-availability samples of one k = {K} resident square, {N} samples per call; "
             f"{ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s) (host buffers in and out); warm-up {WARMUP}, {REPS} timed calls",
             ""]
    med = {}
    for key, name, t, nbytes in (
            ("a", "a: Q0 cells, row axis, one cda_square_sample_proofs call", t_a, bytes_a),
            ("b", f"b: the same cells, {N} cda_square_share_proof calls", t_b, bytes_b),
            ("c", "c: random cells of the whole EDS, random axes, one cda_square_sample_proofs call", t_c, bytes_c),
            ("d", "d: cda_sample_proofs_verify of (c), one call", t_d, bytes_d)):
        m = med[key] = statistics.median(t)
        lines += [name,
                  f"  ms per {N} samples: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}",
                  f"  per sample {m / N * 1e6:.3f} us  samples/s {N / m:,.0f}  "
                  f"bytes {nbytes} ({nbytes / N:.0f} per sample)  {nbytes / m / 1e9:.3f} GB/s",
                  ""]
    lines += [f"per-sample time of (a) / (b): {med['a'] / N * 1e6:.3f} us / {med['b'] / N * 1e6:.3f} us = "
              f"1 / {med['b'] / med['a']:.1f}", ""]
    assert med["a"] < med["b"], "the batched call must cost less per sample than one call per proof"
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
