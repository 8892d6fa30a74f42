#!/usr/bin/env python3
"""Axis halves of a resident square on one GPU: serving, verifying, and the
route to a right half's data that exists without the recovery kernels.  A
measurement, not a gate: no threshold is set.

For k = 128 and k = 512, one resident square:
  (a) serving one half of every row (2k halves, sides alternating):
      one cda_square_axis_halves call;
  (b) cda_axis_halves_verify of the halves of rows 0 .. 255:
        256 left halves; 256 right halves; the 512 mixed in one call
        (with and without the completed vectors returned);
  (c) the same 256 right halves through the calls that exist without the
      recovery kernels: cda_rs_decode of the 256 codewords with the data half
      erased, then cda_nmt_axis_roots of the rebuilt vectors (the roots are
      compared with the DAH's on the host, outside the clock).
Every route ends synchronised and its answer is checked once against the
square.  Wall time around the C calls, buffers allocated before; WARMUP calls
first, then REPS timed ones; median, min and max.

The kernels' own times come from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/axis_halves_bench.py --trace
verifies the 256 left and the 256 right halves TRACE_CALLS times each, and
    python tools/axis_halves_bench.py --summarise DIR profiles/axis_halves.txt
appends the median duration of every Reed-Solomon kernel of those calls: the
forward instantiation that completes the left halves next to the recovery
instantiation that completes the right ones, 256 codewords each.

Writes profiles/axis_halves.txt (or argv[1]).
"""
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

import numpy as np  # noqa: E402

WARMUP = int(os.environ.get("WARMUP", "2"))
REPS = int(os.environ.get("REPS", "10"))
TRACE_CALLS = 5
KS = (128, 512)
N = 256
U32P = C.POINTER(C.c_uint32)
I32P = C.POINTER(C.c_int32)


def timed(call):
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= WARMUP:
            times.append(dt)
    return times


def line(name, t, count, unit):
    m = statistics.median(t)
    return (f"  {name}\n    ms: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"
            f"   per {unit} {m / count * 1e6:.2f} us")


class Case:
    """One resident square of width k, its DAH, and the halves of rows 0 .. 255."""

    def __init__(self, ctx, k):
        from celestia_da import axis_halves as ah
        from celestia_da import proof, testfactory
        self.ctx, self.k, self.W = ctx, k, 2 * k
        self.sq = proof.ResidentSquare(testfactory.random_square(k, 7), ctx)
        rows, cols, _ = self.sq.dah()
        self.rows = np.frombuffer(b"".join(bytes(r) for r in rows), dtype=np.uint8).reshape(self.W, 90)
        self.cols = np.frombuffer(b"".join(bytes(c) for c in cols), dtype=np.uint8).reshape(self.W, 90)
        self.left = self.sq.axis_halves([(0, r, 0) for r in range(N)])
        self.right = self.sq.axis_halves([(0, r, 1) for r in range(N)])
        self.mixed = ah.HalfBatch(k, np.concatenate([self.left.coords, self.right.coords]),
                                  np.concatenate([self.left.shares, self.right.shares]))
        self.vectors = np.concatenate([self.left.shares, self.right.shares], axis=1)   # (N, 2k, 512)

    def verify(self, batch, vectors):
        from celestia_da import axis_halves as ah
        return ah.verify_axis_halves(batch, (self.rows, self.cols), self.ctx, vectors=vectors)

    def close(self):
        self.sq.close()


def report(out_path):
    from celestia_da import _lib, default_context
    ctx = default_context()
    ptr = _lib.ptr
    lines = [f"axis halves of one resident square, {N} halves per side; WARMUP {WARMUP}, REPS {REPS}", ""]
    for k in KS:
        c = Case(ctx, k)
        W = c.W
        lines.append(f"k = {k}")
        # (a) one half of every row
        every = np.array([(0, r, r & 1) for r in range(W)], dtype=np.int64)
        assert np.array_equal(c.sq.axis_halves(every).shares[:N:2], c.left.shares[:N:2])
        lines.append(line(f"(a) serve one half of every row ({W} halves, {W * k * 512 >> 20} MiB)",
                          timed(lambda: c.sq.axis_halves(every)), W, "half"))
        # (b) verify
        for name, batch, want in (("256 left halves", c.left, c.vectors), ("256 right halves", c.right, c.vectors),
                                  ("512 mixed", c.mixed, np.concatenate([c.vectors, c.vectors]))):
            v, vec = c.verify(batch, True)
            assert not v.any() and np.array_equal(vec, want), name
            lines.append(line(f"(b) verify {name}, vectors returned", timed(lambda: c.verify(batch, True)),
                              len(batch), "half"))
            lines.append(line(f"(b) verify {name}, verdicts only", timed(lambda: c.verify(batch, False)),
                              len(batch), "half"))
        # (c) the right halves through the general decoder and the standalone trees
        shards = np.zeros((N, W, 512), dtype=np.uint8)
        present = np.zeros((N, W), dtype=np.uint8)
        present[:, k:] = 1
        axis = np.arange(N, dtype=np.uint32)
        roots = np.zeros((N, 90), dtype=np.uint8)
        status = np.zeros(N, dtype=np.int32)

        def old_route():
            shards[:, :k] = 0
            shards[:, k:] = c.right.shares
            ctx.check(ctx.lib.cda_rs_decode(ctx.h, ptr(shards), ptr(present), k, 512, N))
            ctx.check(ctx.lib.cda_nmt_axis_roots(ctx.h, ptr(shards), 512, W, N, k, axis.ctypes.data_as(U32P),
                                                 ptr(roots), status.ctypes.data_as(I32P)))

        old_route()
        assert np.array_equal(shards, c.vectors) and np.array_equal(roots, c.rows[:N]) and not status.any()
        lines.append(line("(c) 256 right halves: cda_rs_decode, then cda_nmt_axis_roots",
                          timed(old_route), N, "half"))
        lines.append("")
        c.close()
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


def trace():
    from celestia_da import default_context
    ctx = default_context()
    for k in KS:
        c = Case(ctx, k)
        for batch in (c.left, c.right):
            for _ in range(TRACE_CALLS):
                assert not c.verify(batch, False).any()
        c.close()


def summarise(trace_dir, out_path):
    """The Reed-Solomon kernels of the trace's verify calls: per kernel and grid, the last TRACE_CALLS
    dispatches (the square's own extension, which comes first, runs a kernel at most once per grid)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    groups = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "rs8" in name or "rs16" in name:
                key = (name.replace("void ", "").replace("cda::(anonymous namespace)::", "").split("(")[0],
                       int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_X"])))
                groups.setdefault(key, []).append((int(r["Start_Timestamp"]),
                                                   (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    lines = ["", f"Reed-Solomon kernels of {TRACE_CALLS} verify calls of {N} left and of {N} right halves per k "
                 "(rocprofv3 --kernel-trace, a run of its own; median us)"]
    for (name, wgs), runs in sorted(groups.items()):
        if len(runs) >= TRACE_CALLS:
            t = [d for _, d in sorted(runs)[-TRACE_CALLS:]]
            lines.append(f"  {name}: {wgs} workgroups, {statistics.median(t):.1f} us  (min {min(t):.1f}, max {max(t):.1f})")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace()
    elif len(sys.argv) > 1 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3])
    else:
        report(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "axis_halves.txt"))
