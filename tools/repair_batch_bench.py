#!/usr/bin/env python3
"""Repair of a batch of HBM-resident squares in one call against one call per
square, on one GPU.  A measurement, not a gate: no ratio was fixed in advance.

Cases: k = 128 with Q0 lost and with half of the cells lost at random, n = 1, 8
and 64 squares; k = 32 with the same two patterns, n = 256.  The squares are
DISTINCT random squares extended by the library (their DAHs differ), repeated
to fill the batch; every square of a batch has its own random mask.
  batch: one cda_repair_batch_device call for the n squares;
  loop:  n cda_repair_device calls in the same process on the same squares --
         the single-square path, which the batch call leaves as it was;
  plan:  cda_repair_batch_plan alone on the same maps (host only): the part of
         the batch call that runs before its first launch.
The squares stay in HBM between calls: the presence maps say which cells are
lost, and a repair ignores and overwrites those, so every call does the same
work.  The timed region is the C call(s) alone, the planning on the host, the
uploads of maps and roots, and the synchronisations included.  Wall time,
WARMUP calls first, then REPS timed calls; median, min and max.  Every status
is checked, and after the first call of each kind the squares are compared
with the originals.

Writes profiles/repair_batch.txt (or argv[1]).
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("celestia-app_amd",):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402

from celestia_da import _lib, default_context, testfactory  # noqa: E402

DISTINCT = 8
WARMUP = int(os.environ.get("WARMUP", "2"))
REPS = int(os.environ.get("REPS", "10"))
ptr = _lib.ptr
I32P, U32P = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def timed(call, warmup=WARMUP, reps=REPS):
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return times


def squares(ctx, k):
    """DISTINCT extended squares of ODS width k with their roots."""
    W = 2 * k
    ods = np.stack([np.ascontiguousarray(testfactory.random_square(k, s), dtype=np.uint8).reshape(-1, 512)
                    for s in range(DISTINCT)])
    eds = np.empty((DISTINCT, W, W, 512), dtype=np.uint8)
    rows = np.empty((DISTINCT, W, 90), dtype=np.uint8)
    cols = np.empty((DISTINCT, W, 90), dtype=np.uint8)
    roots = np.empty((DISTINCT, 32), dtype=np.uint8)
    status = np.empty(DISTINCT, dtype=np.int32)
    ctx.check(ctx.lib.cda_extend_dah_batch(ctx.h, ptr(ods), k, DISTINCT, ptr(eds), ptr(rows), ptr(cols), ptr(roots),
                                           status.ctypes.data_as(I32P)))
    assert not status.any()
    return eds, rows, cols


def masks(k, n, pattern):
    W = 2 * k
    if pattern == "Q0 lost":
        p = np.ones((n, W, W), dtype=np.uint8)
        p[:, :k, :k] = 0
        return p
    rng = np.random.default_rng(1000 + k)
    return (rng.random((n, W, W)) < 0.5).astype(np.uint8)


def line(t, n):
    m = statistics.median(t)
    return (f"ms per call: median {m * 1e3:9.3f}  min {min(t) * 1e3:9.3f}  max {max(t) * 1e3:9.3f}"
            f"  ({m / n * 1e3:7.3f} ms per square)")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "repair_batch.txt")
    import torch
    ctx = default_context()
    lines = [f"batch repair of HBM-resident squares against one cda_repair_device call per square; "
             f"{ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s); warm-up {WARMUP}, {REPS} timed calls; {DISTINCT} distinct "
             "squares repeated to fill a batch, one mask per square", ""]
    for k, sizes in ((128, (1, 8, 64)), (32, (256,))):
        W = 2 * k
        eds, rows, cols = squares(ctx, k)
        for pattern in ("Q0 lost", "half of the cells lost at random"):
            for n in sizes:
                pick = np.arange(n) % DISTINCT
                present = masks(k, n, pattern)
                want = eds[pick]
                rr, cr = np.ascontiguousarray(rows[pick]), np.ascontiguousarray(cols[pick])
                d = torch.from_numpy(np.where(present[..., None] != 0, want, 0).astype(np.uint8).reshape(-1)).to("cuda")
                torch.cuda.synchronize()
                status = np.full(n, 77, dtype=np.int32)
                axis = np.zeros(n, dtype=np.int32)
                index = np.zeros(n, dtype=np.uint32)
                sq_b = W * W * 512

                def batch():
                    ctx.check(ctx.lib.cda_repair_batch_device(ctx.h, d.data_ptr(), ptr(present), W, n, ptr(rr), ptr(cr),
                                                              status.ctypes.data_as(I32P), axis.ctypes.data_as(I32P),
                                                              index.ctypes.data_as(U32P)))
                    assert not status.any(), status

                def loop():
                    a, x = C.c_int32(-1), C.c_uint32(0)
                    for i in range(n):
                        ctx.check(ctx.lib.cda_repair_device(ctx.h, d.data_ptr() + i * sq_b, ptr(present[i]), W,
                                                            ptr(rr[i]), ptr(cr[i]), C.byref(a), C.byref(x)))
                seg_off = np.zeros(4 * W + 1, dtype=np.uint32)
                seg_sweep = np.zeros(4 * W, dtype=np.uint32)
                entries = np.zeros(n * 2 * W * 3, dtype=np.uint32)
                solved = np.zeros(n, dtype=np.uint8)
                n_seg = C.c_uint32(0)

                def plan():
                    rc = ctx.lib.cda_repair_batch_plan(ptr(present), W, n, C.byref(n_seg), seg_off.ctypes.data_as(U32P),
                                                       seg_sweep.ctypes.data_as(U32P), entries.ctypes.data_as(U32P),
                                                       ptr(solved))
                    assert rc == 0
                t_p = timed(plan)
                assert solved.all()
                batch()
                assert np.array_equal(d.cpu().numpy().reshape(want.shape), want), "the batch call must repair the squares"
                t_b = timed(batch)
                d.copy_(torch.from_numpy(np.where(present[..., None] != 0, want, 0).astype(np.uint8).reshape(-1)))
                torch.cuda.synchronize()
                loop()
                assert np.array_equal(d.cpu().numpy().reshape(want.shape), want), "the loop must repair the squares"
                t_l = timed(loop)
                mb, ml = statistics.median(t_b), statistics.median(t_l)
                lines += [f"k = {k}, {pattern}, n = {n}",
                          "  batch: " + line(t_b, n), "  loop:  " + line(t_l, n), "  plan:  " + line(t_p, n),
                          f"  loop / batch = {ml / mb:.2f}   segments {n_seg.value}, entries {int(seg_off[n_seg.value])}",
                          ""]
                print("\n".join(lines[-6:]), flush=True)
                del d
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
