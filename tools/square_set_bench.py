#!/usr/bin/env python3
"""Building resident squares from a device batch, and serving samples across a
set of them, on one GPU.  A measurement, not a gate: no threshold is set.

For k = 128 and k = 32:
  (a) 64 resident squares from a batch that lies in HBM (what
      cda_extend_dah_device, replay or cda_repair_batch_device leave there):
        a1  one cda_square_set_create_device call, CDA_SET_FROM_EDS;
        a2  one cda_square_set_create_device call, CDA_SET_FROM_ODS;
        a0  the only route without sets: one D2H of the 64 original squares,
            then 64 cda_square_create calls (each copies its ODS up and extends
            it again).
      The timed region is the create call(s) plus, for a0, the D2H; every call
      returns with its squares complete.  Allocation of the resident buffers is
      inside the region on both sides; destroying them is outside it.
  (b) 16 samples of each of 256 squares (4 096 samples, random cells and axes,
      squares interleaved):
        b1  one cda_square_set_sample_proofs call;
        b0  256 cda_square_sample_proofs calls on the same members, 16 samples
            each, into the same output arrays.
      The outputs of b1 and b0 are compared byte for byte.
Wall time around calls that end synchronised; WARMUP calls first, then REPS
timed ones; median, min and max are reported.

Writes profiles/square_set.txt (or argv[1]).
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

import numpy as np  # noqa: E402

from celestia_da import _lib, default_context, testfactory  # noqa: E402

WARMUP = int(os.environ.get("WARMUP", "2"))
REPS = int(os.environ.get("REPS", "10"))
SAMPLE_REPS = int(os.environ.get("SAMPLE_REPS", "30"))
N_BUILD, N_SERVE, PER_SQUARE = 64, 256, 16
ptr = _lib.ptr
U32P = C.POINTER(C.c_uint32)


def timed(call, reps, after=None):
    times = []
    for i in range(WARMUP + reps):
        t0 = time.perf_counter()
        r = call()
        dt = time.perf_counter() - t0
        if after:
            after(r)
        if i >= WARMUP:
            times.append(dt)
    return times


def device_batches(ctx, k, n):
    """(d_ods, d_eds, host ODS of the four distinct squares): n squares in HBM, four distinct ones repeated."""
    import torch
    distinct = np.stack([testfactory.random_square(k, 10 + i).reshape(k * k, 512) for i in range(4)])
    d_ods = torch.from_numpy(distinct).cuda()[torch.arange(n, device="cuda") % 4].contiguous()
    W = 2 * k
    d_eds = torch.empty((n, W * W * 512), dtype=torch.uint8, device="cuda")
    rows = torch.empty((n, W * 90), dtype=torch.uint8, device="cuda")
    cols = torch.empty((n, W * 90), dtype=torch.uint8, device="cuda")
    roots = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    ctx.extend_dah_device(d_ods.data_ptr(), k, n, d_eds.data_ptr(), rows.data_ptr(), cols.data_ptr(),
                          roots.data_ptr(), None, None)
    torch.cuda.synchronize()
    return d_ods, d_eds, roots.cpu().numpy()


def build_set(ctx, d, kind, k, n):
    def call():
        h = C.c_void_p()
        ctx.check(ctx.lib.cda_square_set_create_device(ctx.h, d.data_ptr(), kind, k, n, None, C.byref(h)))
        return h
    return call


def build_singles(ctx, d_ods, k, n):
    def call():
        ods = d_ods.cpu().numpy()      # one D2H of every original square
        hs = []
        for i in range(n):
            h = C.c_void_p()
            ctx.check(ctx.lib.cda_square_create(ctx.h, ptr(ods[i]), k * k, C.byref(h)))
            hs.append(h)
        return hs
    return call


def bench_build(ctx, k, lines):
    n = N_BUILD
    d_ods, d_eds, roots = device_batches(ctx, k, n)
    # the three routes give the same data roots
    got = np.empty((n, 32), dtype=np.uint8)
    for d, kind in ((d_eds, _lib.CDA_SET_FROM_EDS), (d_ods, _lib.CDA_SET_FROM_ODS)):
        h = build_set(ctx, d, kind, k, n)()
        ctx.check(ctx.lib.cda_square_set_dah(h, None, None, ptr(got), None))
        ctx.lib.cda_square_set_destroy(h)
        assert np.array_equal(got, roots), "a set's data roots differ from the batch's"
    t1 = timed(build_set(ctx, d_eds, _lib.CDA_SET_FROM_EDS, k, n), REPS, ctx.lib.cda_square_set_destroy)
    t2 = timed(build_set(ctx, d_ods, _lib.CDA_SET_FROM_ODS, k, n), REPS, ctx.lib.cda_square_set_destroy)
    t0 = timed(build_singles(ctx, d_ods, k, n), REPS, lambda hs: [ctx.lib.cda_square_destroy(h) for h in hs])
    med = {}
    lines += [f"(a) k = {k}: {n} resident squares from a device batch; warm-up {WARMUP}, {REPS} timed builds"]
    for key, name, t in (("a1", "a1: cda_square_set_create_device, CDA_SET_FROM_EDS (copy, hash)", t1),
                         ("a2", "a2: cda_square_set_create_device, CDA_SET_FROM_ODS (extend, hash)", t2),
                         ("a0", f"a0: D2H of the ODS batch, then {n} cda_square_create calls", t0)):
        m = med[key] = statistics.median(t)
        lines += [f"  {name}",
                  f"    ms per {n} squares: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"
                  f"   per square {m / n * 1e3:.3f} ms  squares/s {n / m:,.0f}"]
    lines += [f"  a0 / a1 = {med['a0'] / med['a1']:.2f}   a0 / a2 = {med['a0'] / med['a2']:.2f}", ""]


def bench_serve(ctx, k, lines):
    n, per = N_SERVE, PER_SQUARE
    W, D = 2 * k, (2 * k).bit_length() - 1
    d_ods, d_eds, _ = device_batches(ctx, k, n)
    h = build_set(ctx, d_eds, _lib.CDA_SET_FROM_EDS, k, n)()
    del d_ods, d_eds
    count = n * per
    rng = np.random.default_rng(k)
    squares = rng.permutation(np.repeat(np.arange(n, dtype=np.uint32), per))   # interleaved
    rows = rng.integers(0, W, count).astype(np.uint32)
    cols = rng.integers(0, W, count).astype(np.uint32)
    axes = rng.integers(0, 2, count).astype(np.uint8)
    item = (512, 29, D * 90, 90, 32, (D + 1) * 32)
    out1 = [np.zeros((count, s), dtype=np.uint8) for s in item]
    out0 = [np.zeros((count, s), dtype=np.uint8) for s in item]
    args1 = (h, squares.ctypes.data_as(U32P), rows.ctypes.data_as(U32P), cols.ctypes.data_as(U32P), ptr(axes), count,
             *(ptr(a) for a in out1))

    def one_call():
        ctx.check(ctx.lib.cda_square_set_sample_proofs(*args1))

    # the per-member route: requests grouped by square, outputs at the grouped positions, scattered back once
    order = np.argsort(squares, kind="stable")
    g_rows, g_cols, g_axes = rows[order].copy(), cols[order].copy(), axes[order].copy()
    grouped = [np.zeros((count, s), dtype=np.uint8) for s in item]
    members = []
    for y in range(n):
        m = C.c_void_p()
        ctx.check(ctx.lib.cda_square_set_at(h, y, C.byref(m)))
        lo = y * per
        members.append((m, g_rows[lo:].ctypes.data_as(U32P), g_cols[lo:].ctypes.data_as(U32P), ptr(g_axes[lo:]), per,
                        *(ptr(a[lo:]) for a in grouped)))
    fn = ctx.lib.cda_square_sample_proofs

    def per_member():
        for a in members:
            rc = fn(*a)
            if rc:
                ctx.check(rc)

    t1 = timed(one_call, SAMPLE_REPS)
    t0 = timed(per_member, SAMPLE_REPS)
    for dst, src in zip(out0, grouped):
        dst[order] = src
    for a, b in zip(out1, out0):
        assert np.array_equal(a, b), "the set call and the per-member calls differ"
    ctx.lib.cda_square_set_destroy(h)
    nbytes = sum(a.nbytes for a in out1)
    m1, m0 = statistics.median(t1), statistics.median(t0)
    lines += [f"(b) k = {k}: {per} samples of each of {n} squares ({count} samples, {nbytes} bytes returned); "
              f"warm-up {WARMUP}, {SAMPLE_REPS} timed rounds"]
    for name, t, m in (("b1: one cda_square_set_sample_proofs call", t1, m1),
                       (f"b0: {n} cda_square_sample_proofs calls on the members", t0, m0)):
        lines += [f"  {name}",
                  f"    ms per {count} samples: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"
                  f"   per sample {m / count * 1e6:.3f} us  samples/s {count / m:,.0f}  {nbytes / m / 1e9:.3f} GB/s"]
    lines += [f"  b0 / b1 = {m0 / m1:.1f}", ""]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "square_set.txt")
    ctx = default_context()
    lines = [f"sets of resident squares on one GPU; {ctx.lib.cda_version().decode()}",
             "wall time around calls that return with their work complete (host clock)", ""]
    for k in (128, 32):
        bench_build(ctx, k, lines)
        bench_serve(ctx, k, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
