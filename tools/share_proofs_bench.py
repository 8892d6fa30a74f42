#!/usr/bin/env python3
"""Share proofs of many ranges from one k = 128 resident square on one GPU:
the batch call (cda_square_share_proofs, one launch) against the loop of
single-range calls (cda_square_share_proof), which returns the same bytes.
A measurement, not a gate: the only requirement is that the batch call is not
slower than the loop in (a), (b) and (c).

  (a) 4 096 single-share ranges: one batch call / 4 096 single calls;
  (b) the 128 full rows in one batch call / 128 single calls, and the whole
      square as one range in a batch call / one single call;
  (c) the 274 transaction proofs of mainnet block 408 (tests/golden):
      new_tx_inclusion_proofs / new_tx_inclusion_proof per index, and inside the
      former the share-range look-ups (host only) on their own: the one
      cda_square_tx_share_ranges call it makes, and the 274
      cda_square_tx_share_range calls that call replaced.
For (a) and (b) the timed region is the C call alone (for the loop: the loop
of C calls, buffers allocated once, no Python objects built): host buffers
out, the copies and the stream synchronisation inside it.  (c) times the
Python functions, ShareProof objects included, on both sides.  Wall time,
WARMUP calls first, then REPS timed calls (REPS_C for (c)); median, min and
max are reported.

These are whole-call figures.  The kernels' own times come from a kernel
trace of this tool in a run of its own (rocprofv3 --kernel-trace --stats --
python3 tools/share_proofs_bench.py OUT with WARMUP=1 REPS=3 REPS_C=0).

Writes profiles/share_proofs_batch.txt (or argv[1]).
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

from celestia_da import _lib, default_context, testfactory  # noqa: E402
from celestia_da import proof as gpr  # noqa: E402

K = 128
N = 4096
WARMUP = int(os.environ.get("WARMUP", "3"))
REPS = int(os.environ.get("REPS", "15"))
REPS_C = int(os.environ.get("REPS_C", "3"))
ptr = _lib.ptr


def timed(call, warmup=None, reps=None):
    warmup, reps = WARMUP if warmup is None else warmup, REPS if reps is None else reps
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return times


def batch_call(ctx, sq, ranges):
    out = gpr.ShareProofsBatch.empty(K, ranges)
    r = out.ranges
    starts, ends = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    u32p = C.POINTER(C.c_uint32)
    o = out.out_struct()
    args = (sq.h, starts.ctypes.data_as(u32p), ends.ctypes.data_as(u32p), len(r), C.byref(o))

    def call():
        ctx.check(ctx.lib.cda_square_share_proofs(*args))
    return timed(call), out, sum(a.nbytes for a in (out.nodes, out.row_roots, out.rfc_leaf_hash, out.aunts,
                                                   out.shares))


def loop_call(ctx, sq, ranges):
    """One cda_square_share_proof call per range, into buffers sized for the longest."""
    D, A = 8, 9
    rows = max((e - 1) // K - s // K + 1 for s, e in ranges)
    shares = np.empty(max(e - s for s, e in ranges) * 512, dtype=np.uint8)
    nodes = np.empty(rows * 2 * D * 90, dtype=np.uint8)
    root, leaf, aunts = (np.empty(rows * w, dtype=np.uint8) for w in (90, 32, A * 32))
    ns, ne, cnt = (C.c_int32 * rows)(), (C.c_int32 * rows)(), (C.c_uint32 * rows)()
    r0, r1 = C.c_uint32(), C.c_uint32()
    fn, h = ctx.lib.cda_square_share_proof, sq.h
    tail = (ptr(shares), C.byref(r0), C.byref(r1), ns, ne, cnt, ptr(nodes), ptr(root), ptr(leaf), ptr(aunts))
    todo = [(int(s), int(e)) for s, e in ranges]

    def call():
        for s, e in todo:
            rc = fn(h, s, e, *tail)
            if rc:
                ctx.check(rc)
    return timed(call)


def block408():
    from test_square import block408 as load
    return load()[0]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "share_proofs_batch.txt")
    ctx = default_context()
    sq = gpr.ResidentSquare(testfactory.random_square(K, 0), ctx)
    root = sq.dah()[2]
    step = K * K // N
    cases = [("a", f"{N} single-share ranges", [(s, s + 1) for s in range(0, K * K, step)]),
             ("b1", f"the {K} full rows", [(r * K, r * K + K) for r in range(K)]),
             ("b2", "the whole square as one range", [(0, K * K)])]
    lines = [f"share proofs of ranges of one k = {K} resident square; {ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s) (host buffers out); warm-up {WARMUP}, {REPS} timed calls",
             ""]
    slower = []
    for key, name, ranges in cases:
        t_batch, out, nbytes = batch_call(ctx, sq, ranges)
        if key == "a":   # single shares: one namespace each, so the batch verifies as it is
            assert not out.verify(root, ctx).any(), "a proof of the bench failed to verify"
        t_loop = loop_call(ctx, sq, ranges)
        mb, ml = statistics.median(t_batch), statistics.median(t_loop)
        lines += [f"{key}: {name} ({len(ranges)} ranges, {nbytes} bytes of proofs and shares)",
                  f"  one cda_square_share_proofs call, ms: median {mb * 1e3:.3f}  min {min(t_batch) * 1e3:.3f}  "
                  f"max {max(t_batch) * 1e3:.3f}  ({nbytes / mb / 1e9:.3f} GB/s)",
                  f"  {len(ranges)} cda_square_share_proof calls, ms: median {ml * 1e3:.3f}  min {min(t_loop) * 1e3:.3f}  "
                  f"max {max(t_loop) * 1e3:.3f}",
                  f"  loop / batch = {ml / mb:.1f}", ""]
        if mb > ml:
            slower.append(key)
    sq.close()

    if REPS_C:
        txs = block408()
        idx = list(range(len(txs)))
        from celestia_da import square
        ub, thr = square.SQUARE_SIZE_UPPER_BOUND, square.SUBTREE_ROOT_THRESHOLD
        t_batch = timed(lambda: gpr.new_tx_inclusion_proofs(txs), 1, REPS_C)
        t_lookup = timed(lambda: gpr.tx_share_ranges(txs, idx, ub, thr), 1, REPS_C)
        t_singles = timed(lambda: [gpr.tx_share_range(txs, i, ub, thr) for i in idx], 1, REPS_C)
        t_loop = timed(lambda: [gpr.new_tx_inclusion_proof(txs, i) for i in idx], 1, REPS_C)
        mb, mk, ml, ms = (statistics.median(t) for t in (t_batch, t_lookup, t_loop, t_singles))
        lines += [f"c: the {len(txs)} transaction proofs of block 408; warm-up 1, {REPS_C} timed calls",
                  f"  new_tx_inclusion_proofs(txs), ms: median {mb * 1e3:.2f}  min {min(t_batch) * 1e3:.2f}  "
                  f"max {max(t_batch) * 1e3:.2f}",
                  f"    of which the {len(txs)} share-range look-ups, one cda_square_tx_share_ranges call (host), ms: "
                  f"median {mk * 1e3:.2f}  min {min(t_lookup) * 1e3:.2f}  max {max(t_lookup) * 1e3:.2f}  "
                  f"({100 * mk / mb:.0f} %)",
                  f"    (the same look-ups as {len(txs)} cda_square_tx_share_range calls, ms: median {ms * 1e3:.2f}  "
                  f"min {min(t_singles) * 1e3:.2f}  max {max(t_singles) * 1e3:.2f})",
                  f"  {len(txs)} new_tx_inclusion_proof calls, ms: median {ml * 1e3:.2f}  min {min(t_loop) * 1e3:.2f}  "
                  f"max {max(t_loop) * 1e3:.2f}",
                  f"  loop / batch = {ml / mb:.1f}", ""]
        if mb > ml:
            slower.append("c")
    lines += ["the batch call is slower than the loop in: " + (", ".join(slower) if slower else "no case"), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
