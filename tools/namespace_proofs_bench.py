#!/usr/bin/env python3
"""Namespace queries of one k = 128 resident square on one GPU: 4 096 present
and 4 096 absent namespaces, one call each.  A measurement, not a gate.

For each of the two batches, wall time around the synchronised C calls (host
buffers allocated before, no Python objects built):
  * cda_square_namespace_plan + cda_square_namespace_proofs (the search runs in
    both: two search launches, two copies back of n * k words, one emit launch);
  * cda_namespace_proofs_verify of the answer against the square's row roots;
  * cda_square_share_proofs for the same leaf ranges handed over ready-made
    (nodes and shares only), which shows what the search and its extra round
    trip cost.  An absence segment's range is its one leaf.
WARMUP calls first, then REPS timed calls; median, min and max are reported.

Writes profiles/namespace_proofs.txt (or argv[1]).
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
from celestia_da import proof as gpr  # noqa: E402
from celestia_da.namespace import NamespaceProofsBatch, namespace_plan  # noqa: E402

K = 128
N = 4096
WARMUP = int(os.environ.get("WARMUP", "3"))
REPS = int(os.environ.get("REPS", "15"))
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


def line(what, t, nbytes=None):
    m = statistics.median(t)
    rate = f"  ({nbytes / m / 1e9:.3f} GB/s)" if nbytes else ""
    return f"  {what}, ms: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}{rate}"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "namespace_proofs.txt")
    ctx = default_context()
    ods = testfactory.random_square(K, 0).reshape(K * K, 512)
    sq = gpr.ResidentSquare(ods, ctx)
    rows = sq.dah()[0]
    roots = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    step = K * K // N
    present = np.ascontiguousarray(ods[::step, :29])
    have = {x.tobytes() for x in ods[:, :29]}
    absent = np.frombuffer(b"".join((int.from_bytes(x.tobytes(), "big") + 1).to_bytes(29, "big") for x in present),
                           dtype=np.uint8).reshape(N, 29).copy()
    assert len(present) == N and not any(x.tobytes() in have for x in absent)
    lines = [f"namespace queries of one k = {K} resident square; {ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s) (host buffers out); warm-up {WARMUP}, {REPS} timed calls", ""]
    for name, ns in (("present", present), ("absent", absent)):
        plan = namespace_plan(sq, ns)
        out = NamespaceProofsBatch.empty(K, ns, plan)
        o, p = out.out_struct(), _lib.NamespacePlanT()

        def prove():
            ctx.check(ctx.lib.cda_square_namespace_plan(sq.h, ptr(ns), N, C.byref(p)))
            ctx.check(ctx.lib.cda_square_namespace_proofs(sq.h, ptr(ns), N, C.byref(o)))
        t_prove = timed(prove)
        b = out.batch()
        verdict = np.full(N, 255, dtype=np.uint8)

        def verify():
            ctx.check(ctx.lib.cda_namespace_proofs_verify(ctx.h, K, ptr(roots), C.byref(b), ptr(verdict)))
        t_verify = timed(verify)
        assert not verdict.any(), "an answer of the bench failed to verify"
        # the same leaf ranges, ready-made
        ranges = np.stack([out.row * K + out.nmt_start.astype(np.uint32),
                           out.row * K + out.nmt_end.astype(np.uint32)], axis=1).astype(np.uint32)
        made = gpr.ShareProofsBatch.empty(K, ranges)
        starts, ends = np.ascontiguousarray(ranges[:, 0]), np.ascontiguousarray(ranges[:, 1])
        u32p = C.POINTER(C.c_uint32)
        so = made.out_struct(skip=tuple(f for f in made.FIELDS if f not in ("nodes", "shares")))

        def ready_made():
            ctx.check(ctx.lib.cda_square_share_proofs(sq.h, starts.ctypes.data_as(u32p), ends.ctypes.data_as(u32p),
                                                      len(ranges), C.byref(so)))
        t_made = timed(ready_made)
        assert np.array_equal(made.nodes, out.nodes)
        nbytes = out.nodes.nbytes + out.shares.nbytes + out.absence_leaf.nbytes
        mp, mm = statistics.median(t_prove), statistics.median(t_made)
        lines += [f"{name}: {N} namespaces in one call: {plan['n_segments']} segments, {plan['n_nodes']} nodes, "
                  f"{plan['n_shares']} shares ({nbytes} bytes of nodes, shares and absence leaves; "
                  f"{N * K * 4} bytes of search words per search)",
                  line("cda_square_namespace_plan + cda_square_namespace_proofs", t_prove, nbytes),
                  line("cda_namespace_proofs_verify", t_verify),
                  line(f"cda_square_share_proofs of the same {len(ranges)} ranges, nodes and shares only", t_made),
                  f"  plan + proofs / ready-made = {mp / mm:.1f}", ""]
    sq.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
