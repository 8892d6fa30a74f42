#!/usr/bin/env python3
"""Throughput of cda_share_proofs_verify (ShareProof.Validate, batched) on one
GPU.  A measurement, not a gate: there is no earlier figure and no reference
binary to compare with.

Two workloads from one k = 128 resident square whose shares carry one
namespace (Validate takes one namespace per proof):
  (a) 4 096 single-share proofs in one call;
  (b) the one proof of the whole ODS: 128 segments of 128 leaves.
The batch is built once; the timed region is the C call alone (host buffers
in, verdicts out: the H2D copy of the shares and the call's one stream
synchronisation are inside it).  Wall time around the synchronised call,
WARMUP calls first, then REPS timed calls; median, min and max are reported.
Compressions are counted from the proofs' shapes: 9 per 512-byte leaf, 3 per
NMT node hash, 2 for a row root's leaf hash and 2 per aunt.

Writes profiles/proof_verify.txt (or argv[1]).
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

K = 128
WARMUP = int(os.environ.get("WARMUP", "5"))
REPS = int(os.environ.get("REPS", "30"))
SHA_PROBE = 28.45e9   # compressions/s of the register-only SHA probe


def compressions(proofs) -> int:
    n = 0
    for p in proofs:
        n += 9 * len(p.data)
        for sp, q in zip(p.share_proofs, p.row_proof.proofs):
            n += 3 * (sp.end - sp.start - 1 + len(sp.nodes)) + 2 + 2 * len(q.aunts)
    return n


def entries(proofs, root):
    out = []
    for p in proofs:
        ns = bytes([p.namespace_version]) + bytes(p.namespace_id)
        segs = [(s.start, s.end, s.nodes, r, q)
                for s, r, q in zip(p.share_proofs, p.row_proof.row_roots, p.row_proof.proofs)]
        out.append((ns, root, segs, p.data))
    return out


def measure(ctx, proofs, root):
    b, keep = gpr._build_batch(29, 512, entries(proofs, root), rows=True, nmt=True)
    verdict = np.full(len(proofs), 255, dtype=np.uint8)
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        rc = ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(b), _lib.ptr(verdict))
        dt = time.perf_counter() - t0
        ctx.check(rc)
        if i >= WARMUP:
            times.append(dt)
    assert not verdict.any(), "a proof of the bench failed to verify"
    del keep
    return times


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "proof_verify.txt")
    ctx = default_context()
    ods = testfactory.random_square(K, 0).copy()
    ods[:, :29] = ods[0, :29]
    ns = bytes(ods[0, :29])
    sq = gpr.ResidentSquare(ods, ctx)
    root = sq.dah()[2]
    step = K * K // 4096
    work = [("a: 4096 single-share proofs, one call", [sq.share_proof(ns, s, s + 1) for s in range(0, K * K, step)]),
            ("b: one proof of the whole ODS (128 segments x 128 leaves)", [sq.share_proof(ns, 0, K * K)])]
    sq.close()
    lines = [f"cda_share_proofs_verify, k = {K} square, ns_len 29, 512-byte shares; {ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call (host buffers in, verdicts out); warm-up {WARMUP}, {REPS} timed calls",
             ""]
    for name, proofs in work:
        t = measure(ctx, proofs, root)
        med, comp = statistics.median(t), compressions(proofs)
        segs = sum(len(p.share_proofs) for p in proofs)
        lines += [name,
                  f"  proofs {len(proofs)}  segments {segs}  shares {sum(len(p.data) for p in proofs)}  "
                  f"compressions {comp} ({comp / len(proofs):.0f} per proof)",
                  f"  call ms: median {med * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}",
                  f"  proofs/s {len(proofs) / med:,.0f}  shares/s {sum(len(p.data) for p in proofs) / med:,.0f}",
                  f"  compressions/s {comp / med / 1e9:.3f} G = {comp / med / SHA_PROBE:.3f} of the SHA probe's "
                  f"{SHA_PROBE / 1e9:.2f} G/s (whole call, copies included: not a kernel's share of peak)",
                  ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
