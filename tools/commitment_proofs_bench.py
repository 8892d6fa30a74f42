#!/usr/bin/env python3
"""Blob inclusion by share commitment against the share-proof path, for the
blobs of one k = 128 resident square on one GPU.  A measurement, not a gate.

Three workloads: (a) 64 blobs of 256 shares, (b) one blob of 16 384 shares (the
whole square), (c) 4 096 blobs of one share.  For each, wall time around the
synchronised C calls (host buffers allocated before, no Python objects built)
and the bytes the prover returns:
  * commitment proofs: cda_square_commitment_proofs (every output, the
    commitments among them) and cda_commitment_proofs_verify;
  * what the same question costs without them: cda_square_share_proofs over the
    blobs' ranges (every output, the shares among them), cda_share_proofs_verify,
    and cda_square_blob_commitments to recompute the commitments the verdicts
    are then compared with.
WARMUP calls first, then REPS timed calls; median, min and max are reported.

Writes profiles/commitment_proofs.txt (or argv[1]).
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
THRESHOLD = 64
WARMUP = int(os.environ.get("WARMUP", "3"))
REPS = int(os.environ.get("REPS", "15"))
ptr = _lib.ptr
u32p = C.POINTER(C.c_uint32)


def timed(call):
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= WARMUP:
            times.append(dt)
    return times


def line(what, t):
    return f"  {what}, ms: median {statistics.median(t) * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "commitment_proofs.txt")
    ctx = default_context()
    base = testfactory.random_square(K, 0).reshape(K * K, 512)
    # (name, starts, lens, shares per namespace): a blob's shares carry one namespace, as a share proof needs
    workloads = [("(a) 64 blobs of 256 shares", [i * 256 for i in range(64)], [256] * 64, 256),
                 ("(b) one blob of 16 384 shares", [0], [K * K], K * K),
                 ("(c) 4 096 blobs of one share", [i * 4 for i in range(4096)], [1] * 4096, 1)]
    lines = [f"blob inclusion proofs of one k = {K} resident square, threshold {THRESHOLD}; "
             f"{ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s) (host buffers out); warm-up {WARMUP}, {REPS} timed calls", ""]
    for name, starts, lens, per_ns in workloads:
        n = len(starts)
        ods = base.copy()
        group = np.arange(K * K, dtype=np.uint64) // per_ns + 1   # ascending version-0 blob namespaces
        ods[:, :29] = 0
        ods[:, 21:29] = group.astype(">u8").view(np.uint8).reshape(-1, 8)
        sq = gpr.ResidentSquare(ods, ctx)
        assert not sq.push_order_error
        data_root = sq.dah()[2]
        st, ln = np.array(starts, dtype=np.uint32), np.array(lens, dtype=np.uint32)
        # by commitment
        out = gpr.CommitmentProofsBatch.empty(K, st, ln, THRESHOLD)
        o = out.out_struct()

        def build():
            ctx.check(ctx.lib.cda_square_commitment_proofs(sq.h, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p), n,
                                                           THRESHOLD, C.byref(o)))
        t_build = timed(build)
        assert (out.norm_start == st).all()
        b = out.batch(data_root)
        verdict = np.full(n, 255, dtype=np.uint8)

        def verify():
            ctx.check(ctx.lib.cda_commitment_proofs_verify(ctx.h, C.byref(b), ptr(verdict)))
        t_verify = timed(verify)
        assert not verdict.any(), "a commitment proof of the bench failed to verify"
        nbytes = sum(a.nbytes for a in out.arrays())
        # by shares
        ranges = np.stack([st, st + ln], axis=1).astype(np.uint32)
        shp = gpr.ShareProofsBatch.empty(K, ranges)
        so = shp.out_struct()
        ends = np.ascontiguousarray(ranges[:, 1])

        def share_build():
            ctx.check(ctx.lib.cda_square_share_proofs(sq.h, st.ctypes.data_as(u32p), ends.ctypes.data_as(u32p), n,
                                                      C.byref(so)))
        t_share_build = timed(share_build)
        sb = shp.batch(data_root)
        sverdict = np.full(n, 255, dtype=np.uint8)
        commits = np.empty(32 * n, dtype=np.uint8)

        def share_verify():
            ctx.check(ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(sb), ptr(sverdict)))
            ctx.check(ctx.lib.cda_square_blob_commitments(sq.h, st.ctypes.data_as(u32p), ln.ctypes.data_as(u32p), n,
                                                          THRESHOLD, ptr(commits)))
        t_share_verify = timed(share_verify)
        assert not sverdict.any() and commits.tobytes() == out.commitments.tobytes()
        sbytes = sum(a.nbytes for a in shp.arrays()) + commits.nbytes
        mb, mv = statistics.median(t_build), statistics.median(t_verify)
        msb, msv = statistics.median(t_share_build), statistics.median(t_share_verify)
        lines += [f"{name}: {len(out.row_roots)} rows, {len(out.subtree_roots)} subtree roots, {len(out.nodes)} nodes",
                  f"  by commitment: {nbytes} bytes returned",
                  line("  cda_square_commitment_proofs", t_build),
                  line("  cda_commitment_proofs_verify", t_verify),
                  f"  by shares: {sbytes} bytes returned",
                  line("  cda_square_share_proofs", t_share_build),
                  line("  cda_share_proofs_verify + cda_square_blob_commitments", t_share_verify),
                  f"  bytes {sbytes / nbytes:.1f}x fewer, build {msb / mb:.2f}x, verify {msv / mv:.2f}x "
                  f"(shares path / commitment path)", ""]
        sq.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
