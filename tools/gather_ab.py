#!/usr/bin/env python3
"""The resident squares' gather kernel (csrc/proof.hip gather_kernel) through the
callers it had before the share parser: cda_square_subtree_root (one piece of 90
bytes) and cda_square_blob_commitments (96-byte slots: one per subtree root of
every blob), on one k = 128 resident square.  Run once per library to compare
two builds of the kernel:

    python tools/gather_ab.py LABEL OUT          (the library: CDA_LIB, or libcda.so)

appends one block of lines to OUT.  Wall time around the synchronised C call
(the commitment call's Merkle launch included), WARMUP calls, then REPS timed
calls; median, min and max.  The outputs' SHA-256 is printed so that two builds
can be seen to return the same bytes.
"""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("celestia-app_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402

K = 128
WARMUP = int(os.environ.get("WARMUP", "5"))
REPS = int(os.environ.get("REPS", "40"))


def timed(call):
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= WARMUP:
            times.append(dt)
    return times


def main():
    label, out_path = sys.argv[1], sys.argv[2]
    from celestia_da import default_context, proof, testfactory
    ctx = default_context()
    ods = np.ascontiguousarray(testfactory.random_square(K, 0), dtype=np.uint8).reshape(-1, 512)
    sq = proof.ResidentSquare(ods, ctx)
    digest = hashlib.sha256()
    cases = [("subtree_root, 1 piece", lambda: sq.subtree_root(5, [False, True, True]))]
    for name, starts, lens in (("blob_commitments, 4 096 one-share blobs (4 096 slots)", list(range(4096)), [1] * 4096),
                               ("blob_commitments, 64 blobs of 256 shares", [256 * i for i in range(64)], [256] * 64),
                               ("blob_commitments, the whole square as one blob", [0], [K * K])):
        cases.append((name, lambda s=starts, n=lens: sq.blob_commitments(s, n)))
    lines = [f"{label}: {ctx.lib.cda_version().decode()}; k = {K}; warm-up {WARMUP}, {REPS} timed calls"]
    for name, call in cases:
        got = call()
        digest.update(got if isinstance(got, bytes) else b"".join(got))
        t = timed(call)
        lines.append(f"  {name}: ms per call: median {statistics.median(t) * 1e3:.4f}  min {min(t) * 1e3:.4f}  "
                     f"max {max(t) * 1e3:.4f}")
    lines.append(f"  outputs sha256 {digest.hexdigest()[:16]}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out_path, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
