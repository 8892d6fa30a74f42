#!/usr/bin/env python3
"""Building and checking bad-encoding fraud proofs of one k = 128 square on one
GPU.  A measurement, not a gate: no target was fixed in advance.

The square: a random k = 128 square extended by the library, one Q1 cell
flipped, all 4k roots recomputed from the corrupted cells; the proofs accuse
the corrupted row.
  (a) cda_befp_build from the host EDS (the 32 MiB square goes up in the call);
  (b) cda_befp_build_device from the same square in HBM;
  (c) the same W proofs through W cda_nmt_prove_range calls, one per orthogonal
      vector: the only route without (a) / (b);
  (d) cda_befp_verify of 1 proof with all W shares;
  (e) cda_befp_verify of 64 such proofs in one call;
  (f) the CPU yardstick (tests/befp_ref.py validate, numpy + hashlib) on one
      proof -- what (d) and (e) are compared with, per proof.
The timed region is the C call alone (for (c): the loop of C calls, buffers
allocated once), host buffers in and out, copies and synchronisations included.
Wall time, WARMUP calls first, then REPS timed calls; median, min and max.

Writes profiles/befp.txt (or argv[1]).
"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("celestia-app_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402

from celestia_da import _lib, byzantine, default_context, testfactory  # noqa: E402

K = 128
W = 2 * K
D = 8
N_BATCH = 64
WARMUP = int(os.environ.get("WARMUP", "3"))
REPS = int(os.environ.get("REPS", "20"))
ptr = _lib.ptr


def timed(call, warmup=WARMUP, reps=REPS):
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return times


def malicious_square(ctx):
    ods = np.ascontiguousarray(testfactory.random_square(K, 0), dtype=np.uint8).reshape(-1, 512)
    eds = np.empty((W, W, 512), dtype=np.uint8)
    rows, cols = np.empty((W, 90), dtype=np.uint8), np.empty((W, 90), dtype=np.uint8)
    root = np.empty(32, dtype=np.uint8)
    ctx.check(ctx.lib.cda_extend_dah(ctx.h, ptr(ods), K * K, ptr(eds), ptr(rows), ptr(cols), ptr(root)))
    r, c = K - 1, K
    eds[r, c, 100:104] ^= 0x5A
    ctx.check(ctx.lib.cda_dah_from_eds(ctx.h, ptr(eds), W, ptr(rows), ptr(cols), ptr(root)))
    return eds, rows, cols, r


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "befp.txt")
    import torch
    ctx = default_context()
    eds, rows, cols, r = malicious_square(ctx)
    u32p = C.POINTER(C.c_uint32)
    n = C.c_uint32(0)
    positions = np.empty(W, dtype=np.uint32)
    shares = np.empty((W, 512), dtype=np.uint8)
    nodes = np.empty((W, D, 90), dtype=np.uint8)
    tail = (W, 0, r, ptr(rows), ptr(cols), C.byref(n), positions.ctypes.data_as(u32p), ptr(shares), ptr(nodes))

    def build_host():
        ctx.check(ctx.lib.cda_befp_build(ctx.h, ptr(eds), *tail))
    t_a = timed(build_host)
    assert n.value == W
    nodes_a = nodes.copy()

    d_eds = torch.from_numpy(eds.reshape(-1)).to("cuda")
    torch.cuda.synchronize()

    def build_device():
        ctx.check(ctx.lib.cda_befp_build_device(ctx.h, d_eds.data_ptr(), *tail))
    t_b = timed(build_device)
    assert n.value == W and np.array_equal(nodes, nodes_a)

    columns = np.ascontiguousarray(eds.transpose(1, 0, 2))   # orthogonal vector p, contiguous
    one = np.empty((2 * D, 90), dtype=np.uint8)
    cnt = C.c_uint32(0)
    got = np.empty((W, D, 90), dtype=np.uint8)

    def prove_one_by_one():
        for p in range(W):
            rc = ctx.lib.cda_nmt_prove_range(ctx.h, ptr(columns[p]), 512, W, K, p, r, r + 1, ptr(one), C.byref(cnt),
                                             None)
            if rc:
                ctx.check(rc)
            got[p] = one[:D]
    t_c = timed(prove_one_by_one, 1, max(3, REPS // 5))
    assert np.array_equal(got, nodes_a), "the two routes must give the same proofs"

    proof = byzantine.BadEncodingProof(K, 0, r, positions.copy(), np.ones(W, dtype=np.uint8), shares.copy(),
                                       nodes_a)
    res = {}
    for key, count in (("d", 1), ("e", N_BATCH)):
        b, keep = byzantine.pack_batch([proof] * count, [(rows, cols)] * count)
        verdict = np.full(count, 255, dtype=np.uint8)
        rebuilt = np.empty((count, 90), dtype=np.uint8)

        def verify():
            ctx.check(ctx.lib.cda_befp_verify(ctx.h, C.byref(b), ptr(verdict), ptr(rebuilt)))
        res[key] = timed(verify)
        assert not verdict.any(), "the bench's proof must confirm the fraud"
        del keep

    import befp_ref
    want = None

    def yardstick():
        nonlocal want
        want = befp_ref.validate(proof, rows, cols)
    t_f = timed(yardstick, 0, 3)
    assert want[0] == 0 and want[1] == rebuilt[0].tobytes()

    def line(t, per=None, unit=""):
        m = statistics.median(t)
        s = f"  ms per call: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"
        return s + (f"  ({m / per * 1e6:.1f} us per {unit})" if per else "")
    med = {k_: statistics.median(v) for k_, v in (("a", t_a), ("b", t_b), ("c", t_c), ("d", res["d"]),
                                                   ("e", res["e"]), ("f", t_f))}
    lines = [f"bad-encoding fraud proofs of one k = {K} square (row {r}, {W} shares per proof); "
             f"{ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised call(s) (host buffers in and out); warm-up {WARMUP}, {REPS} timed calls",
             "",
             "a: cda_befp_build, host EDS (32 MiB up in the call)", line(t_a, W, "share"), "",
             "b: cda_befp_build_device, EDS in HBM", line(t_b, W, "share"), "",
             f"c: the same proofs, {W} cda_nmt_prove_range calls (1 warm-up, {len(t_c)} timed)", line(t_c, W, "share"), "",
             "d: cda_befp_verify, 1 proof", line(res["d"], 1, "proof"), "",
             f"e: cda_befp_verify, {N_BATCH} proofs in one call", line(res["e"], N_BATCH, "proof"), "",
             "f: CPU yardstick (tests/befp_ref.py validate), 1 proof (no warm-up, 3 timed)", line(t_f, 1, "proof"), "",
             f"(c) / (a) = {med['c'] / med['a']:.1f}   (c) / (b) = {med['c'] / med['b']:.1f}",
             f"(f) / (d) = {med['f'] / med['d']:.1f}   {N_BATCH} x (f) / (e) = {N_BATCH * med['f'] / med['e']:.1f}",
             ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
