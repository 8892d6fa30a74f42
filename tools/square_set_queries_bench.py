#!/usr/bin/env python3
"""Namespace and share-range proofs across a set of resident squares, and the
verification of the namespace answers, on one GPU, against the routes that
exist without the set calls.  A measurement, not a gate: no threshold is set.

For k = 128 and k = 32, a set of 256 members (four distinct squares repeated):
  (c) one namespace per member (256 queries), and (d) 16 per member (4 096,
      members interleaved), half of them present and half absent:
        1  one cda_square_set_namespace_proofs call;
        0  256 cda_square_namespace_proofs calls on the members.
  (e) 4 096 single-share ranges, 16 of each member, members interleaved:
        1  one cda_square_set_share_proofs call;
        0  256 cda_square_share_proofs calls on the members, 16 ranges each.
  (f), (g) verification of the answers of (c) and (d):
        1  one cda_namespace_proofs_verify_set call against the 256 DAHs;
        0  256 cda_namespace_proofs_verify calls, one per member's batch.
Every route writes into buffers sized before the timed region (the plans are
outside it on both sides), and the answers of both routes are compared byte
for byte.  Wall time around calls that end synchronised; WARMUP rounds first,
then REPS timed ones; median, min and max are reported.

Writes profiles/square_set_queries.txt (or argv[1]).
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
from celestia_da.namespace import NamespaceProofsBatch  # noqa: E402
from celestia_da.proof import ShareProofsBatch  # noqa: E402

WARMUP = int(os.environ.get("WARMUP", "2"))
REPS = int(os.environ.get("REPS", "20"))
N, DISTINCT = 256, 4
ptr = _lib.ptr
U32P = C.POINTER(C.c_uint32)


def p32(a):
    return a.ctypes.data_as(U32P)


def timed(call):
    times = []
    for i in range(WARMUP + REPS):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= WARMUP:
            times.append(dt)
    return times


def report(lines, title, unit, count, routes):
    lines += [title]
    med = []
    for name, t in routes:
        m = statistics.median(t)
        med.append(m)
        lines += [f"  {name}",
                  f"    ms: median {m * 1e3:.3f}  min {min(t) * 1e3:.3f}  max {max(t) * 1e3:.3f}"
                  f"   per {unit} {m / count * 1e6:.3f} us"]
    lines += [f"  route 0 / route 1 = {med[1] / med[0]:.1f}", ""]


def make_set(ctx, k):
    import torch
    distinct = np.stack([testfactory.random_square(k, 10 + i).reshape(k * k, 512) for i in range(DISTINCT)])
    d_ods = torch.from_numpy(distinct).cuda()[torch.arange(N, device="cuda") % DISTINCT].contiguous()
    h = C.c_void_p()
    ctx.check(ctx.lib.cda_square_set_create_device(ctx.h, d_ods.data_ptr(), _lib.CDA_SET_FROM_ODS, k, N, None, C.byref(h)))
    members = []
    for y in range(N):
        m = C.c_void_p()
        ctx.check(ctx.lib.cda_square_set_at(h, y, C.byref(m)))
        members.append(m)
    return h, members, distinct


def namespace_queries(distinct, k, per, seed):
    """per queries of each member, grouped by member: even ones present, odd ones just above a present one."""
    rng = np.random.default_rng(seed)
    nss = np.zeros((N, per, 29), dtype=np.uint8)
    for y in range(N):
        cells = rng.integers(0, k * k, per)
        for j, c in enumerate(cells.tolist()):
            ns = distinct[y % DISTINCT][c, :29].tobytes()
            if j % 2:
                ns = (int.from_bytes(ns, "big") + 1).to_bytes(29, "big")
            nss[y, j] = np.frombuffer(ns, dtype=np.uint8)
    return nss


def bench_namespaces(ctx, k, h, members, distinct, per, tag, lines):
    nss = namespace_queries(distinct, k, per, 100 * k + per)
    count = N * per
    rng = np.random.default_rng(per)
    order = rng.permutation(count) if per > 1 else np.arange(count)   # request i is grouped query order[i]
    squares = np.ascontiguousarray((order // per).astype(np.uint32))
    flat = np.ascontiguousarray(nss.reshape(count, 29)[order])
    plan = _lib.NamespacePlanT()
    ctx.check(ctx.lib.cda_square_set_namespace_plan(h, p32(squares), ptr(flat), count, C.byref(plan)))
    plan = {n: getattr(plan, n) for n, _ in _lib.NamespacePlanT._fields_}
    out1 = NamespaceProofsBatch.empty(k, flat, plan)
    o1 = out1.out_struct()

    def one_call():
        ctx.check(ctx.lib.cda_square_set_namespace_proofs(h, p32(squares), ptr(flat), count, C.byref(o1)))

    outs, calls = [], []
    for y, m in enumerate(members):
        q = np.ascontiguousarray(nss[y])
        p = _lib.NamespacePlanT()
        ctx.check(ctx.lib.cda_square_namespace_plan(m, ptr(q), per, C.byref(p)))
        b = NamespaceProofsBatch.empty(k, q, {n: getattr(p, n) for n, _ in _lib.NamespacePlanT._fields_})
        outs.append(b)
        calls.append((m, ptr(q), per, b.out_struct(), q))
    fn = ctx.lib.cda_square_namespace_proofs

    def per_member():
        for m, q, n, o, _ in calls:
            rc = fn(m, q, n, C.byref(o))
            if rc:
                ctx.check(rc)

    t1, t0 = timed(one_call), timed(per_member)
    # the same bytes: the grouped order through the set call once more, against the members' answers one behind the other
    g_sq = np.repeat(np.arange(N, dtype=np.uint32), per)
    g_ns = np.ascontiguousarray(nss.reshape(count, 29))
    grouped = NamespaceProofsBatch.empty(k, g_ns, plan)
    og = grouped.out_struct()
    ctx.check(ctx.lib.cda_square_set_namespace_proofs(h, p32(g_sq), ptr(g_ns), count, C.byref(og)))
    for name in ("row", "kind", "nmt_start", "nmt_end", "nodes", "shares", "absence_leaf"):
        assert np.array_equal(getattr(grouped, name), np.concatenate([getattr(b, name) for b in outs])), name
    nbytes = sum(a.nbytes for a in out1.arrays())
    report(lines, f"({tag}) k = {k}: {per} namespace(s) of each of {N} members ({count} queries, {plan['n_segments']} "
                  f"segments, {nbytes} bytes returned); warm-up {WARMUP}, {REPS} timed rounds", "query", count,
           [("1: one cda_square_set_namespace_proofs call", t1),
            (f"0: {N} cda_square_namespace_proofs calls on the members", t0)])
    return out1, squares, outs


def bench_verify(ctx, k, h, rows, set_batch, squares, outs, tag, lines):
    count = len(set_batch)
    b1 = set_batch.batch()
    v1 = np.full(count, 255, dtype=np.uint8)
    roots = np.ascontiguousarray(rows).reshape(-1)

    def one_call():
        ctx.check(ctx.lib.cda_namespace_proofs_verify_set(ctx.h, k, ptr(roots), N, p32(squares), C.byref(b1), ptr(v1)))

    calls = []
    for y, b in enumerate(outs):
        calls.append((ptr(np.ascontiguousarray(rows[y])), b.batch(), np.full(len(b), 255, dtype=np.uint8), rows[y]))
    fn = ctx.lib.cda_namespace_proofs_verify

    def per_member():
        for r, b, v, _ in calls:
            rc = fn(ctx.h, k, r, C.byref(b), ptr(v))
            if rc:
                ctx.check(rc)

    t1, t0 = timed(one_call), timed(per_member)
    assert not v1.any() and not any(v.any() for _, _, v, _ in calls), "an honest answer did not verify"
    report(lines, f"({tag}) k = {k}: verification of {count} answers against {N} DAHs "
                  f"({roots.nbytes} bytes of row roots); warm-up {WARMUP}, {REPS} timed rounds", "query", count,
           [("1: one cda_namespace_proofs_verify_set call", t1),
            (f"0: {N} cda_namespace_proofs_verify calls", t0)])


def bench_shares(ctx, k, h, members, lines):
    per = 16
    count = N * per
    rng = np.random.default_rng(7 * k)
    starts_g = rng.integers(0, k * k, (N, per)).astype(np.uint32)
    order = rng.permutation(count)
    squares = np.ascontiguousarray((order // per).astype(np.uint32))
    starts = np.ascontiguousarray(starts_g.reshape(-1)[order])
    ends = starts + 1
    out1 = ShareProofsBatch.empty(k, np.stack([starts, ends], axis=1))
    o1 = out1.out_struct()

    def one_call():
        ctx.check(ctx.lib.cda_square_set_share_proofs(h, p32(squares), p32(starts), p32(ends), count, C.byref(o1)))

    outs, calls = [], []
    for y, m in enumerate(members):
        s = np.ascontiguousarray(starts_g[y])
        e = s + 1
        b = ShareProofsBatch.empty(k, np.stack([s, e], axis=1))
        outs.append(b)
        calls.append((m, p32(s), p32(e), per, b.out_struct(), s, e))
    fn = ctx.lib.cda_square_share_proofs

    def per_member():
        for m, s, e, n, o, _, _ in calls:
            rc = fn(m, s, e, n, C.byref(o))
            if rc:
                ctx.check(rc)

    t1, t0 = timed(one_call), timed(per_member)
    for name in ("nodes", "row_roots", "rfc_leaf_hash", "aunts", "shares", "namespaces"):
        got = getattr(out1, name)
        per_item = len(got) // count
        want = np.concatenate([getattr(b, name) for b in outs]).reshape(count, per_item, -1)[order]
        assert np.array_equal(got.reshape(count, per_item, -1), want), name
    nbytes = sum(a.nbytes for a in out1.arrays())
    report(lines, f"(e) k = {k}: {per} single-share ranges of each of {N} members ({count} ranges, {nbytes} bytes "
                  f"returned); warm-up {WARMUP}, {REPS} timed rounds", "range", count,
           [("1: one cda_square_set_share_proofs call", t1),
            (f"0: {N} cda_square_share_proofs calls on the members", t0)])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "square_set_queries.txt")
    ctx = default_context()
    lines = [f"namespace and share-range proofs across a set of {N} resident squares on one GPU; "
             f"{ctx.lib.cda_version().decode()}",
             "wall time around calls that return with their work complete (host clock)", ""]
    for k in (128, 32):
        h, members, distinct = make_set(ctx, k)
        W = 2 * k
        rows = np.empty((N, W, 90), dtype=np.uint8)
        ctx.check(ctx.lib.cda_square_set_dah(h, ptr(rows), None, None, None))
        c = bench_namespaces(ctx, k, h, members, distinct, 1, "c", lines)
        d = bench_namespaces(ctx, k, h, members, distinct, 16, "d", lines)
        bench_shares(ctx, k, h, members, lines)
        bench_verify(ctx, k, h, rows, *c, "f", lines)
        bench_verify(ctx, k, h, rows, *d, "g", lines)
        ctx.lib.cda_square_set_destroy(h)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
