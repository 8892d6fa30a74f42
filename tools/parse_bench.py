#!/usr/bin/env python3
"""Parsing a resident k = 128 square back into transactions and blobs on one
GPU.  A measurement, not a gate: no target was fixed in advance.

Four squares of 16 384 shares:
  full_block   celestia_da.blobfactory.full_block through square.construct;
  one_blob     the whole square one blob of 478 + 16 383 * 482 bytes;
  one_share    4 096 blobs of one share each (lengths 1..478), then tail padding;
  get_all      256 namespaces of 15 three-share blobs and one one-share blob each,
               a query for 64 of them: the ranges blob.get_all parses.
For each:
  (a) cda_square_parse, every output into host buffers of the plan's sizes;
  (b) cda_square_parse with blob_data NULL: the table, the units and the blobs'
      positions, no blob bytes (what blob.get asks for before it gathers its match);
  (c) cda_square_parse_plan alone;
  (d) the yardstick, cda_shares_parse on a host copy of the same original square
      (for get_all: of the ranges' shares, concatenated once outside the clock);
  (e) (d) plus the time to copy Q0 back from the device first (a device tensor of
      the 8 MiB original square to pageable host memory).
The timed region is the C call alone, buffers allocated once, copies and
synchronisations included.  Wall time, WARMUP calls first, then REPS timed
calls; median, min and max.

The gather kernel's own time comes from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/parse_bench.py --trace
runs (a) TRACE_CALLS times per square (two launches of gather_kernel each: headers, payload), and
    python tools/parse_bench.py --summarise DIR profiles/parse.txt
appends the kernels' times per square, in dispatch order, to the report.

Writes profiles/parse.txt (or argv[1]).
"""
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("celestia-app_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402

K = 128
N = K * K
WARMUP = int(os.environ.get("WARMUP", "3"))
REPS = int(os.environ.get("REPS", "20"))
TRACE_CALLS = 5
CASES = ("full_block", "one_blob", "one_share", "get_all")
U32P = C.POINTER(C.c_uint32)


def timed(call, warmup=WARMUP, reps=REPS):
    times = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return times


def blob_ns(i: int) -> bytes:
    return bytes(19) + b"\x01" + i.to_bytes(9, "big")


def sparse(ns: bytes, data: np.ndarray) -> np.ndarray:
    """The sparse shares of one blob, as an (n, 512) array."""
    L = len(data)
    n = 1 if L <= 478 else 1 + -(-(L - 478) // 482)
    out = np.zeros((n, 512), dtype=np.uint8)
    out[:, :29] = np.frombuffer(ns, dtype=np.uint8)
    out[0, 29] = 1
    out[0, 30:34] = np.frombuffer(L.to_bytes(4, "big"), dtype=np.uint8)
    out[0, 34:34 + min(L, 478)] = data[:478]
    if n > 1:
        rest = np.zeros((n - 1) * 482, dtype=np.uint8)
        rest[:L - 478] = data[478:]
        out[1:, 30:] = rest.reshape(n - 1, 482)
    return out


def tail(n: int) -> np.ndarray:
    out = np.zeros((n, 512), dtype=np.uint8)
    out[:, :28] = 0xFF
    out[:, 28] = 0xFE
    out[:, 29] = 1
    return out


def make_square(case: str, ctx):
    """(the original square as an (N, 512) array, the ranges to parse or None)."""
    from celestia_da import blobfactory, square
    rng = np.random.default_rng(7)
    if case == "full_block":
        sq = square.construct(blobfactory.full_block(1, K), K, 64, ctx=ctx)
        ods = np.frombuffer(sq.to_bytes(), dtype=np.uint8).reshape(-1, 512)
        assert ods.shape[0] == N, ods.shape
        return ods.copy(), None
    if case == "one_blob":
        return sparse(blob_ns(1), rng.integers(0, 256, 478 + (N - 1) * 482, dtype=np.uint8)), None
    if case == "one_share":
        parts = [sparse(blob_ns(1 + i), rng.integers(0, 256, 1 + (i * 37) % 478, dtype=np.uint8)) for i in range(4096)]
        return np.concatenate(parts + [tail(N - 4096)]), None
    parts = []
    for i in range(256):
        for j in range(15):
            parts.append(sparse(blob_ns(1 + i), rng.integers(0, 256, 961 + (i + j) % 480, dtype=np.uint8)))
        parts.append(sparse(blob_ns(1 + i), rng.integers(0, 256, 1 + i, dtype=np.uint8)))
    ods = np.concatenate(parts + [tail(N - 256 * 46)])
    return ods, "query"


def square_ranges(case, sq):
    from celestia_da import blob
    if case != "get_all":
        return None
    return blob.namespace_ranges(sq, [blob_ns(1 + 4 * i) for i in range(64)])


def range_args(ranges):
    if ranges is None:
        return None, None, 0, None
    r = np.array(ranges, dtype=np.uint32).reshape(-1, 2)
    st, en = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    return st.ctypes.data_as(U32P), en.ctypes.data_as(U32P), len(r), (st, en)


def bench_case(case, ctx, torch):
    from celestia_da import _lib, proof, shares
    ods, _ = make_square(case, ctx)
    sq = proof.ResidentSquare(ods, ctx)
    ranges = square_ranges(case, sq)
    st, en, n, keep = range_args(ranges)
    lib = ctx.lib
    plan = _lib.ParsePlanT()

    def plan_call():
        ctx.check(lib.cda_square_parse_plan(sq.h, st, en, n, C.byref(plan)))
    t_c = timed(plan_call)
    buf = shares.ParseBuffers(plan)
    o = buf.out_struct()

    def parse_call():
        ctx.check(lib.cda_square_parse(sq.h, st, en, n, C.byref(o)))
    t_a = timed(parse_call)
    tbuf = shares.ParseBuffers(plan, blob_data=False)
    to = tbuf.out_struct()

    def table_call():
        ctx.check(lib.cda_square_parse(sq.h, st, en, n, C.byref(to)))
    t_b = timed(table_call)
    assert np.array_equal(tbuf.blob_off, buf.blob_off) and np.array_equal(tbuf.unit_data, buf.unit_data)

    # the yardstick: the host-only call on the same shares
    host = ods if ranges is None else np.concatenate([ods[s:e] for s, e in ranges])
    hplan = _lib.ParsePlanT()
    assert lib.cda_shares_parse_plan(_lib.ptr(host), host.shape[0], C.byref(hplan)) == 0
    assert (hplan.blob_bytes, hplan.unit_bytes, hplan.n_blobs) == (plan.blob_bytes, plan.unit_bytes, plan.n_blobs)
    hbuf = shares.ParseBuffers(hplan)
    ho = hbuf.out_struct()

    def host_call():
        assert lib.cda_shares_parse(_lib.ptr(host), host.shape[0], C.byref(ho)) == 0
    t_d = timed(host_call)
    assert np.array_equal(hbuf.blob_data, buf.blob_data) and np.array_equal(hbuf.unit_data, buf.unit_data)
    d_ods = torch.from_numpy(ods.reshape(-1)).to("cuda")
    torch.cuda.synchronize()
    back = np.empty(ods.size, dtype=np.uint8)
    back_t = torch.from_numpy(back)

    def copy_and_host_call():
        back_t.copy_(d_ods)
        torch.cuda.synchronize()
        host_call()
    t_e = timed(copy_and_host_call)
    sizes = dict(shares=host.shape[0], blobs=plan.n_blobs, txs=plan.n_txs, pfbs=plan.n_pfbs,
                 padding=plan.n_padding_shares, blob_bytes=plan.blob_bytes, unit_bytes=plan.unit_bytes,
                 ranges=0 if ranges is None else len(ranges))
    sq.close()
    return sizes, dict(a=t_a, b=t_b, c=t_c, d=t_d, e=t_e)


def report(out_path):
    import torch
    from celestia_da import default_context
    ctx = default_context()
    lines = [f"parsing one resident k = {K} square back into transactions and blobs; {ctx.lib.cda_version().decode()}",
             f"wall time around the synchronised C call (host buffers allocated once); warm-up {WARMUP}, {REPS} timed calls",
             "a cda_square_parse   b cda_square_parse without blob bytes   c cda_square_parse_plan   d cda_shares_parse (host "
             "yardstick)   e d + Q0 copied back first", ""]
    for case in CASES:
        sizes, t = bench_case(case, ctx, torch)
        lines.append(f"{case}: " + "  ".join(f"{k_} {v}" for k_, v in sizes.items()))
        med = {}
        for key in "abcde":
            med[key] = statistics.median(t[key])
            lines.append(f"  {key}: ms per call: median {med[key] * 1e3:.3f}  min {min(t[key]) * 1e3:.3f}  "
                         f"max {max(t[key]) * 1e3:.3f}")
        moved = sizes["blob_bytes"] + sizes["unit_bytes"]
        lines.append(f"  (d) / (a) = {med['d'] / med['a']:.2f}   (e) / (a) = {med['e'] / med['a']:.2f}   "
                     f"(d) / (b) = {med['d'] / med['b']:.2f}   (e) / (b) = {med['e'] / med['b']:.2f}   "
                     f"payload {moved / 1e6:.2f} MB: (a) {moved / med['a'] / 1e9:.2f} GB/s, (d) {moved / med['d'] / 1e9:.2f} GB/s")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


def trace():
    """TRACE_CALLS cda_square_parse calls per square, for a kernel trace: two gather_kernel launches each."""
    from celestia_da import _lib, default_context, proof, shares
    ctx = default_context()
    for case in CASES:
        ods, _ = make_square(case, ctx)
        sq = proof.ResidentSquare(ods, ctx)
        st, en, n, keep = range_args(square_ranges(case, sq))
        plan = _lib.ParsePlanT()
        ctx.check(ctx.lib.cda_square_parse_plan(sq.h, st, en, n, C.byref(plan)))
        o = shares.ParseBuffers(plan)
        os_ = o.out_struct()
        for _ in range(TRACE_CALLS):
            ctx.check(ctx.lib.cda_square_parse(sq.h, st, en, n, C.byref(os_)))
        sq.close()


def summarise(trace_dir, out_path):
    """Per square, the durations of the two gather_kernel dispatches (headers, then payload) of the trace's
    cda_square_parse calls: the last 2 * TRACE_CALLS gather dispatches before the next square is created."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    rows = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
    # a square's run ends where the next square's extension (or the trace) begins: cut at the RS kernels
    runs, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "gather_kernel" in name and "gen_gather" not in name:
            if cur is None:
                cur = []
                runs.append(cur)
            cur.append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Grid_Size_X"])))
        elif "rs8" in name or "rs16" in name:
            cur = None
    assert len(runs) == len(CASES), [len(x) for x in runs]
    lines = ["", f"kernel times (rocprofv3 --kernel-trace, a run of its own; {TRACE_CALLS} cda_square_parse calls per square, "
                 "median; us)"]
    for case, run in zip(CASES, runs):
        # the plan call: a headers launch, and a payload launch when the square has compact sequences; then
        # TRACE_CALLS parse calls of two launches each -- any other gather_kernel launch is an error here
        assert len(run) in (2 * TRACE_CALLS + 1, 2 * TRACE_CALLS + 2), (case, len(run))
        mine = run[-2 * TRACE_CALLS:]
        headers, payload = mine[0::2], mine[1::2]
        assert len({g for _, g in headers}) == 1 and len({g for _, g in payload}) == 1, (case, mine)
        if case != "get_all":   # one 40-byte piece per share of the whole square, four pieces per workgroup
            assert headers[0][1] == (N + 3) // 4 * 256, (case, headers[0][1])
        lines.append(f"  {case}: gather_kernel, headers {statistics.median(t for t, _ in headers):.1f}   "
                     f"gather_kernel, payload {statistics.median(t for t, _ in payload):.1f}")
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
        report(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parse.txt"))
