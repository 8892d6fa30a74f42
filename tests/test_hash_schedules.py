"""Every hash schedule the engine can choose for a batch, byte-checked.

csrc/hash_plan.h holds the launch schedule of the hashing half of
cda_extend_dah* as pure functions of (k, n, knob values); engine.hip and
nmt.hip call them, and tools/hash_plan_host_test.cpp prints the plan of every
part of every (k, n).  A *plan class* is k plus the ordered launches of a part
with the parameters that select a kernel form (hash_plan_tool.class_key).

CPU part: the classes of SWEEP (run on the GPU below) and ELSEWHERE (run by
other oracle-pinned GPU tests) cover every class the header can produce; plan
invariants hold for every (k, n); every A/B form of test_variants.py reaches
a plan the default schedule does not.

GPU part: one in-place device batch per SWEEP row, every square's EDS, packed
row / column roots and data root bit-exact against the C oracle (k = 128:
the committed oracle digests of tests/golden/config4_k128*.json), and the
push-order status and detail of a square with two Q0 namespaces swapped, whose
roots are the blind oracle's up to k = 128.

A changed threshold in hash_plan.h must come with a SWEEP row: the coverage
test names the (k, n) to add."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import guarded
import hash_plan_tool as hp

HERE = os.path.dirname(os.path.abspath(__file__))

needs_gxx = pytest.mark.skipif(not hp.HAVE_GXX, reason="g++ not available")

# (k, n) batches the GPU test below runs: for every class no ELSEWHERE test
# reaches, the smallest n that reaches it.
SWEEP = [
    (1, 17),
    (2, 17),
    (4, 17), (4, 513), (4, 1024),
    (8, 17), (8, 129), (8, 256), (8, 513), (8, 1024),
    (16, 17), (16, 64), (16, 129), (16, 257), (16, 512), (16, 513), (16, 1024),
    (32, 17), (32, 31), (32, 33), (32, 64), (32, 65), (32, 129), (32, 256), (32, 257), (32, 512), (32, 1024),
    (64, 5), (64, 7), (64, 9), (64, 17), (64, 33), (64, 63), (64, 64), (64, 65), (64, 128), (64, 129), (64, 256),
    (64, 512), (64, 1024),
    (128, 3), (128, 4), (128, 5), (128, 9), (128, 15), (128, 17), (128, 33),
    (256, 2), (256, 3), (256, 5), (256, 9), (256, 16), (256, 17), (256, 32), (256, 33), (256, 64),
    (512, 2), (512, 3), (512, 4), (512, 5), (512, 8), (512, 9), (512, 16), (512, 17),
]

# (k, n) batches that GPU tests pinned to the oracle (or to a committed oracle
# fixture) already run on the product library with the default knobs.
ELSEWHERE = [
    *[(k, 1, "test_gpu_parity.py::test_random_square_parity") for k in (1, 2, 4, 8, 16, 32, 64, 128)],
    *[(k, 1, "test_gpu_parity.py::test_gf16_square_parity") for k in (256, 512)],
    *[(128, n, "test_config4.py::test_inplace_batch_sizes_around_schedule_switches") for n in (1, 2, 7, 63, 64, 65)],
    (128, 128, "test_config4.py::test_config4_rank_shard_on_gpu"),
    (128, 256, "test_config4.py::test_config4_multi_gpu_shard_one_submission"),
    (128, 512, "test_config4.py::test_config4_multi_gpu_shard_one_submission"),
    (128, 1024, "test_config4.py::test_config4_all_1024_squares_one_submission"),
    (512, 32, "test_gpu_parity.py::test_k512_batch_of_32_matches_committed_oracle_digest"),
    (1024, 1, "test_k1024.py::test_one_square_three_entry_points"),
    *[(1024, n, "test_k1024.py::test_inplace_batch") for n in (2, 3, 4, 5, 8)],
]

# Classes no test can reach within the memory bound of a sweep case (at most
# 3, each named by hash_plan_tool.describe): none.
UNREACHED = []


def _classes(pairs, plans):
    return {hp.class_key(part) for kn in pairs for part in plans[kn]}


@needs_gxx
def test_elsewhere_names_existing_tests():
    for k, n, where in ELSEWHERE:
        path, name = where.split("::")
        with open(os.path.join(HERE, path)) as f:
            assert re.search(rf"^def {name}\(", f.read(), re.M), where


@needs_gxx
def test_every_plan_class_is_byte_checked():
    """SWEEP + ELSEWHERE reach every plan class of hash_plan.h (default
    knobs, k in 1 .. 1024, n in 1 .. 1024, <= 64 at k = 256, <= 32 at k = 512,
    <= 8 at k = 1024).
    An uncovered class fails with the smallest (k, n) that reaches it: the
    SWEEP row to add."""
    plans = hp.plans()
    assert sorted({k for k, _ in plans}) == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
    assert len(plans) == 8 * 1024 + 64 + 32 + 8
    first = {}
    for (k, n), parts in sorted(plans.items()):
        for part in parts:
            first.setdefault(hp.class_key(part), (k, n))
    elsewhere = _classes([(k, n) for k, n, _ in ELSEWHERE], plans)
    sweep = _classes(SWEEP, plans)
    print(f"\nhash_plan.h plan classes: {len(first)}; reached by ELSEWHERE: {len(elsewhere)}; "
          f"added by SWEEP: {len(sweep - elsewhere)}")
    assert len(UNREACHED) <= 3 and set(UNREACHED) <= {hp.describe(c) for c in first}
    missing = sorted((kn, hp.describe(c)) for c, kn in first.items()
                     if c not in elsewhere and c not in sweep and hp.describe(c) not in UNREACHED)
    assert not missing, "plan classes no GPU test runs; add these (k, n) to SWEEP:\n" + "\n".join(
        f"  {kn}: {text}" for kn, text in missing)
    # every SWEEP row earns its GPU time: it reaches a class ELSEWHERE does not
    idle = [kn for kn in SWEEP if _classes([kn], plans) <= elsewhere]
    assert not idle, idle
    assert len(set(SWEEP)) == len(SWEEP)


@needs_gxx
def test_plan_invariants():
    plans = hp.plans()
    for (k, n), parts in plans.items():
        W = 2 * k
        # the parts of a split partition [0, n)
        assert [p.p for p in parts] == list(range(len(parts))) and len(parts) == parts[0].parts, (k, n)
        assert parts[0].i0 == 0 and parts[-1].i0 + parts[-1].m == n, (k, n)
        for a, b in zip(parts, parts[1:]):
            assert a.i0 + a.m == b.i0, (k, n)
        assert len(parts) == (2 if n < 64 and k <= 128 and n > 1 else 1), (k, n)
        for part in parts:
            assert part.m >= 1 and part.room == W * W * 96 // 2, (k, n)
            ls = [l for l in part.launches if l.kernel != "rs8"]
            assert [l.kernel for l in part.launches if l.kernel == "rs8"] == (["rs8"] * 2 if k == 128 else [])
            assert ls[0].kernel in ("leaf", "leaf_pair") and ls[0].n_in == W, (k, n)
            assert (ls[0].kernel == "leaf_pair") == (W * W * part.m <= 32768), (k, n)
            assert ls[-1].kernel == "data_root" and [l.kernel for l in ls].count("data_root") == 1, (k, n)
            # every tree level from W down to 1 runs exactly once, in one of
            # the subtree launch, the level launches and the tree top
            cur, tops, n_dig = W, 0, 2 * W
            for l in ls[1:-1]:
                if l.kernel == "subtree":
                    assert l.n_in == cur and cur == W and 1 <= l.sub < cur and cur % l.sub == 0, (k, n, l)
                    depth = (cur // l.sub).bit_length() - 1
                    assert cur // l.sub >= 8 and 1 << depth == cur // l.sub, (k, n, l)
                    # roots and per-lane stacks fit the forest's output region
                    assert l.scratch == W * l.sub * depth * 96 and l.scratch <= part.room, (k, n, l)
                    assert W % 64 == 0, (k, n)
                    cur = l.sub
                elif l.kernel == "level":
                    assert l.n_in == cur and cur >= 2, (k, n, l)
                    cur //= 2
                elif l.kernel == "tree_top":
                    assert l.n_in == cur and (8 if l.wide else 2) <= cur <= (512 if l.wide else 256), (k, n, l)
                    tpw = (512 if l.wide else 256) // cur
                    assert l.sub == tpw and l.n_dig << l.lv == 2 * W and l.n_dig >= 2, (k, n, l)
                    assert l.lv == 0 or tpw <= 2 * W, (k, n, l)
                    assert l.ragged == (2 * W % tpw != 0), (k, n, l)
                    assert not l.ragged or l.lv == 0, (k, n, l)   # RFC levels only over whole workgroups
                    assert l.pair or not l.wide, (k, n, l)
                    assert l.pair == (l.wide or 2 * part.m * 2 * W * (cur // 2) <= 65536), (k, n, l)
                    cur, tops, n_dig = 1, tops + 1, l.n_dig
                else:
                    assert l.kernel == "rfc_leaf" and cur == 1 and tops == 0, (k, n, l)
            assert cur == 1 and tops <= 1, (k, n)
            assert ("rfc_leaf" in [l.kernel for l in ls]) == (tops == 0), (k, n)
            dr = ls[-1]
            assert dr.n_dig == n_dig and dr.pmax == (256 if part.m <= 8 else 128) and dr.mode == 2, (k, n)
            assert dr.threads % 64 == 0 and min(n_dig // 2, 512) <= dr.threads <= 512, (k, n, dr)
            assert dr.threads >= min(n_dig, 2 * dr.pmax), (k, n, dr)


@needs_gxx
@pytest.mark.parametrize("env", hp.VARIANT_ENVS, ids=lambda e: "-".join(f"{a}={b}" for a, b in e.items()))
def test_variant_reaches_a_plan_the_default_does_not(env):
    """The (k, n) list of test_variants.py's A/B children, planned with the
    child's knob values, holds a plan class the default schedule does not
    give that list -- and one it gives no (k, n) at all, except for
    CDA_SUBTREE=0: per-level launches in place of the subtree launch of
    128 x 16 are also what the default runs where a part is too small for a
    subtree launch (k = 128, n = 9 .. 15), so that child re-checks a default
    class at another batch size."""
    forced = hp.plans(hp.env_knobs(env))
    reached = _classes(hp.VARIANT_CASES, forced)
    assert reached - _classes(hp.VARIANT_CASES, hp.plans()), env
    default = {hp.class_key(part) for parts in hp.plans().values() for part in parts}
    assert bool(reached - default) == (env != {"CDA_SUBTREE": "0"}), env


# ---------------------------------------------------------------------------
# GPU sweep
# ---------------------------------------------------------------------------
_expect = {"k": None}


def _distinct(k, n):
    return min(n, 7 if k <= 128 else 3)


def _first_violation(q0):
    """Brute-force nmt push-order check of one Q0 (k x k x 512): the smallest
    (axis, index, position) whose namespace is below its predecessor's (rows
    before columns), as cda_push_order_detail_at reports."""
    k = q0.shape[0]
    ns = [[q0[r, c, :29].tobytes() for c in range(k)] for r in range(k)]
    for r in range(k):
        for c in range(1, k):
            if ns[r][c] < ns[r][c - 1]:
                return (0, r, c)
    for c in range(k):
        for r in range(1, k):
            if ns[r][c] < ns[r - 1][c]:
                return (1, c, r)
    return None


def _swapped(k):
    """Distinct square 2 with two adjacent, different Q0 namespaces of one row
    swapped, and the first violation that leaves."""
    from celestia_da import testfactory
    q0 = testfactory.random_square(k, 2).reshape(k, k, 512).copy()
    r = min(2, k - 1)
    c = next(c for c in range(k - 1) if q0[r, c, :29].tobytes() != q0[r, c + 1, :29].tobytes())
    q0[r, c, :29], q0[r, c + 1, :29] = q0[r, c + 1, :29].copy(), q0[r, c, :29].copy()
    want = _first_violation(q0)
    assert want is not None and want <= (0, r, c + 1)
    return q0, want


def _expected(k, j, bad):
    """Oracle outputs of distinct square j of width k (cached for the k in
    hand): (ods, eds, rows, cols, root, detail); a digest dict instead of the
    bytes at k = 128; for the swapped square, whose honest roots the oracle
    refuses, the blind oracle's rows, cols and root over coracle.extend's EDS
    up to k = 128, and None above."""
    import coracle
    from celestia_da import testfactory
    if _expect["k"] != k:
        _expect.clear()
        _expect["k"] = k
    key = (j, bad)
    if key in _expect:
        return _expect[key]
    if bad:
        q0, want = _swapped(k)
        ods = q0.reshape(k * k, 512)
        eds = coracle.extend(ods) if k <= 128 else None
        if k <= 32:   # the oracle's own push-order verdict names the same axis and index
            with pytest.raises(coracle.PushOrderError, match=f"{'col' if want[0] else 'row'} {want[1]}$"):
                coracle.roots(eds, k)
        # its roots are the blind ones (BlindTree: the hashing without the order check)
        rows, cols, root = coracle.blind_dah(eds, k, 16 if k >= 64 else 0) if k <= 128 else (None, None, None)
        out = (ods, eds, rows, cols, root, want)
    else:
        ods = testfactory.random_square(k, j)
        if k == 128:
            g = _fixture_k128()[str(j)]
            assert hashlib.sha256(np.ascontiguousarray(ods).tobytes()).hexdigest() == g["ods_sha256"]
            out = (ods, g, None, None, bytes.fromhex(g["data_root"]), (-1, 0, 0))
        else:
            eds, rows, cols, root = coracle.cpu_baseline(ods, 16) if k >= 64 else coracle.extend_dah(ods)
            out = (ods, eds, rows, cols, root, (-1, 0, 0))
    _expect[key] = out
    return out


def _fixture_k128():
    if "g128" not in _expect:
        with open(os.path.join(HERE, "golden", "config4_k128.json")) as f:
            g = json.load(f)["squares"]
        with open(os.path.join(HERE, "golden", "config4_k128_rest.json")) as f:
            g.update(json.load(f)["squares"])
        _expect["g128"] = g
    return _expect["g128"]


def _sha(t) -> str:
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", SWEEP)
def test_sweep_batch_matches_oracle(ctx, k, n):
    """One in-place device batch of n squares of width k on the product
    library: square i holds distinct square i % d (d = 7, or 3 for k >= 256:
    an odd period, so a square stride wrong by a power of two never lands on
    an equal square).  Every square's EDS, row roots, column roots and data
    root equal the oracle's, compared on the device; for n >= 4 distinct
    square 2 carries a push-order violation and exactly its copies report
    CDA_ERR_PUSH_ORDER with the brute-force detail (and, up to k = 128, the
    blind oracle's roots and data root)."""
    import torch
    W = 2 * k
    d = _distinct(k, n)
    bad_j = 2 if n >= 4 and k >= 2 else None
    dev = torch.device("cuda", 0)
    exp = [_expected(k, j, j == bad_j) for j in range(d)]
    eds = rows = cols = roots = status = guards = None
    try:
        eds = torch.zeros((n, W, W, 512), dtype=torch.uint8, device=dev)
        for j in range(d):
            eds[j::d, :k, :k] = torch.from_numpy(exp[j][0]).to(dev).view(k, k, 512)
        # The kernel that stores the packed roots, the data roots and the
        # status words depends on the plan class, so these four lie in guarded
        # buffers (tests/guarded.py), each at exactly its documented minimum
        # alignment: an unwritten byte still holds the pattern and fails the
        # comparisons below, a store next to a buffer fails its guards.
        guards = [guarded.alloc(n * W * 90, stride=W * 90, align=2, backend="torch", name="d_row_roots"),
                  guarded.alloc(n * W * 90, stride=W * 90, align=2, backend="torch", name="d_col_roots"),
                  guarded.alloc(n * 32, stride=32, align=4, backend="torch", name="d_data_roots"),
                  guarded.alloc(n * 4, stride=4, align=4, backend="torch", name="d_status")]
        rows, cols = guards[0].payload().view(n, W * 90), guards[1].payload().view(n, W * 90)
        roots, status = guards[2].payload().view(n, 32), guards[3].payload().view(torch.int32)
        ctx.extend_dah_inplace_device(k, n, eds.data_ptr(), *[g.ptr for g in guards],
                                      torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()

        def check(which, got, want, j):
            """got[j::d] (device) against `want` (one square's bytes)."""
            w = torch.from_numpy(np.ascontiguousarray(want).reshape(-1)).to(dev)
            g = got[j::d].reshape(-1, w.numel())
            if bool((g == w).all()):
                return
            for p in range(g.shape[0]):   # name the first square that differs
                if not torch.equal(g[p], w):
                    off = int((g[p] != w).nonzero()[0])
                    pytest.fail(f"k={k} n={n} square i={j + p * d} (distinct {j}): {which} differs from the oracle "
                                f"at byte {off}: got {g[p][off:off + 8].cpu().tolist()} want "
                                f"{w[off:off + 8].cpu().tolist()}")

        for j in range(d):
            ods, e_eds, e_rows, e_cols, e_root, _ = exp[j]
            if k == 128 and j != bad_j:
                # committed oracle digests for the first copy, device equality for the rest
                assert _sha(eds[j]) == e_eds["eds_sha256"], f"k={k} n={n} i={j}: EDS"
                assert _sha(rows[j]) == e_eds["row_roots_sha256"], f"k={k} n={n} i={j}: row roots"
                assert _sha(cols[j]) == e_eds["col_roots_sha256"], f"k={k} n={n} i={j}: column roots"
                check("EDS", eds, eds[j].cpu().numpy(), j)
                check("row roots", rows, rows[j].cpu().numpy(), j)
                check("column roots", cols, cols[j].cpu().numpy(), j)
            else:
                if e_eds is not None:
                    check("EDS", eds, e_eds, j)
                if e_rows is not None:
                    check("row roots", rows, e_rows, j)
                    check("column roots", cols, e_cols, j)
            if e_root is not None:
                check("data root", roots, np.frombuffer(e_root, dtype=np.uint8).copy(), j)
        st = status.cpu().tolist()
        want_st = [-3 if bad_j is not None and i % d == bad_j else 0 for i in range(n)]   # CDA_ERR_PUSH_ORDER
        assert st == want_st, f"k={k} n={n}: status differs first at i={[a == b for a, b in zip(st, want_st)].index(False)}"
        if bad_j is not None:
            bad_i = [i for i in range(n) if i % d == bad_j]
            for i in (bad_i[0], bad_i[-1]):
                assert ctx.push_order_detail_at(i) == exp[bad_j][5], f"k={k} n={n} i={i}: push-order detail"
        assert ctx.push_order_detail_at(0) == (-1, 0, 0) and ctx.push_order_detail_at(n - 1) == (
            exp[(n - 1) % d][5]), f"k={k} n={n}: push-order detail of the first / last square"
        for g in guards:
            g.assert_guards(f"k={k} n={n} {g.name}")
    finally:
        del eds, rows, cols, roots, status, guards
        torch.cuda.empty_cache()
