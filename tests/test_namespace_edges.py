"""Edge namespaces and blind roots through every node-hashing kernel form.

The squares of tests/nmt_edge_squares.py -- runs of equal namespaces,
namespaces that differ only in byte 28 or only in byte 0, tail padding, Q0
shares that carry the parity namespace FF*29, and unordered squares whose
blind trees (test/util/malicious: BlindTree + the hasher's computeNsRange)
have left children with min = FF*29 and max below it -- run through
cda_extend_dah's hashing half in every kernel form csrc/hash_plan.h can pick:
leaf_pair, leaf, level, subtree, and tree_top in pair, wide and plain form.

CPU part: the blind entry point of the C oracle is pinned to pyref's BlindTree
restatement and pyref.nmt_hash_node to three nodes written out with hashlib;
both oracles accept the ordered families and refuse the unordered ones at the
brute-force first violation; the P-left square of every width in TABLE has the
nodes that make the GPU comparison able to fail; TABLE reaches every form.

GPU part: one in-place device batch per TABLE row, edge squares with the
oracle's random squares in between, every square's EDS, row roots, column
roots and data root against the oracle (the blind oracle for the unordered
ones), status and push-order detail; and once more through the A/B forms of
the test build that move levels between level, subtree and tree_top.

The CPU oracle takes under a second for a k = 512 square on 8 cores, so the
expected values of the k = 256 and k = 512 rows are computed here like the
others, not read from a fixture.
"""
import hashlib

import numpy as np
import pytest

import hash_plan_tool as hp
import nmt_edge_squares as es

needs_gxx = pytest.mark.skipif(not hp.HAVE_GXX, reason="g++ not available")

CDA_ERR_PUSH_ORDER = -3

# (k, n) batches of the GPU test.  From hash_plan_tool.plans() with the
# default knobs: the smallest batches whose plan has a level launch over
# inner nodes (n_in <= W/2) are (16, 257), (32, 65), (64, 17), (128, 5) and
# (256, 2), the smallest with a subtree launch (32, 129), (64, 63), (128, 15),
# (256, 3) and (512, 1); (4, 1), (16, 1), (16, 21) and (32, 21) hash every
# inner node in tree_top (after leaf_pair, or leaf at k = 32) and hold the
# whole list of edge squares at n = 21.
TABLE = [(4, 1), (16, 1), (16, 21), (32, 21),
         (16, 257), (32, 65), (64, 17), (256, 2),
         (32, 129), (64, 63), (128, 15), (256, 3), (512, 1)]
TABLE_KS = sorted({k for k, _ in TABLE})

# One (k, n) of hash_plan_tool.VARIANT_CASES per A/B form that moves tree
# levels between level, subtree and tree_top: where the forced plan differs.
AB_CASES = [({"CDA_SUBTREE": "0"}, (128, 16)),
            ({"CDA_TOP_FUSE": "0"}, (64, 9)),
            ({"CDA_LEAF_PAIR_MAX": "0"}, (32, 3)),
            ({"CDA_TOP_PAIR": "0"}, (128, 2))]

CPU_KS = (2, 4, 16)


def _forms(parts) -> set:
    out = set()
    for part in parts:
        W = 2 * part.k
        for l in part.launches:
            if l.kernel in ("leaf", "leaf_pair"):
                out.add(l.kernel)
            elif l.kernel == "level":
                out.add("level over inner nodes" if l.n_in <= W // 2 else "level over leaves")
            elif l.kernel == "subtree":
                out.add("subtree n_in=1024" if l.n_in == 1024 else "subtree n_in<1024")
            elif l.kernel == "tree_top":
                out.add("tree_top wide" if l.wide else "tree_top pair" if l.pair else "tree_top non-pair")
    return out


# ---------------------------------------------------------------------------
# CPU: the oracle
# ---------------------------------------------------------------------------
def _pin_nmt_hash_node():
    """pyref.nmt_hash_node against computeNsRange restated here (min from the
    left child; max from the right child, or from the left one if the right
    min is FF*29): the right child a parity node, the left child a blind node
    with min = FF*29 > max, and an ordinary pair."""
    import pyref
    P, X, Y, Z = es.PARITY, es.ns_a(1), es.ns_a(2), es.TAIL_PADDING
    d = [hashlib.sha256(bytes([i])).digest() for i in range(4)]
    cases = [((X + Y + d[0], P + P + d[1]), X + Y),      # right min = FF*29: the parent takes the left max
             ((P + X + d[2], Y + Z + d[3]), P + Z),      # left min = FF*29, left max = X != FF*29
             ((X + X + d[0], Y + Z + d[1]), X + Z)]
    for (left, right), ns_range in cases:
        want = ns_range + hashlib.sha256(b"\x01" + left + right).digest()
        assert pyref.nmt_hash_node(left, right) == want
    # and on the C oracle's node hash
    import ctypes as C
    import coracle
    for (left, right), ns_range in cases:
        out = (C.c_uint8 * 90)()
        coracle.lib().oracle_hash_node((C.c_uint8 * 90)(*left), (C.c_uint8 * 90)(*right), out)
        assert bytes(out) == ns_range + hashlib.sha256(b"\x01" + left + right).digest()


@pytest.mark.parametrize("k", CPU_KS)
def test_blind_oracle_matches_pyref(k):
    """coracle.blind_dah / blind_extend_dah (scalar and threaded) against
    pyref.dah_from_eds(..., blind=True) on every edge square, ordered or not;
    on the ordered ones the blind roots are the honest ones.  First the node
    hash of both on three hand-written pairs (_pin_nmt_hash_node)."""
    import coracle
    import pyref
    _pin_nmt_hash_node()   # the node rule both restatements share, on nodes written out by hand
    W = 2 * k
    for name, (_, ordered) in es.SQUARES.items():
        ods = es.square(name, k).reshape(k * k, 512)
        eds = coracle.extend(ods)
        rows, cols, root = coracle.blind_dah(eds, k)
        p_rows, p_cols, p_root = pyref.dah_from_eds(eds.reshape(W, W, 512), blind=True)
        assert rows.tobytes() == b"".join(p_rows), (k, name)
        assert cols.tobytes() == b"".join(p_cols), (k, name)
        assert root == p_root, (k, name)
        for threads in (0, 3):
            e2, r2, c2, root2 = coracle.blind_extend_dah(ods, threads)
            assert np.array_equal(e2, eds) and np.array_equal(r2, rows) and np.array_equal(c2, cols), (k, name)
            assert root2 == root, (k, name)
        r3, c3, root3 = coracle.blind_dah(eds, k, 3)
        assert np.array_equal(r3, rows) and np.array_equal(c3, cols) and root3 == root, (k, name)
        if ordered:
            _, h_rows, h_cols, h_root = coracle.extend_dah(ods)
            assert np.array_equal(h_rows, rows) and np.array_equal(h_cols, cols) and h_root == root, (k, name)


# ---------------------------------------------------------------------------
# CPU: the families
# ---------------------------------------------------------------------------
def test_ladder_holds_every_rung():
    for k in (4, 16, 128):
        assert sorted(set(es.ladder_ranks(k).reshape(-1).tolist())) == list(range(10)), k
        rank = es.ladder_ranks(k)
        ends = rank[:, -1] == 9, rank[-1, :] == 9
        for e in ends:   # some rows / columns end in a run of parity-namespaced Q0 shares, others do not
            assert e.any() and not e.all(), k
    for k in TABLE_KS:   # P-left: at least a quarter of the cells are FF*29
        assert (es.ladder_rank_of(es.square("p_left", k)) == 9).sum() * 4 >= k * k, k


@pytest.mark.parametrize("k", sorted(set(CPU_KS) | {k for k in TABLE_KS if k <= 128}))
def test_ordered_families_accepted(k):
    """Every ordered square is non-decreasing along rows and columns and the
    oracles accept it: coracle at every width, pyref (equal to it) at k <=
    16."""
    import coracle
    import pyref
    for name in es.ORDERED:
        q0 = es.square(name, k)
        assert q0.shape == (k, k, 512) and q0.dtype == np.uint8
        assert np.array_equal(q0, es.square(name, k)), (k, name)   # deterministic
        assert es.descents(q0) == [], (k, name)
        eds, rows, cols, root = coracle.cpu_baseline(q0, 8) if k >= 64 else coracle.extend_dah(q0)
        if k <= 16:
            p_eds, p_rows, p_cols, p_root = pyref.extend_and_dah(q0)
            assert np.array_equal(p_eds.reshape(-1, 512), eds), (k, name)
            assert b"".join(p_rows) == rows.tobytes() and b"".join(p_cols) == cols.tobytes(), (k, name)
            assert p_root == root, (k, name)


def test_byte29_trap_descends_below_the_namespace():
    for k in (4, 16, 128, 512):
        q0 = es.byte29_trap(k)
        tail = q0[:, :, 29].astype(np.int64) << 16 | q0[:, :, 30].astype(np.int64) << 8 | q0[:, :, 31]
        assert (np.diff(tail, axis=0) < 0).all() and (np.diff(tail, axis=1) < 0).all(), k
        ns = q0[:, :, :29]
        same = (ns[:, 1:] == ns[:, :-1]).all(axis=2)
        only28 = (ns[:, 1:, :28] == ns[:, :-1, :28]).all(axis=2) & ~same
        assert same.sum() >= k * (k - 1) // 2 and only28.any(), k   # runs: at least half the row neighbours


@pytest.mark.parametrize("k", sorted(set(CPU_KS) | {k for k in TABLE_KS if k <= 128}))
def test_unordered_families_refused(k):
    """Both oracles refuse every unordered square, at the brute-force first
    violation; a byte-28 descent square has exactly one descending pair, in
    byte 28 alone, the `last` ones on the last Q0 position."""
    import coracle
    import pyref
    import test_hash_schedules as sweep
    W = 2 * k
    for name in es.UNORDERED:
        q0 = es.square(name, k)
        assert np.array_equal(q0, es.square(name, k)), (k, name)
        d = es.descents(q0)
        want = es.first_violation(q0)
        assert d and want == min(d)[:3] == sweep._first_violation(q0), (k, name)
        if name.startswith("descent"):
            axis = 1 if "col" in name else 0
            assert len(d) == 1 and d[0][0] == axis and d[0][3] == 28, (k, name, d)
            if name.endswith("last"):
                assert d[0][2] == k - 1, (k, name, d)
        if k <= 16:
            with pytest.raises(coracle.PushOrderError):
                coracle.extend_dah(q0)
        eds = coracle.extend(q0.reshape(k * k, 512))
        with pytest.raises(coracle.PushOrderError, match=f"{'col' if want[0] else 'row'} {want[1]}$"):
            coracle.roots(eds, k)
        if k <= 16:
            g = q0 if want[0] == 0 else q0.transpose(1, 0, 2)
            last, pushed = g[want[1], want[2] - 1, :29].tobytes(), g[want[1], want[2], :29].tobytes()
            with pytest.raises(pyref.PushOrderError, match=f"last namespace: {last.hex()}, pushed: {pushed.hex()}$"):
                pyref.dah_from_eds(eds.reshape(W, W, 512))


def _pyref_levels(cells, k, axis_index):
    """The inner levels of one blind pyref tree: [level 1 nodes, level 2 ...]."""
    import pyref
    nodes = pyref.erasured_leaves(cells, k, axis_index, blind=True)
    out = []
    while len(nodes) > 1:
        nodes = [pyref.nmt_hash_node(nodes[i], nodes[i + 1]) for i in range(0, len(nodes), 2)]
        out.append(nodes)
    return out


@pytest.mark.parametrize("k", TABLE_KS)
def test_p_left_reaches_the_parity_min_left_children(k):
    """What makes the GPU comparison of the P-left square able to fail: among
    the blind row trees, and among the column trees, at least k inner nodes
    are left children at level >= 1 with min = FF*29 and max != FF*29, some
    at every level from 1 to log2(k) - 1.  Counted on namespace ranks
    (nmt_edge_squares.ns_tree_levels); at k <= 16 the same count on the nodes
    of pyref's trees."""
    import coracle
    q0 = es.square("p_left", k)
    rank = es.ladder_rank_of(q0)
    lg = k.bit_length() - 1
    for axis, rk in ((0, rank), (1, rank.T)):
        count = es.parity_min_left_children(rk)
        print(f"k={k} axis={axis}: {count}")
        assert sum(count.values()) >= k, (k, axis, count)
        assert all(count[level] >= 1 for level in range(1, lg)), (k, axis, count)
        if k <= 16:
            W = 2 * k
            eds = coracle.extend(q0.reshape(k * k, 512)).reshape(W, W, 512)
            g = eds if axis == 0 else eds.transpose(1, 0, 2)
            seen = {}
            for i in range(W):
                for level, nodes in enumerate(_pyref_levels([c.tobytes() for c in g[i]], k, i), 1):
                    hit = [j for j, nd in enumerate(nodes) if j % 2 == 0 and len(nodes) > 1
                           and nd[:29] == es.PARITY and nd[29:58] != es.PARITY]
                    seen[level] = seen.get(level, 0) + len(hit)
            assert {l: c for l, c in seen.items() if l <= lg} == count, (k, axis)
            assert all(c == 0 for l, c in seen.items() if l > lg)


@pytest.mark.parametrize("name", ["ladder", "last_p_cell", "last_p_row", "last_p_col"])
def test_ignore_max_fires_inside_q0(name):
    """At least one Q0-half subtree root has max < FF*29 although its last
    leaves are FF*29: IgnoreMaxNamespace applies inside the Q0 half."""
    for k in TABLE_KS:
        q0 = es.square(name, k)
        is_p = (q0[:, :, :29] == 0xFF).all(axis=2).astype(np.int64)
        found = 0
        for rk in (is_p, is_p.T):
            for level, mins, maxs in es.ns_tree_levels(rk, parity_rank=1):
                span = 1 << level
                last_leaf = rk[:, span - 1::span]
                found += int(((last_leaf == 1) & (maxs != 1)).sum())
        assert found >= 1, (name, k)


@needs_gxx
def test_table_reaches_every_node_hashing_form():
    plans = hp.plans()
    forms = {kn: _forms(plans[kn]) for kn in TABLE}
    reached = set().union(*forms.values())
    assert reached >= {"leaf_pair", "leaf", "level over inner nodes", "subtree n_in<1024", "subtree n_in=1024",
                       "tree_top pair", "tree_top wide", "tree_top non-pair"}, reached
    # the rows that keep every inner node in tree_top, which has no mid-state branch
    for kn in ((4, 1), (16, 1), (16, 21), (32, 21)):
        assert not any(f.startswith(("level", "subtree")) for f in forms[kn]), kn
    assert len(set(TABLE)) == len(TABLE)
    for env, kn in AB_CASES:
        assert kn in hp.VARIANT_CASES and env in hp.VARIANT_ENVS
        forced = hp.plans(hp.env_knobs(env))[kn]
        assert [hp.class_key(p) for p in forced] != [hp.class_key(p) for p in plans[kn]], (env, kn)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
_expect = {"k": None}


def _expected(k, name):
    """(ods, eds, rows, cols, root, status, detail) of one distinct square of
    width k from the C oracle, cached for the k in hand: the honest oracle for
    ordered and random squares, the blind one for unordered squares."""
    import coracle
    from celestia_da import testfactory
    if _expect["k"] != k:
        _expect.clear()
        _expect["k"] = k
    if name in _expect:
        return _expect[name]
    if name.startswith("random:"):
        ods, ordered = testfactory.random_square(k, int(name.split(":")[1])), True
    else:
        ods, ordered = es.square(name, k).reshape(k * k, 512), es.SQUARES[name][1]
    if ordered:
        eds, rows, cols, root = coracle.cpu_baseline(ods, 16) if k >= 64 else coracle.extend_dah(ods)
        out = (ods, eds, rows, cols, root, 0, (-1, 0, 0))
    else:
        eds, rows, cols, root = coracle.blind_extend_dah(ods, 16 if k >= 64 else 0)
        out = (ods, eds, rows, cols, root, CDA_ERR_PUSH_ORDER, es.first_violation(ods.reshape(k, k, 512)))
    _expect[name] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", TABLE)
def test_edge_batch_matches_oracle(ctx, k, n):
    """One in-place device batch of n squares of width k on the product
    library: square i holds distinct square i % d of nmt_edge_squares.
    batch_names(k) (d odd, or n if smaller).  Every square's EDS, row roots,
    column roots and data root equal the oracle's -- the blind oracle's for
    the unordered squares -- compared on the device; the status is
    CDA_ERR_PUSH_ORDER exactly on the unordered squares, with the brute-force
    first violation as detail at their first and last copy.

    Before the mid-state branch of hash_node checked all 55 bytes of its
    constant head, the P-left square failed here on every row with a level
    launch over inner nodes or a subtree launch (first: k=16 n=257 square
    i=0, row roots, byte 238 -- the digest of row 2) and passed on the four
    tree_top-only rows; no other square differed."""
    import torch
    W = 2 * k
    names = es.batch_names(k)
    names = names[:min(n, len(names))]
    d = len(names)
    dev = torch.device("cuda", 0)
    exp = [_expected(k, name) for name in names]
    eds = rows = cols = roots = status = None
    try:
        eds = torch.zeros((n, W, W, 512), dtype=torch.uint8, device=dev)
        for j in range(d):
            eds[j::d, :k, :k] = torch.from_numpy(exp[j][0]).to(dev).view(k, k, 512)
        rows = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
        cols = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
        roots = torch.empty(n, 32, dtype=torch.uint8, device=dev)
        status = torch.full((n,), 77, dtype=torch.int32, device=dev)
        ctx.extend_dah_inplace_device(k, n, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                      status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()

        failures = []

        def check(which, got, want, j):
            """got[j::d] (device) against `want` (one square's bytes)."""
            w = torch.from_numpy(np.ascontiguousarray(want).reshape(-1)).to(dev)
            g = got[j::d].reshape(-1, w.numel())
            if bool((g == w).all()):
                return
            for p in range(g.shape[0]):   # name the first square that differs
                if not torch.equal(g[p], w):
                    off = int((g[p] != w).nonzero()[0])
                    failures.append(f"k={k} n={n} square i={j + p * d} ({names[j]}): {which} differs from the "
                                    f"oracle at byte {off}: got {g[p][off:off + 8].cpu().tolist()} want "
                                    f"{w[off:off + 8].cpu().tolist()}")
                    return

        for j in range(d):
            _, e_eds, e_rows, e_cols, e_root, _, _ = exp[j]
            check("EDS", eds, e_eds, j)
            check("row roots", rows, e_rows, j)
            check("column roots", cols, e_cols, j)
            check("data root", roots, np.frombuffer(e_root, dtype=np.uint8).copy(), j)
        assert not failures, "\n".join(failures)
        st = status.cpu().tolist()
        want_st = [exp[i % d][5] for i in range(n)]
        assert st == want_st, f"k={k} n={n}: status differs first at i={[a == b for a, b in zip(st, want_st)].index(False)}"
        for j in range(d):
            copies = list(range(j, n, d))
            for i in {copies[0], copies[-1]}:
                assert ctx.push_order_detail_at(i) == exp[j][6], f"k={k} n={n} i={i} ({names[j]}): push-order detail"
    finally:
        del eds, rows, cols, roots, status
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("env,kn", AB_CASES, ids=lambda x: "-".join(f"{a}={b}" for a, b in x.items())
                         if isinstance(x, dict) else f"{x[0]}x{x[1]}")
def test_ab_form_matches_oracle_on_edge_squares(env, kn):
    """The A/B forms of the test build that move tree levels between level,
    subtree and tree_top, one child process each as test_variants.py starts
    them, over P-left (even squares) and the ladder square (odd squares):
    status, EDS digest, row and column root digests and data root against the
    oracle, the blind one for P-left."""
    import coracle
    import test_variants
    k, n = kn
    got = test_variants._run_cases(env, [kn], squares="edges")[0]
    assert len(got) == n
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    want = []
    for name in ("p_left", "ladder")[:n]:
        ods = es.square(name, k)
        if name == "p_left":
            eds, rows, cols, root = coracle.blind_extend_dah(ods, 16)
        else:
            eds, rows, cols, root = coracle.cpu_baseline(ods, 16)
        want.append({"status": CDA_ERR_PUSH_ORDER if name == "p_left" else 0, "data_root": root.hex(),
                     "eds_sha256": sha(eds), "row_roots_sha256": sha(rows), "col_roots_sha256": sha(cols)})
    for i in range(n):
        for field in ("status", "eds_sha256", "row_roots_sha256", "col_roots_sha256", "data_root"):
            assert got[i][field] == want[i % 2][field], (env, k, n, i, ("p_left", "ladder")[i % 2], field)
