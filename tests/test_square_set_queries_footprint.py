"""The footprint of the caller-owned buffers of the set query calls, with
tests/guarded.py as tests/test_square_set_footprint.py uses it: every output
and every const input lies inside lead | payload | trail filled with a pattern.

  cda_square_set_namespace_plan    squares n*4, namespaces n*29 (inputs)
  cda_square_set_namespace_proofs  the ten arrays of cda_namespace_proofs_out
  cda_square_set_share_proofs      squares, starts, ends n*4; the sixteen arrays of cda_share_proofs_out
  cda_namespace_proofs_verify_set  row_roots n_squares*2k*90, squares, the batch's arrays (inputs); verdict n

Each case asserts: the payload equals what the members answer, the guards still
hold the pattern, a NULL output or a refused call writes nothing, and every
input is byte-identical afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import coracle
import guarded

U8P, U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
OK, INVALID = 0, -6


def _p(g, t=U8P):
    return C.cast(g.ptr, t)


def test_argument_errors_that_need_no_device():
    """A NULL set or context is refused before any device work, and the mirror knows the symbols."""
    from celestia_da import _lib, namespace, proof
    L = _lib.load()
    sq = np.zeros(1, dtype=np.uint32)
    ns = np.zeros(29, dtype=np.uint8)
    plan = _lib.NamespacePlanT(7, 7, 7)
    u32 = sq.ctypes.data_as(U32P)
    assert L.cda_square_set_namespace_plan(None, u32, _lib.ptr(ns), 1, C.byref(plan)) == INVALID
    assert (plan.n_segments, plan.n_nodes, plan.n_shares) == (7, 7, 7)
    assert L.cda_square_set_namespace_proofs(None, u32, _lib.ptr(ns), 1, C.byref(_lib.NamespaceProofsOut())) == INVALID
    assert L.cda_square_set_share_proofs(None, u32, u32, u32, 1, C.byref(_lib.ShareProofsOut())) == INVALID
    verdict = np.full(1, 0xAA, dtype=np.uint8)
    b = _lib.NamespaceProofBatch()
    b.n_queries = 1
    assert L.cda_namespace_proofs_verify_set(None, 1, _lib.ptr(ns), 1, u32, C.byref(b), _lib.ptr(verdict)) == INVALID
    assert L.cda_last_error(None).decode() == "null context" and verdict[0] == 0xAA
    assert all(hasattr(proof.ResidentSquareSet, n) for n in ("namespace_plan", "namespace_proofs", "share_proofs_batch"))
    assert all(hasattr(namespace, n) for n in ("SetNamespaceProofs", "namespace_proofs_set", "get_shares_by_namespace_set",
                                               "verify_namespaced_shares_set"))
    import celestia_da
    assert celestia_da.get_shares_by_namespace_set is namespace.get_shares_by_namespace_set
    assert celestia_da.verify_namespaced_shares_set is namespace.verify_namespaced_shares_set


def _ods(k, n):
    return np.stack([coracle.random_square(k, 9300 + 8 * k + i) for i in range(n)])


def _queries(ods, k, n, count, seed):
    """count (square, namespace): present namespaces of the member, the ones just above them, the all-zero one."""
    rng = np.random.default_rng(seed)
    squares = rng.integers(0, n, count).astype(np.uint32)
    nss = np.zeros((count, 29), dtype=np.uint8)
    for i, y in enumerate(squares.tolist()):
        cell = ods[y].reshape(k * k, 512)[int(rng.integers(0, k * k)), :29]
        kind = i % 3
        if kind == 0:
            nss[i] = cell
        elif kind == 1:
            nss[i] = np.frombuffer((int.from_bytes(cell.tobytes(), "big") + 1).to_bytes(29, "big"), dtype=np.uint8)
    return squares, nss


NS_OUT = (("seg_off", 4, U32P), ("row", 4, U32P), ("kind", 1, U8P), ("nmt_start", 4, C.POINTER(C.c_int32)),
          ("nmt_end", 4, C.POINTER(C.c_int32)), ("node_off", 4, U32P), ("nodes", 1, U8P),
          ("share_off", 8, C.POINTER(C.c_uint64)), ("shares", 1, U8P), ("absence_leaf", 1, U8P))


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,count", [(4, 5, 37), (32, 3, 130)])
def test_namespace_calls_and_the_verifier(ctx, k, n, count):
    from celestia_da import _lib, proof as gpr
    from celestia_da.namespace import NamespaceProofsBatch
    W = 2 * k
    ods = _ods(k, n)
    sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    try:
        squares, nss = _queries(ods, k, n, count, 5 * k)
        g_sq = guarded.from_data(squares, align=4, backend="numpy", name="squares")
        g_ns = guarded.from_data(nss, stride=29, align=1, backend="numpy", name="namespaces")
        # what the members answer, query by query
        answers = [sqset[int(y)].namespace_proofs([nss[i]]).answers()[0] for i, y in enumerate(squares)]
        want = NamespaceProofsBatch.from_answers(k, nss, answers)
        assert (want.kind == 1).any() and (want.kind == 2).any() and len(want.shares)
        plan = _lib.NamespacePlanT()
        assert ctx.lib.cda_square_set_namespace_plan(sqset.h, _p(g_sq, U32P), _p(g_ns), count, C.byref(plan)) == OK
        assert (plan.n_segments, plan.n_nodes, plan.n_shares) == (len(want.row), len(want.nodes), len(want.shares))

        def run(mask, sq_arg=None):
            bufs = [guarded.alloc(a.nbytes, stride=a.nbytes // max(1, a.shape[0]), align=al, backend="numpy", name=nm)
                    for (nm, al, _), a in zip(NS_OUT, want.arrays())]
            o = _lib.NamespaceProofsOut()
            for j, ((nm, _, t), b) in enumerate(zip(NS_OUT, bufs)):
                if mask >> j & 1:
                    setattr(o, nm, _p(b, t))
            rc = ctx.lib.cda_square_set_namespace_proofs(sqset.h, sq_arg or _p(g_sq, U32P), _p(g_ns), count, C.byref(o))
            return rc, bufs

        full = (1 << len(NS_OUT)) - 1
        for mask in [full] + [1 << j for j in range(len(NS_OUT))] + [full ^ (1 << j) for j in range(len(NS_OUT))] + [0]:
            rc, bufs = run(mask)
            assert rc == OK, mask
            for j, (b, a) in enumerate(zip(bufs, want.arrays())):
                if mask >> j & 1:
                    b.assert_written(a)
                    b.assert_guards()
                else:
                    b.assert_untouched()
        # a refused call (square out of range in the last query) writes nothing
        bad_sq = squares.copy()
        bad_sq[-1] = n
        bad = guarded.from_data(bad_sq, align=4, backend="numpy", name="squares")
        rc, bufs = run(full, _p(bad, U32P))
        assert rc == INVALID
        assert ctx.lib.cda_last_error(ctx.h).decode().startswith(f"query {count - 1}: square {n} ")
        for b in bufs:
            b.assert_untouched()
        bad.assert_unchanged()

        # the verifier: every array of the batch, the squares and all the DAHs inside guards
        rows, _, _ = sqset.dah()
        g_rows = guarded.from_data(rows, stride=W * 90, align=1, backend="numpy", name="row_roots")
        ins = [guarded.from_data(a, align=al, backend="numpy", name=nm) for (nm, al, _), a in zip(NS_OUT, want.arrays())]
        b = _lib.NamespaceProofBatch()
        b.n_queries, b.n_nodes, b.n_shares = count, len(want.nodes), len(want.shares)
        b.namespaces = _p(g_ns)
        for (nm, _, _), g in zip(NS_OUT, ins):
            setattr(b, nm, C.cast(g.ptr, dict(_lib.NamespaceProofBatch._fields_)[nm]))
        verdict = guarded.alloc(count, align=1, backend="numpy", name="verdict")
        assert ctx.lib.cda_namespace_proofs_verify_set(ctx.h, k, _p(g_rows), n, _p(g_sq, U32P), C.byref(b),
                                                       _p(verdict)) == OK
        verdict.assert_written(np.zeros(count, dtype=np.uint8))
        verdict.assert_guards()
        refused = guarded.alloc(count, align=1, backend="numpy", name="verdict")
        assert ctx.lib.cda_namespace_proofs_verify_set(ctx.h, k, _p(g_rows), n, _p(bad, U32P), C.byref(b),
                                                       _p(refused)) == INVALID
        refused.assert_untouched()
        for g in ins + [g_rows, g_sq, g_ns, bad]:
            g.assert_unchanged()
    finally:
        sqset.close()


SH_OUT = (("seg_off", 4, U32P), ("nmt_start", 4, None), ("nmt_end", 4, None), ("node_off", 4, U32P), ("nodes", 1, U8P),
          ("row_roots", 1, U8P), ("rfc_total", 8, None), ("rfc_index", 8, None), ("rfc_leaf_hash", 1, U8P),
          ("aunt_off", 4, U32P), ("aunts", 1, U8P), ("shares", 1, U8P), ("namespaces", 1, U8P), ("start_row", 4, U32P),
          ("end_row", 4, U32P), ("one_namespace", 1, U8P))


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,count", [(4, 5, 37), (32, 3, 130)])
def test_share_proofs(ctx, k, n, count):
    from celestia_da import _lib, proof as gpr
    from celestia_da.proof import ShareProofsBatch
    ods = _ods(k, n)
    sqset = gpr.ResidentSquareSet.from_ods(ods, ctx)
    try:
        rng = np.random.default_rng(count + k)
        squares = rng.integers(0, n, count).astype(np.uint32)
        starts = rng.integers(0, k * k, count).astype(np.uint32)
        ends = np.minimum(starts + rng.integers(1, 3 * k, count).astype(np.uint32), k * k).astype(np.uint32)
        ins = [guarded.from_data(a, align=4, backend="numpy", name=nm)
               for a, nm in zip((squares, starts, ends), ("squares", "starts", "ends"))]
        in_args = [_p(g, U32P) for g in ins]
        # what the members answer: range by range, put together as the flat batch
        want = ShareProofsBatch.empty(k, np.stack([starts, ends], axis=1), fill=0)
        seg = node = aunt = share = 0
        want.seg_off[0] = want.node_off[0] = want.aunt_off[0] = 0
        for i, y in enumerate(squares.tolist()):
            one = sqset[y].share_proofs_batch([(int(starts[i]), int(ends[i]))])
            S, N, A, H = len(one.row_roots), len(one.nodes), len(one.aunts), len(one.shares)
            want.seg_off[i + 1] = seg + S
            want.node_off[seg + 1:seg + S + 1] = one.node_off[1:] + node
            want.aunt_off[seg + 1:seg + S + 1] = one.aunt_off[1:] + aunt
            for name in ("nmt_start", "nmt_end", "row_roots", "rfc_total", "rfc_index", "rfc_leaf_hash"):
                getattr(want, name)[seg:seg + S] = getattr(one, name)
            want.nodes[node:node + N], want.aunts[aunt:aunt + A], want.shares[share:share + H] = one.nodes, one.aunts, one.shares
            for name in ("namespaces", "start_row", "end_row", "one_namespace"):
                getattr(want, name)[i] = getattr(one, name)[0]
            seg, node, aunt, share = seg + S, node + N, aunt + A, share + H
        assert (seg, node, aunt, share) == (len(want.row_roots), len(want.nodes), len(want.aunts), len(want.shares))
        types = dict(_lib.ShareProofsOut._fields_)

        def run(mask, inputs=in_args):
            bufs = [guarded.alloc(a.nbytes, stride=a.nbytes // max(1, a.shape[0]), align=al, backend="numpy", name=nm)
                    for (nm, al, _), a in zip(SH_OUT, want.arrays())]
            o = _lib.ShareProofsOut()
            for j, ((nm, _, _), b) in enumerate(zip(SH_OUT, bufs)):
                if mask >> j & 1:
                    setattr(o, nm, C.cast(b.ptr, types[nm]))
            return ctx.lib.cda_square_set_share_proofs(sqset.h, *inputs, count, C.byref(o)), bufs

        full = (1 << len(SH_OUT)) - 1
        for mask in [full] + [1 << j for j in range(len(SH_OUT))] + [full ^ (1 << j) for j in range(len(SH_OUT))] + [0]:
            rc, bufs = run(mask)
            assert rc == OK, mask
            for j, (b, a) in enumerate(zip(bufs, want.arrays())):
                if mask >> j & 1:
                    b.assert_written(a)
                    b.assert_guards()
                else:
                    b.assert_untouched()
        bad_sq = squares.copy()
        bad_sq[-1] = n
        bad = guarded.from_data(bad_sq, align=4, backend="numpy", name="squares")
        rc, bufs = run(full, [_p(bad, U32P)] + in_args[1:])
        assert rc == INVALID
        assert ctx.lib.cda_last_error(ctx.h).decode().startswith(f"range {count - 1}: square {n} ")
        for b in bufs:
            b.assert_untouched()
        for g in ins + [bad]:
            g.assert_unchanged()
    finally:
        sqset.close()
