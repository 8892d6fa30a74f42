"""The widest square the library accepts, k = 1024, through every entry point
that takes it -- and the rejection of every call that does not.

k = 1024 is the only width that runs rs16_lds_kernel (64 KiB of LDS, the
log/exp GF(2^16) encoder), six hash schedules of hash_plan.h, depth-11 axis
trees and the 4 096-leaf data-root tree.  Everything here is byte-exact:

  * extension and DAH against tests/golden/k1024.json, the C oracle's digests
    of squares 0 and 1 (oracle/gen_config4.py --k 1024 --count 2);
  * a square with a push-order violation against coracle.blind_extend_dah;
  * Reed-Solomon codewords against coracle / pyref leopard_encode;
  * samples, share proofs, subtree walks, namespace and commitment proofs
    against oracle/proofs.py and the restatements tests/nmt_namespace_ref.py
    and tests/commitment_proof_ref.py.

Cost: the oracle runs twice at this width (the swapped square of the batch of
three, the ordered square of the namespace and commitment tests).  The
reference EDS of square 0 is the library's own, once its SHA-256 equals the
oracle's committed digest; it stays on the device and only the rows and
columns a reference needs come to the host, so no test holds more than one
2 GiB EDS in host memory.  The tests run in file order, narrow to wide: the
small cda_rs_encode codewords first.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import coracle
import proofs as opr
import pyref
from celestia_da import CdaError, _lib
from celestia_da._lib import ptr

HERE = os.path.dirname(os.path.abspath(__file__))
K = 1024
W = 2 * K
TOO_WIDE = "square width must be a power of two <= 1024"
EDS_WIDTH = "EDS width must be a power of two in [2, 1024]"


def golden():
    with open(os.path.join(HERE, "golden", "k1024.json")) as f:
        g = json.load(f)
    assert g["k"] == K and sorted(g["squares"]) == ["0", "1"]
    return g["squares"]


def _sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _sha_dev(t) -> str:
    """SHA-256 of a device tensor's bytes, 128 MiB at a time on the host."""
    h = hashlib.sha256()
    for part in t.reshape(-1).split(1 << 27):
        h.update(part.cpu().numpy())
    return h.hexdigest()


_ods = {}


def ods(i):
    """Square i of the fixture (k*k, 512), made once and never changed."""
    if i not in _ods:
        _ods[i] = coracle.random_square(K, i)
        assert _sha(_ods[i]) == golden()[str(i)]["ods_sha256"]
    return _ods[i]


def first_violation(q0):
    """Brute-force nmt push-order check of one Q0 (k, k, 512), every adjacent
    pair compared: the smallest (axis, index, position) whose namespace is
    below its predecessor's, rows before columns, as cda_push_order_detail_at
    reports it; None if ordered."""
    for axis in (0, 1):
        ns = (q0 if axis == 0 else q0.transpose(1, 0, 2))[:, :, :29]
        a, b = ns[:, :-1], ns[:, 1:]
        ne = a != b
        at = ne.argmax(axis=-1)[..., None]
        below = ne.any(axis=-1) & (np.take_along_axis(b, at, -1)[..., 0] < np.take_along_axis(a, at, -1)[..., 0])
        if below.any():
            i, p = np.argwhere(below)[0]
            return (axis, int(i), int(p) + 1)
    return None


def test_first_violation_is_the_brute_force_one():
    import nmt_edge_squares as edge
    for name in ("descent_row", "descent_col", "p_left", "ladder"):
        q0 = edge.square(name, 16)
        assert first_violation(q0) == edge.first_violation(q0), name


def assert_roots(rows, cols, root, want, what):
    assert _sha(rows) == want["row_roots_sha256"], f"{what}: row roots"
    assert _sha(cols) == want["col_roots_sha256"], f"{what}: column roots"
    assert bytes(root) == bytes.fromhex(want["data_root"]), f"{what}: data root"


# ---------------------------------------------------------------------------
# 1. cda_rs_encode: rs16_flat_kernel at 1 024 shards (the smallest inputs that
#    run encode_block_column at this width)
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("length", [64, 512])
def test_rs_encode_1024_shards(ctx, length):
    from celestia_da import rsmt2d
    rng = np.random.default_rng(1024 + length)
    data = rng.integers(0, 256, (3, K, length), dtype=np.uint8)
    got = rsmt2d.LeoRSCodec(ctx).encode_batch(data)
    for i in range(3):
        assert np.array_equal(got[i], coracle.leopard_encode(data[i])), i


@pytest.mark.gpu
@pytest.mark.parametrize("n_shards", [513, 1000, 1023])
def test_rs_encode_pads_to_1024_shards(ctx, n_shards):
    """klauspost pads a non-power-of-two shard count with zero shards up to
    ceilPow2 = 1 024 and keeps the first n_shards parity shards."""
    from celestia_da import rsmt2d
    rng = np.random.default_rng(n_shards)
    data = rng.integers(0, 256, (2, n_shards, 64), dtype=np.uint8)
    got = rsmt2d.LeoRSCodec(ctx).encode_batch(data)
    for i in range(2):
        assert np.array_equal(got[i], pyref.leopard_encode(data[i])), i


@pytest.mark.gpu
def test_rs_encode_rejects_1025_shards(ctx):
    data = np.zeros((1025, 64), dtype=np.uint8)
    out = np.full_like(data, 0xAA)
    assert ctx.lib.cda_rs_encode(ctx.h, ptr(data), 1025, 64, 1, ptr(out)) == _lib.CDA_ERR_UNSUPPORTED
    assert ctx.lib.cda_last_error(ctx.h).decode() == "more than 2048 shards"
    assert (out == 0xAA).all()


# ---------------------------------------------------------------------------
# 2. extension and DAH
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def d_ods():
    """Squares 0 and 1 on the device, (k, k, 512) each."""
    import torch
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(ods(i)).to(dev).view(K, K, 512) for i in (0, 1)]
    yield t
    del t
    torch.cuda.empty_cache()


def _outs(n, dev):
    import torch
    return (torch.zeros(n, W * 90, dtype=torch.uint8, device=dev), torch.zeros(n, W * 90, dtype=torch.uint8, device=dev),
            torch.zeros(n, 32, dtype=torch.uint8, device=dev), torch.full((n,), 77, dtype=torch.int32, device=dev))


def _inplace(ctx, squares):
    """cda_extend_dah_inplace_device of the device squares `squares`:
    (eds (n, W, W, 512), rows, cols, roots, status) as device tensors."""
    import torch
    dev = squares[0].device
    n = len(squares)
    eds = torch.zeros((n, W, W, 512), dtype=torch.uint8, device=dev)
    for i, q0 in enumerate(squares):
        eds[i, :K, :K] = q0
    rows, cols, roots, status = _outs(n, dev)
    ctx.extend_dah_inplace_device(K, n, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                  status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return eds, rows, cols, roots, status


@pytest.mark.gpu
def test_one_square_three_entry_points(ctx, d_ods):
    """Square 0 through cda_extend_dah (host buffers), cda_extend_dah_device
    (a separate ODS: rs16_lds_kernel's copy path) and
    cda_extend_dah_inplace_device (kNoCopy), each against the oracle's digests."""
    import torch
    want = golden()["0"]
    dev = d_ods[0].device
    # host buffers
    eds = np.zeros(W * W * 512, dtype=np.uint8)
    rows, cols = np.zeros(W * 90, dtype=np.uint8), np.zeros(W * 90, dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    assert ctx.lib.cda_extend_dah(ctx.h, ptr(ods(0)), K * K, ptr(eds), ptr(rows), ptr(cols), ptr(root)) == _lib.CDA_OK
    assert _sha(eds) == want["eds_sha256"], "cda_extend_dah: EDS"
    assert_roots(rows, cols, root, want, "cda_extend_dah")
    del eds
    # a separate ODS on the device
    d_eds = torch.zeros((W, W, 512), dtype=torch.uint8, device=dev)
    d_rows, d_cols, d_roots, d_status = _outs(1, dev)
    ctx.extend_dah_device(d_ods[0].data_ptr(), K, 1, d_eds.data_ptr(), d_rows.data_ptr(), d_cols.data_ptr(),
                          d_roots.data_ptr(), d_status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [0]
    assert _sha_dev(d_eds) == want["eds_sha256"], "cda_extend_dah_device: EDS"
    assert_roots(d_rows.cpu().numpy(), d_cols.cpu().numpy(), d_roots.cpu().numpy().tobytes(), want,
                 "cda_extend_dah_device")
    assert ctx.push_order_detail_at(0) == (-1, 0, 0)
    # in place: equal to the EDS just digested
    i_eds, i_rows, i_cols, i_roots, i_status = _inplace(ctx, [d_ods[0]])
    assert i_status.cpu().tolist() == [0]
    assert torch.equal(i_eds[0], d_eds), "cda_extend_dah_inplace_device: EDS"
    assert_roots(i_rows.cpu().numpy(), i_cols.cpu().numpy(), i_roots.cpu().numpy().tobytes(), want,
                 "cda_extend_dah_inplace_device")
    del d_eds, i_eds
    torch.cuda.empty_cache()


def _swapped():
    """Square 0 with two adjacent, different Q0 namespaces of row 2 swapped,
    and the first violation that leaves."""
    q0 = ods(0).reshape(K, K, 512).copy()
    r = 2
    c = next(c for c in range(K - 1) if q0[r, c, :29].tobytes() != q0[r, c + 1, :29].tobytes())
    q0[r, c, :29], q0[r, c + 1, :29] = q0[r, c + 1, :29].copy(), q0[r, c, :29].copy()
    want = first_violation(q0)
    assert want is not None and want <= (0, r, c + 1)
    return q0, want


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_inplace_batch(ctx, d_ods, n):
    """In-place batches of squares 0, 1, 0, 1, ...: n = 2, 3, 4, 5 and 8 are
    the batch sizes at which hash_plan.h changes the schedule of a k = 1024
    batch.  Every square's roots and data root against the oracle's digests,
    every EDS equal on the device to the first copy of its square, the two
    first copies digested.  The last square of the batch of three carries a
    push-order violation: its status and detail, and its EDS, roots and data
    root against the blind oracle (BlindTree: the hashing without the order
    check)."""
    import torch
    g = golden()
    dev = d_ods[0].device
    squares = [d_ods[i % 2] for i in range(n)]
    bad = None
    if n == 3:
        q0, detail = _swapped()
        bad = 2
        squares[bad] = torch.from_numpy(q0).to(dev)
    eds, rows, cols, roots, status = _inplace(ctx, squares)
    try:
        assert status.cpu().tolist() == [-3 if i == bad else 0 for i in range(n)]   # CDA_ERR_PUSH_ORDER
        h_rows, h_cols, h_roots = rows.cpu().numpy(), cols.cpu().numpy(), roots.cpu().numpy()
        for i in range(n):
            if i != bad:
                assert_roots(h_rows[i], h_cols[i], h_roots[i].tobytes(), g[str(i % 2)], f"n={n} square {i}")
        for j in (0, 1):
            assert _sha_dev(eds[j]) == g[str(j)]["eds_sha256"], f"n={n} square {j}: EDS"
        for i in range(2, n):
            if i != bad:
                assert torch.equal(eds[i], eds[i % 2]), f"n={n} square {i}: EDS differs from square {i % 2}'s"
        assert ctx.push_order_detail_at(0) == (-1, 0, 0) and ctx.push_order_detail_at(n - 1) == (
            detail if bad == n - 1 else (-1, 0, 0))
        if bad is not None:
            assert ctx.push_order_detail_at(bad) == detail
            e_eds, e_rows, e_cols, e_root = coracle.blind_extend_dah(q0.reshape(K * K, 512), 16)
            assert np.array_equal(h_rows[bad].reshape(W, 90), e_rows), "swapped square: row roots"
            assert np.array_equal(h_cols[bad].reshape(W, 90), e_cols), "swapped square: column roots"
            assert h_roots[bad].tobytes() == e_root, "swapped square: data root"
            assert torch.equal(eds[bad].reshape(-1), torch.from_numpy(e_eds.reshape(-1)).to(dev)), "swapped square: EDS"
            del e_eds
    finally:
        del eds, squares
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_extend_shares_then_dah_from_eds(ctx):
    """cda_extend_shares and cda_dah_from_eds, called separately, on square 0."""
    want = golden()["0"]
    eds = np.zeros(W * W * 512, dtype=np.uint8)
    assert ctx.lib.cda_extend_shares(ctx.h, ptr(ods(0)), K * K, ptr(eds)) == _lib.CDA_OK
    assert _sha(eds) == want["eds_sha256"]
    rows, cols = np.zeros(W * 90, dtype=np.uint8), np.zeros(W * 90, dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    assert ctx.lib.cda_dah_from_eds(ctx.h, ptr(eds), W, ptr(rows), ptr(cols), ptr(root)) == _lib.CDA_OK
    assert_roots(rows, cols, root, want, "cda_dah_from_eds")
    # cda_data_root over the 4 096 roots: the widest RFC-6962 tree
    again = np.zeros(32, dtype=np.uint8)
    assert ctx.lib.cda_data_root(ctx.h, ptr(rows), ptr(cols), W, ptr(again)) == _lib.CDA_OK
    assert again.tobytes().hex() == want["data_root"]


# ---------------------------------------------------------------------------
# 3. resident squares
# ---------------------------------------------------------------------------
class DeviceEds:
    """A (2k, 2k, 512) EDS that stays on the device and is read like a numpy
    array: only the cells a reference asks for come to the host."""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, idx):
        return self.t[idx].cpu().numpy()


class Leaves:
    """leaves[r]: the leaf nodes of row tree r, hashed on first use."""

    def __init__(self, eds):
        self.eds, self.made = eds, {}

    def __getitem__(self, r):
        if r not in self.made:
            self.made[r] = pyref.erasured_leaves([bytes(c) for c in self.eds[r]], K, r)
        return self.made[r]


class RefSquare:
    """What tests/nmt_namespace_ref.py reads of a square (k, eds, leaves,
    row_roots), over an EDS and row roots that are the oracle's."""

    def __init__(self, eds, row_roots):
        self.k, self.eds, self.leaves, self.row_roots = K, eds, Leaves(eds), [bytes(r) for r in row_roots]


class Resident:
    pass


@pytest.fixture(scope="module")
def resident(ctx, d_ods):
    """Square 0 as cda_square_create makes it, and squares 0 and 1 as a set
    built by cda_square_set_create_device from the EDS of an in-place batch.
    That batch's EDS, roots and data roots equal the oracle's digests, so they
    are the reference the proofs are compared with; the EDS stays on the device."""
    import torch
    from celestia_da import proof as gpr
    g = golden()
    eds, rows, cols, roots, status = _inplace(ctx, [d_ods[0], d_ods[1]])
    r = Resident()
    r.rows, r.cols, r.roots = rows.cpu().numpy().reshape(2, W, 90), cols.cpu().numpy().reshape(2, W, 90), roots.cpu().numpy()
    for i in (0, 1):
        assert_roots(r.rows[i], r.cols[i], r.roots[i].tobytes(), g[str(i)], f"square {i}")
        assert _sha_dev(eds[i]) == g[str(i)]["eds_sha256"]
    r.eds = [DeviceEds(eds[0]), DeviceEds(eds[1])]
    r.root = [r.roots[i].tobytes() for i in (0, 1)]
    r.set = gpr.ResidentSquareSet.from_device_eds(eds, K, 2, torch.cuda.current_stream(eds.device).cuda_stream, ctx)
    r.sq = gpr.ResidentSquare(ods(0), ctx)
    r.ref = [RefSquare(r.eds[i], r.rows[i]) for i in (0, 1)]
    yield r
    r.sq.close()
    r.set.close()
    del eds, r
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_resident_dah(resident):
    g = golden()
    rows, cols, root = resident.sq.dah()
    assert_roots(np.frombuffer(b"".join(rows), np.uint8), np.frombuffer(b"".join(cols), np.uint8), root, g["0"],
                 "cda_square_dah")
    assert not resident.sq.push_order_error and resident.set.status.tolist() == [0, 0]
    s_rows, s_cols, s_roots = resident.set.dah()
    for i in (0, 1):
        assert_roots(s_rows[i], s_cols[i], s_roots[i].tobytes(), g[str(i)], f"cda_square_set_dah member {i}")


EDGES = (0, K - 1, K, W - 1)
# the four corners of each quadrant on both axes, and cells inside every quadrant's edge rows and columns
SAMPLES = np.array([(r, c, a) for a in (0, 1) for r in EDGES for c in EDGES]
                   + [(5, K - 1, 0), (K, 7, 1), (W - 1, 1500, 0), (1500, W - 1, 1), (K - 1, 600, 1), (300, K, 0)],
                   dtype=np.int64)


def _deepest(p):
    """Index, among the 11 proof nodes of leaf p, of its sibling leaf: the
    nodes run left siblings top-down, then right siblings bottom-up."""
    ones = bin(p).count("1")
    return ones - 1 if p & 1 else ones


@pytest.mark.gpu
def test_samples(ctx, resident):
    """Cells at the corners of every quadrant, rows and columns 1 023, 1 024
    and 2 047 on both axes: 11 NMT nodes and 12 aunts each, equal to
    oracle/proofs.py over the oracle's EDS; verified honest and with one node
    of the deepest level flipped; the set call gives the single-square answers."""
    from celestia_da import sampling
    from test_sampling import Checker, assert_batch_equals, batch_verdicts
    ch = object.__new__(Checker)
    ch.k, ch.W, ch.ods, ch.eds = K, W, None, resident.eds[0]
    ch.rows, ch.cols = [bytes(x) for x in resident.rows[0]], [bytes(x) for x in resident.cols[0]]
    ch.root, ch._leaves, ch._rfc = resident.root[0], {}, {}
    batch = resident.sq.sample_proofs(SAMPLES)
    assert batch.nmt_nodes.shape[1:] == (11, 90) and batch.aunts.shape[1:] == (12, 32)
    assert_batch_equals(batch, ch.arrays(SAMPLES))
    n = len(SAMPLES)
    assert sampling.verify_samples(batch, ch.root, ctx).tolist() == [0] * n == batch_verdicts(batch, [ch.root] * n)
    bad = batch.copy()
    for i, (row, col, axis) in enumerate(SAMPLES.tolist()):
        bad.nmt_nodes[i, _deepest(col if axis == 0 else row), 60] ^= 1
    assert sampling.verify_samples(bad, ch.root, ctx).tolist() == [2] * n == batch_verdicts(bad, [ch.root] * n)
    # across the set: member 0 is square 0, member 1 answers as its own handle does
    coords = np.array([(m, *c) for c in SAMPLES.tolist() for m in (1, 0)], dtype=np.int64)
    got = resident.set.sample_proofs(coords)
    one = resident.set[1].sample_proofs(SAMPLES)
    for name, a, b0, b1 in zip(("shares", "namespaces", "nmt_nodes", "axis_roots", "leaf_hash", "aunts"),
                               got.batch.arrays(), batch.arrays(), one.arrays()):
        assert np.array_equal(a[1::2], b0) and np.array_equal(a[0::2], b1), name
    assert not sampling.verify_samples(got.batch, got.data_roots(resident.roots), ctx).any()
    assert (sampling.verify_samples(got.batch, got.data_roots(resident.roots[::-1]), ctx) == 1).all()


@pytest.mark.gpu
def test_share_proofs(ctx, resident):
    """The single shares test_resident_square_k512 proves, at this width:
    every proof validates with the oracle's ShareProof.Validate against the
    oracle's data root, the batch call gives the same proofs and
    cda_share_proofs_verify accepts them; the set call gives the members'."""
    from test_share_proof_validate import to_dict
    sq, shares = resident.sq, ods(0)
    at = (0, 5, K - 1, K, 3 * K + 100, K * K // 2 + 17, K * K - 1)
    ranges = [(s, s + 1) for s in at]
    singles = [sq.share_proof(bytes(shares[s][:29]), s, s + 1) for s in at]
    for s, p in zip(at, singles):
        assert opr.share_proof_validate(to_dict(p), resident.root[0]) is None, s
        assert p.data == [bytes(shares[s])] and len(p.share_proofs[0].nodes) == 11 and len(p.row_proof.proofs[0].aunts) == 12
    batch = sq.share_proofs_batch(ranges)
    assert batch.proofs() == singles
    assert batch.verify(resident.root[0], ctx).tolist() == [0] * len(at)
    assert (batch.verify(resident.root[1], ctx) == 1).all()
    req = [(m, s, s + 1) for s in at for m in (1, 0)]
    got = resident.set.share_proofs_batch(req)
    one = resident.set[1].share_proofs_batch(ranges)
    assert got.proofs()[1::2] == singles and got.proofs()[0::2] == one.proofs()
    assert got.verify(resident.roots, ctx).tolist() == [0] * len(req)
    for p, s in zip(one.proofs(), at):
        assert opr.share_proof_validate(to_dict(p), resident.root[1]) is None and p.data == [bytes(ods(1)[s])]


@pytest.mark.gpu
def test_subtree_walk_of_the_last_row(resident):
    leaves = resident.ref[0].leaves[W - 1]
    walk = [True, False, True, True, False, False, True, False, True, True]
    assert resident.sq.subtree_root(W - 1, walk) == opr.walk_subtree_root(leaves, walk)
    assert resident.sq.subtree_root(W - 1, []) == bytes(resident.rows[0][W - 1])
    assert resident.sq.subtree_root(W - 1, [True] * 11) == leaves[W - 1]


@pytest.mark.gpu
def test_namespace_queries_across_the_set(ctx, resident):
    """cda_square_set_namespace_proofs over both members against the
    restatement, cda_namespace_proofs_verify_set against the two DAHs."""
    import nmt_namespace_ref as ref
    from celestia_da.namespace import NamespaceProofsBatch
    from test_namespace_proofs import assert_batch_equals
    up = lambda ns: (int.from_bytes(ns, "big") + 1).to_bytes(29, "big")   # noqa: E731
    a, b = ods(0), ods(1)
    absent = up(bytes(b[777, :29]))
    assert bytes(b[777, :29]) < absent < bytes(b[778, :29]) and bytes(29) < bytes(a[0, :29])
    queries = [(0, bytes(a[12345, :29])), (1, bytes(b[K * K - 1, :29])), (1, absent), (0, bytes(29)),
               (1, bytes(a[12345, :29]))]
    answers = [ref.get_shares_by_namespace(resident.ref[m], ns) for m, ns in queries]
    assert [len(x) for x in answers[:4]] == [1, 1, 1, 0] and answers[2][0][1].leaf_hash and not answers[0][0][1].leaf_hash
    got = resident.set.namespace_proofs(queries)
    assert_batch_equals(got.batch, K, [ns for _, ns in queries], answers)
    assert resident.set.namespace_plan(queries) == {"n_segments": len(got.batch.row), "n_nodes": len(got.batch.nodes),
                                                    "n_shares": len(got.batch.shares)}
    want = [ref.answer_verdict(resident.ref[m].row_roots, ns, x) for (m, ns), x in zip(queries, answers)]
    assert got.verify(resident.rows, ctx).tolist() == want == [0] * len(queries)
    # the same answers under the other member's DAH
    swapped = [ref.answer_verdict(resident.ref[1 - m].row_roots, ns, x) for (m, ns), x in zip(queries, answers)]
    assert got.verify(resident.rows[::-1], ctx).tolist() == swapped and 0 not in swapped[:3]
    single = resident.sq.namespace_proofs([ns for m, ns in queries if m == 0])
    assert_batch_equals(single, K, [ns for m, ns in queries if m == 0], [x for (m, _), x in zip(queries, answers) if m == 0])
    assert not single.verify(resident.rows[0], ctx).any()
    assert isinstance(single, NamespaceProofsBatch)


# ---------------------------------------------------------------------------
# 4. an ordered square with runs of equal namespaces
# ---------------------------------------------------------------------------
RUN = 2500   # shares per namespace: every run covers at least one whole row


class Ordered:
    pass


@pytest.fixture(scope="module")
def ordered(ctx):
    """Square 2 with share i under the namespace of share 2500 * (i // 2500),
    extended by the oracle; its resident square.  Of the oracle's EDS only the
    upper half (Q0 | Q1, the rows the original shares lie in) is kept."""
    import commitment_proof_ref as cref
    from celestia_da import proof as gpr
    o = Ordered()
    o.ods = coracle.random_square(K, 2)
    o.ods[:, :29] = o.ods[(np.arange(K * K) // RUN) * RUN, :29]
    assert first_violation(o.ods.reshape(K, K, 512)) is None
    eds, rows, cols, root = coracle.cpu_baseline(o.ods, 16)
    o.top = np.ascontiguousarray(eds.reshape(W, W, 512)[:K])
    del eds
    o.rows, o.cols, o.root = rows, cols, root
    o.ref = RefSquare(o.top, rows)
    o.trees = object.__new__(cref.RefTrees)
    o.trees.k, o.trees.eds, o.trees.data_root = K, o.top, root
    o.trees.row_roots, o.trees.col_roots = [bytes(r) for r in rows], [bytes(c) for c in cols]
    o.trees._leaves = o.ref.leaves.made
    o.sq = gpr.ResidentSquare(o.ods, ctx)
    g_rows, g_cols, g_root = o.sq.dah()
    assert g_root == root and g_rows == o.trees.row_roots and g_cols == o.trees.col_roots
    yield o
    o.sq.close()


@pytest.mark.gpu
def test_namespace_proofs(ctx, ordered):
    """A namespace that spans more than one whole row, one that is absent
    inside a row, one below and one above every namespace, the first and the
    last run: plan and proofs equal the restatement, verdicts from
    cda_namespace_proofs_verify."""
    import nmt_namespace_ref as ref
    from celestia_da.namespace import NamespaceProofsBatch, namespace_plan
    from test_namespace_proofs import assert_batch_equals, assert_plan_equals
    up = lambda ns: (int.from_bytes(ns, "big") + 1).to_bytes(29, "big")   # noqa: E731
    run_ns = [bytes(ordered.ods[s, :29]) for s in range(0, K * K, RUN)]
    assert run_ns == sorted(set(run_ns)) and len(run_ns) == 420
    inside, below, above = up(run_ns[1]), bytes(29), up(run_ns[-1])
    assert inside < run_ns[2] and below < run_ns[0] and above < ref.PARITY and (2 * RUN) % K not in (0, K - 1)
    nss = [run_ns[1], inside, below, above, run_ns[0], run_ns[-1]]
    answers = [ref.get_shares_by_namespace(ordered.ref, ns) for ns in nss]
    rows_of = [[r for r, _, _ in x] for x in answers]
    assert rows_of[:4] == [[2, 3, 4], [4], [], []] and rows_of[4] == [0, 1, 2] and rows_of[5][-1] == K - 1
    assert (answers[0][1][1].start, answers[0][1][1].end) == (0, K) and answers[1][0][1].leaf_hash
    got = ordered.sq.namespace_proofs(nss)
    want = assert_batch_equals(got, K, nss, answers)
    assert_plan_equals(namespace_plan(ordered.sq, nss), want)
    assert got.verify(ordered.rows, ctx).tolist() == [0] * len(nss) == [
        ref.answer_verdict(ordered.ref.row_roots, ns, x) for ns, x in zip(nss, answers)]
    # tampered: a share of the whole-row segment flipped, the absence proof's row dropped
    bad = [ref.flip_share(answers[0], 1), []] + answers[2:]
    verdicts = NamespaceProofsBatch.from_answers(K, nss, bad).verify(ordered.rows, ctx).tolist()
    assert verdicts == [2, 1, 0, 0, 0, 0] == [ref.answer_verdict(ordered.ref.row_roots, ns, x) for ns, x in zip(nss, bad)]


@pytest.mark.gpu
def test_commitment_proofs(ctx, ordered):
    """One blob of 3 * 1024 + 17 shares that starts inside a row and one of a
    single share in the last row: equal to the restatement, verified by
    cda_commitment_proofs_verify."""
    import commitment_proof_ref as cref
    from test_commitment_proofs import assert_equals_restatement
    blobs = [(5 * K + 512, 3 * K + 17), (K * K - 5, 1)]
    starts, lens = [b[0] for b in blobs], [b[1] for b in blobs]
    batch = ordered.sq.commitment_proofs(starts, lens, 64)
    want = [cref.prove(ordered.top, K, s, n, 64, trees=ordered.trees) for s, n in blobs]
    assert [len(w.rows) for w in want] == [4, 1] and want[1].rows[0].index == K - 1
    assert_equals_restatement(batch, want, "k = 1024")
    assert batch.commitments.tobytes() == b"".join(cref.commitment(w) for w in want)
    assert batch.commitments.tobytes() == b"".join(ordered.sq.blob_commitments(starts, lens, 64))
    assert batch.verify(ordered.root, ctx=ctx).tolist() == [0, 0]
    assert [cref.verdict(w, ordered.root, cref.commitment(w), 64) for w in want] == [cref.VALID] * 2
    assert batch.verify(ordered.root, [cref.commitment(want[1]), cref.commitment(want[0])], ctx).tolist() == [3, 3]


@pytest.mark.gpu
def test_share_range_across_three_rows(ctx, ordered):
    """One run of 2 500 shares of one namespace -- the end of row 2, all of
    row 3, the start of row 4 -- as a ShareProof: the oracle's Validate
    accepts it against the oracle's data root, and cda_share_proofs_verify
    folds the 1 024 leaves of row 3 and the node beside them, its widest run."""
    from test_share_proof_validate import to_dict
    s, e = RUN, 2 * RUN
    ns = bytes(ordered.ods[s, :29])
    p = ordered.sq.share_proof(ns, s, e)
    assert (p.row_proof.start_row, p.row_proof.end_row) == (2, 4)
    assert [(q.start, q.end, len(q.nodes)) for q in p.share_proofs][1] == (0, K, 1)
    assert b"".join(p.data) == ordered.ods[s:e].tobytes()
    assert opr.share_proof_validate(to_dict(p), ordered.root) is None
    batch = ordered.sq.share_proofs_batch([(s, e), (3 * K, 4 * K), (K * K - 1076, K * K)])
    assert batch.proofs()[0] == p and batch.one_namespace.tolist() == [1, 1, 1]
    assert batch.verify(ordered.root, ctx).tolist() == [0, 0, 0]
    batch.shares[RUN - 1, 300] ^= 1        # the last share of the first range
    assert batch.verify(ordered.root, ctx).tolist() == [2, 0, 0]


@pytest.mark.gpu
def test_whole_square_as_one_share_range(ctx):
    """Every share of a square under one namespace, proven as one range of
    1 024 whole rows: ShareProof.Validate as the oracle restates it rebuilds
    every row root from the shares and the data root from the row roots."""
    from celestia_da import proof as gpr
    from test_share_proof_validate import to_dict
    one = ods(0).copy()
    one[:, :29] = one[0, :29]
    sq = gpr.ResidentSquare(one, ctx)
    try:
        rows, _, root = sq.dah()
        batch = sq.share_proofs_batch([(0, K * K)])
        assert batch.seg_off.tolist() == [0, K] and len(batch.nodes) == K and len(batch.aunts) == 12 * K
        assert np.array_equal(batch.shares, one) and batch.row_roots.tobytes() == b"".join(rows[:K])
        assert batch.verify(root, ctx).tolist() == [0]
        assert opr.share_proof_validate(to_dict(batch.proofs()[0]), root) is None
        batch.shares[K * K - 1, 511] ^= 1
        assert batch.verify(root, ctx).tolist() == [2]
    finally:
        sq.close()


# ---------------------------------------------------------------------------
# 5. the edges of the supported range
# ---------------------------------------------------------------------------
def test_host_plans_take_1024_and_reject_2048():
    from celestia_da import proof as gpr
    p = gpr.share_proofs_plan(K, [(0, K * K), (K - 1, K + 1)])
    assert p["n_segments"] == K + 2 and p["aunts_per_segment"] == 12 and p["n_shares"] == K * K + 2
    assert p["n_nodes"] == K + 2 * 11
    c = gpr.commitment_proofs_plan(K, [K // 2], [3 * K], 64)
    assert c["n_segments"] == 4 and c["aunts_per_segment"] == 12
    assert _lib.split_layout(K, 8)["R"] == K // 8
    for call in (lambda: gpr.share_proofs_plan(2 * K, [(0, 1)]), lambda: gpr.commitment_proofs_plan(2 * K, [0], [1], 64)):
        with pytest.raises(CdaError) as e:
            call()
        assert e.value.code == _lib.CDA_ERR_INVALID and str(e.value) == "square width 2048 is not a power of two <= 1024"
    with pytest.raises(CdaError):
        _lib.split_layout(2 * K, 8)


@pytest.mark.gpu
def test_calls_that_do_not_take_k1024(ctx):
    """Repair, Reed-Solomon decoding and the fraud proofs stop at k = 512:
    status and text of each at W = 2 048 / 1 024 shards.  Every check comes
    before a buffer is read, so the buffers here are a few bytes."""
    import torch
    lib, tiny = ctx.lib, np.zeros(64, dtype=np.uint8)
    d_tiny = torch.zeros(64, dtype=torch.uint8, device="cuda")
    i32, u32 = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    pi32, pu32 = i32.ctypes.data_as(C.POINTER(C.c_int32)), u32.ctypes.data_as(C.POINTER(C.c_uint32))

    def rejected(rc, code, text):
        assert rc == code and lib.cda_last_error(ctx.h).decode() == text, (rc, lib.cda_last_error(ctx.h).decode())

    inv, uns = _lib.CDA_ERR_INVALID, _lib.CDA_ERR_UNSUPPORTED
    rejected(lib.cda_repair(ctx.h, ptr(tiny), ptr(tiny), W, ptr(tiny), ptr(tiny), pi32, pu32), inv, EDS_WIDTH)
    rejected(lib.cda_repair_device(ctx.h, d_tiny.data_ptr(), ptr(tiny), W, ptr(tiny), ptr(tiny), pi32, pu32), inv, EDS_WIDTH)
    rejected(lib.cda_repair_batch(ctx.h, ptr(tiny), ptr(tiny), W, 1, ptr(tiny), ptr(tiny), pi32, pi32, pu32), inv, EDS_WIDTH)
    rejected(lib.cda_repair_batch_device(ctx.h, d_tiny.data_ptr(), ptr(tiny), W, 1, ptr(tiny), ptr(tiny), pi32, pi32, pu32),
             inv, EDS_WIDTH)
    assert lib.cda_repair_batch_plan(ptr(tiny), W, 1, pu32, None, None, None, None) == inv
    assert lib.cda_last_error(None).decode() == EDS_WIDTH
    rejected(lib.cda_rs_decode(ctx.h, ptr(tiny), ptr(tiny), K, 64, 1), uns, "shard count must be a power of two <= 512")
    rejected(lib.cda_befp_build(ctx.h, ptr(tiny), W, 0, 0, ptr(tiny), ptr(tiny), pu32, pu32, ptr(tiny), ptr(tiny)), inv, EDS_WIDTH)
    rejected(lib.cda_befp_build_device(ctx.h, d_tiny.data_ptr(), W, 0, 0, ptr(tiny), ptr(tiny), pu32, pu32, ptr(tiny), ptr(tiny)),
             inv, EDS_WIDTH)
    b = _lib.BefpBatch()
    b.n_proofs, b.k = 1, K
    rejected(lib.cda_befp_verify(ctx.h, C.byref(b), ptr(tiny), None), inv, "k 1024 is not a power of two <= 512")
    assert lib.cda_befp_batch_check(C.byref(b)) == inv
    assert not tiny.any() and not d_tiny.any()


@pytest.mark.gpu
def test_every_width_check_rejects_2048(ctx):
    """Each call that takes k = 1024 refuses k = 2048, before it reads a
    buffer or stages a byte (the buffers here are a few bytes)."""
    import torch
    lib, tiny = ctx.lib, np.zeros(64, dtype=np.uint8)
    d = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
    u32 = np.zeros(2, dtype=np.uint32)
    pu32 = u32.ctypes.data_as(C.POINTER(C.c_uint32))
    k2, n2, inv = 2 * K, 4 * K * K, _lib.CDA_ERR_INVALID
    h = C.c_void_p()
    ns_batch = _lib.NamespaceProofBatch()
    calls = {
        "cda_extend_shares": lambda: lib.cda_extend_shares(ctx.h, ptr(tiny), n2, ptr(tiny)),
        "cda_extend_dah": lambda: lib.cda_extend_dah(ctx.h, ptr(tiny), n2, ptr(tiny), ptr(tiny), ptr(tiny), ptr(tiny)),
        "cda_dah_from_eds": lambda: lib.cda_dah_from_eds(ctx.h, ptr(tiny), 2 * k2, ptr(tiny), ptr(tiny), ptr(tiny)),
        "cda_extend_dah_batch": lambda: lib.cda_extend_dah_batch(ctx.h, ptr(tiny), k2, 1, ptr(tiny), ptr(tiny), ptr(tiny),
                                                                 ptr(tiny), None),
        "cda_extend_dah_batch_ex": lambda: lib.cda_extend_dah_batch_ex(ctx.h, ptr(tiny), k2, 1, ptr(tiny), 0, ptr(tiny),
                                                                       ptr(tiny), ptr(tiny), None),
        "cda_extend_dah_device": lambda: lib.cda_extend_dah_device(ctx.h, d, k2, 1, d, d, d, d, None, None),
        "cda_extend_dah_inplace_device": lambda: lib.cda_extend_dah_inplace_device(ctx.h, k2, 1, d, d, d, d, None, None),
        "cda_reserve": lambda: lib.cda_reserve(ctx.h, k2, 1),
        "cda_square_create": lambda: lib.cda_square_create(ctx.h, ptr(tiny), n2, C.byref(h)),
        "cda_square_set_create": lambda: lib.cda_square_set_create(ctx.h, ptr(tiny), _lib.CDA_SET_FROM_ODS, k2, 1, C.byref(h)),
        "cda_square_set_create_device": lambda: lib.cda_square_set_create_device(ctx.h, d, _lib.CDA_SET_FROM_EDS, k2, 1, None,
                                                                                 C.byref(h)),
        "cda_sample_proofs_verify": lambda: lib.cda_sample_proofs_verify(ctx.h, k2, 1, ptr(tiny), pu32, pu32, ptr(tiny),
                                                                         ptr(tiny), ptr(tiny), ptr(tiny), ptr(tiny),
                                                                         ptr(tiny), ptr(tiny)),
        "cda_namespace_proofs_verify": lambda: lib.cda_namespace_proofs_verify(ctx.h, k2, ptr(tiny), C.byref(ns_batch),
                                                                               ptr(tiny)),
    }
    for name, call in calls.items():
        assert call() == inv, name
        assert lib.cda_last_error(ctx.h).decode() == TOO_WIDE, (name, lib.cda_last_error(ctx.h).decode())
        assert not h.value, name
    assert lib.cda_split_rows(ctx.h, d, k2, 1, 0, d, d, None) == inv
    assert lib.cda_last_error(ctx.h).decode() == "bad row block"
    assert lib.cda_split_cols(ctx.h, d, k2, 2, 0, d, d, d, None) == inv
    assert lib.cda_last_error(ctx.h).decode() == "bad column block"
    assert lib.cda_data_root(ctx.h, ptr(tiny), ptr(tiny), 2 * W, ptr(tiny)) == _lib.CDA_ERR_UNSUPPORTED
    assert lib.cda_last_error(ctx.h).decode() == "more than 2048 roots per axis"
    assert not tiny.any()
