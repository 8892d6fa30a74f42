"""Verification of share and row proofs on the GPU: ShareProof.Validate /
VerifyProof and RowProof.Validate (pkg/proof/share_proof.go:16-82,
row_proof.go:13-51) through cda_share_proofs_verify and
celestia_da.proof.{ShareProof.validate, RowProof.validate,
validate_share_proofs, nmt_verify_inclusion}.

The checker is the oracle's restatement (oracle/proofs.py
share_proof_validate, row_proof_validate, nmt_range_proof), pinned by the
reference's own vector (tests/golden/share_proof_valid.json).

Validate takes ONE namespace per proof and hashes every share under it, so a
range that spans several namespaces fails with "share proof failed to verify"
in the reference.  testfactory's random squares give every share a namespace
of its own; where a test needs every range of a square to be valid, the
square therefore carries one namespace in all its shares (one_namespace).
Ranges of a constructed square that span several namespaces are kept and must
give the oracle's answer, which is that error.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import proofs as opr
import pyref
from celestia_da import _lib, testfactory
from celestia_da import proof as gpr
from test_share_proof_validate import fixture, to_dict

ROW = "row proof failed to verify"
SHARE = "share proof failed to verify"


def from_dict(d) -> gpr.ShareProof:
    rp = d["row_proof"]
    return gpr.ShareProof(
        data=d["data"], share_proofs=[gpr.NMTProof(p["start"], p["end"], list(p["nodes"])) for p in d["share_proofs"]],
        namespace_id=d["namespace_id"], namespace_version=d["namespace_version"],
        row_proof=gpr.RowProof(list(rp["row_roots"]),
                               [gpr.Proof(q["total"], q["index"], q["leaf_hash"], list(q["aunts"])) for q in rp["proofs"]],
                               rp["start_row"], rp["end_row"]))


def one_namespace(k, index):
    """testfactory's random square with the first share's namespace written
    over every share (still namespace ordered)."""
    ods = testfactory.random_square(k, index).copy()
    ods[:, :29] = ods[0, :29]
    return ods


def flip(b: bytes, byte: int, bit: int = 0) -> bytes:
    a = bytearray(b)
    a[byte] ^= 1 << bit
    return bytes(a)


# ------------------------------------------------------------------ CPU tests
def test_structural_cases_need_no_gpu():
    """TestShareProofValidate / TestRowProofValidate's structural cases: the
    reference's text, the oracle's, with no GPU touched."""
    d, root = fixture()
    s0 = d["share_proofs"][0]["start"]

    def share_case(mut):
        bad = copy.deepcopy(d)
        mut(bad)
        return bad

    def doubled_proofs(b):
        b["share_proofs"] = b["share_proofs"] * 2

    def doubled_data(b):
        b["data"] = b["data"] * 2

    def negative_start(b):
        b["share_proofs"][0].update(start=-1, end=0)

    def end_not_above_start(b):   # two rows whose counts still add up to the one share
        b["share_proofs"] = [dict(b["share_proofs"][0], start=s0, end=s0 + 2), dict(b["share_proofs"][0], start=s0, end=s0 - 1)]
        b["row_proof"]["row_roots"] = b["row_proof"]["row_roots"] * 2

    cases = [
        (lambda b: b.update(data=[]), "empty share proof"),
        (doubled_proofs, "the number of share proofs 2 must equal the number of row roots 1"),
        (doubled_data, "the number of shares 2 must equal the number of shares in share proofs 1"),
        (negative_start, "proof index cannot be negative"),
        (end_not_above_start, "proof total must be positive"),
    ]
    for mut, want in cases:
        bad = share_case(mut)
        assert opr.share_proof_validate(bad, root) == want
        with pytest.raises(ValueError) as e:
            from_dict(bad).validate(root)
        assert str(e.value) == want
        assert gpr.validate_share_proofs([from_dict(bad)], [root]) == [want]
    for field, value, want in [
        ("row_roots", [], "the number of rows 1 must equal the number of row roots 0"),
        ("proofs", [], "the number of proofs 0 must equal the number of row roots 1"),
        ("end_row", 10, "the number of rows 11 must equal the number of row roots 1"),
    ]:
        bad = copy.deepcopy(d["row_proof"])
        bad[field] = value
        assert opr.row_proof_validate(bad, root) == want
        rp = from_dict(dict(d, row_proof=bad)).row_proof
        with pytest.raises(ValueError) as e:
            rp.validate(root)
        assert str(e.value) == want
    # a mismatch inside the row proof surfaces through ShareProof.validate after its own checks
    bad = copy.deepcopy(d)
    bad["row_proof"]["end_row"] = 10
    with pytest.raises(ValueError) as e:
        from_dict(bad).validate(root)
    assert str(e.value) == opr.share_proof_validate(bad, root) == "the number of rows 11 must equal the number of row roots 1"


# ------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def squares(ctx):
    """Resident squares shared by the GPU tests: name -> (square, data root)."""
    from test_proofs import constructed_square
    out = {}
    for name, ods in (("k2", one_namespace(2, 1)), ("k4", one_namespace(4, 2)), ("k128", one_namespace(128, 3))):
        sq = gpr.ResidentSquare(ods, ctx)
        out[name] = (sq, sq.dah()[2], ods.reshape(-1, 512), None)
    ods, k, blobs = constructed_square(3, 16, 8, (1, 6000))
    assert k == 16
    sq = gpr.ResidentSquare(ods, ctx)
    out["k16"] = (sq, sq.dah()[2], ods.reshape(-1, 512), blobs)
    yield out
    for sq, _, _, _ in out.values():
        sq.close()


def all_ranges(k):
    return [(s, e) for s in range(k * k) for e in range(s + 1, k * k + 1)]


@pytest.mark.gpu
def test_reference_vector(ctx):
    """The reference's own proof: 33-byte namespace, 98-byte nodes, total 128, 7 aunts."""
    d, root = fixture()
    p = from_dict(d)
    assert len(p.namespace_id) == 32 and len(p.share_proofs[0].nodes[0]) == 98
    assert p.validate(root, ctx) is None
    assert p.verify_proof(ctx) is True
    assert p.row_proof.validate(root, ctx) is None
    with pytest.raises(ValueError) as e:
        p.validate(bytes(32), ctx)
    assert str(e.value) == ROW == opr.share_proof_validate(d, bytes(32))
    with pytest.raises(ValueError) as e:
        p.row_proof.validate(bytes(32), ctx)
    assert str(e.value) == ROW
    bad = copy.deepcopy(d)
    bad["namespace_version"] = 256
    assert from_dict(bad).verify_proof(ctx) is False
    assert gpr.validate_share_proofs([from_dict(bad)], [root], ctx) == [SHARE] == [opr.share_proof_validate(bad, root)]


@pytest.mark.gpu
def test_round_trip_one_batch(ctx, squares):
    """Every range of a k = 2 and a k = 4 square and test_proofs' ranges of a
    constructed k = 16 square in ONE call: 1-row, 2-row and k-row proofs."""
    from test_proofs import ranges
    proofs, roots, single_ns = [], [], []
    for name, k in (("k2", 2), ("k4", 4)):
        sq, root, shares, _ = squares[name]
        for s, e in all_ranges(k):
            proofs.append(sq.share_proof(bytes(shares[s][:29]), s, e))
            roots.append(root)
            single_ns.append(True)
    sq, root, shares, blobs = squares["k16"]
    assert blobs
    for s, e in ranges(16, blobs):
        proofs.append(sq.share_proof(bytes(shares[s][:29]), s, e))
        roots.append(root)
        single_ns.append(len({bytes(shares[i][:29]) for i in range(s, e)}) == 1)
    assert {len(p.share_proofs) for p in proofs} >= {1, 2, 4, 16}
    got = gpr.validate_share_proofs(proofs, roots, ctx)
    want = [opr.share_proof_validate(to_dict(p), r) for p, r in zip(proofs, roots)]
    assert got == want
    # one namespace: valid; several: the reference hashes every share under the proof's one namespace
    assert all((g is None) == one for g, one in zip(got, single_ns))
    assert sum(single_ns) >= len(all_ranges(2)) + len(all_ranges(4)) + 3 and SHARE in got


@pytest.mark.gpu
def test_two_squares_in_one_batch(ctx, squares):
    (a, root_a, sh_a, _), (b, root_b, sh_b, _) = squares["k2"], squares["k4"]
    assert root_a != root_b
    pa = [a.share_proof(bytes(sh_a[0][:29]), s, e) for s, e in all_ranges(2)]
    pb = [b.share_proof(bytes(sh_b[0][:29]), s, e) for s, e in all_ranges(4)[::13]]
    proofs, roots = [], []
    for i in range(max(len(pa), len(pb))):
        for lst, r in ((pa, root_a), (pb, root_b)):
            if i < len(lst):
                proofs.append(lst[i])
                roots.append(r)
    assert gpr.validate_share_proofs(proofs, roots, ctx) == [None] * len(proofs)
    swapped = [i for i in range(len(proofs)) if i % 3 == 1]
    other = {root_a: root_b, root_b: root_a}
    roots2 = [other[r] if i in swapped else r for i, r in enumerate(roots)]
    got = gpr.validate_share_proofs(proofs, roots2, ctx)
    assert got == [ROW if i in swapped else None for i in range(len(proofs))]
    assert got == [opr.share_proof_validate(to_dict(p), r) for p, r in zip(proofs, roots2)]


def two_row_blob_range(blobs, k):
    for s, n, _, _ in blobs:
        if (s + n - 1) // k - s // k == 1 and s % k and (s + n) % k:
            return s, s + n
    raise AssertionError("no blob over exactly two rows")


def mutants(d, root):
    """(name, proof dict, root) of every tampering of the valid two-row proof d."""
    out = []

    def add(name, mut, r=root):
        bad = copy.deepcopy(d)
        mut(bad)
        out.append((name, bad, r))

    sp0 = d["share_proofs"][0]
    n_left = bin(sp0["start"]).count("1")
    assert 0 < n_left < len(sp0["nodes"])   # nodes on both sides of the first row's range
    ns = 29

    def share_byte(b): b["data"][1] = flip(b["data"][1], 300, 3)
    def left_digest(b): b["share_proofs"][0]["nodes"][0] = flip(b["share_proofs"][0]["nodes"][0], 2 * ns + 5)
    def right_min_ns(b): b["share_proofs"][0]["nodes"][n_left] = flip(b["share_proofs"][0]["nodes"][n_left], 28)
    def row_root(b): b["row_proof"]["row_roots"][1] = flip(b["row_proof"]["row_roots"][1], 70, 7)
    def leaf_hash(b): b["row_proof"]["proofs"][0]["leaf_hash"] = flip(b["row_proof"]["proofs"][0]["leaf_hash"], 31)
    def aunt(b): b["row_proof"]["proofs"][1]["aunts"][2] = flip(b["row_proof"]["proofs"][1]["aunts"][2], 0, 6)
    def index(b): b["row_proof"]["proofs"][0]["index"] ^= 1
    def total(b): b["row_proof"]["proofs"][1]["total"] *= 2
    def shifted(b): b["share_proofs"][1].update(start=b["share_proofs"][1]["start"] + 1, end=b["share_proofs"][1]["end"] + 1)
    def swapped(b):
        n = b["share_proofs"][0]["nodes"]
        n[0], n[-1] = n[-1], n[0]
    def appended(b): b["share_proofs"][1]["nodes"].append(b["share_proofs"][1]["nodes"][-1])
    def aunt_dropped(b): b["row_proof"]["proofs"][0]["aunts"].pop()

    for f in (share_byte, left_digest, right_min_ns, row_root, leaf_hash, aunt):
        add(f.__name__, f)
    add("data_root", lambda b: None, flip(root, 9, 2))
    for f in (index, total, shifted, swapped, appended, aunt_dropped):
        add(f.__name__, f)
    return out


@pytest.mark.gpu
def test_tampering_interleaved_with_valid(ctx, squares):
    sq, root, shares, blobs = squares["k16"]
    s, e = two_row_blob_range(blobs, 16)
    p = sq.share_proof(bytes(shares[s][:29]), s, e)
    d = to_dict(p)
    assert len(p.share_proofs) == 2 and opr.share_proof_validate(d, root) is None
    ms = mutants(d, root)
    assert len(ms) == 13
    proofs, roots, want = [], [], []
    for name, bad, r in ms:
        proofs += [from_dict(bad), p]
        roots += [r, root]
        w = opr.share_proof_validate(bad, r)
        assert w in (ROW, SHARE), name
        want += [w, None]
    got = gpr.validate_share_proofs(proofs, roots, ctx)
    for (name, _, _), g, w in zip(ms, got[0::2], want[0::2]):
        assert g == w, name
    assert got[1::2] == [None] * len(ms)
    # the oracle's restatement raises on a truncated node list, so this one is asserted directly
    bad = copy.deepcopy(d)
    bad["share_proofs"][0]["nodes"].pop()
    assert gpr.validate_share_proofs([p, from_dict(bad), p], [root] * 3, ctx) == [None, SHARE, None]
    # fields of the wrong length are answered as Validate would
    short_node, short_aunt = copy.deepcopy(d), copy.deepcopy(d)
    short_node["share_proofs"][1]["nodes"][0] = short_node["share_proofs"][1]["nodes"][0][:-1]
    short_aunt["row_proof"]["proofs"][0]["aunts"][0] = short_aunt["row_proof"]["proofs"][0]["aunts"][0][:-1]
    both = copy.deepcopy(short_node)
    both["row_proof"]["proofs"][0]["index"] ^= 1
    assert gpr.validate_share_proofs([from_dict(x) for x in (short_node, short_aunt, both)], [root] * 3, ctx) == \
        [SHARE, ROW, ROW]


@pytest.mark.gpu
def test_wave_boundaries(ctx, squares):
    """128 leaves in a segment, 65 leaves across lane 64, two-leaf segments around lane 63 / 64."""
    sq, root, shares, _ = squares["k128"]
    ns = bytes(shares[0][:29])
    proofs = [sq.share_proof(ns, s, e) for s, e in ((0, 128), (3, 68), (127, 129), (128 * 5 + 63, 128 * 5 + 65))]
    assert [len(p.share_proofs) for p in proofs] == [1, 1, 2, 1]
    got = gpr.validate_share_proofs(proofs, [root] * 4, ctx)
    assert got == [None] * 4 == [opr.share_proof_validate(to_dict(p), root) for p in proofs]
    for p in proofs:
        assert p.verify_proof(ctx) is True
    bad = copy.deepcopy(proofs[1])
    bad.data[64] = flip(bad.data[64], 511, 7)     # the leaf of lane 64
    assert gpr.validate_share_proofs([bad], [root], ctx) == [SHARE]


def prove_range(ctx, cells, square_size, start, end):
    n = len(cells)
    flat = np.frombuffer(b"".join(cells), dtype=np.uint8)
    nodes = np.zeros(64 * 90, dtype=np.uint8)
    cnt = C.c_uint32()
    root = np.zeros(90, dtype=np.uint8)
    ctx.check(ctx.lib.cda_nmt_prove_range(ctx.h, _lib.ptr(flat), len(cells[0]), n, square_size, 0, start, end,
                                          _lib.ptr(nodes), C.byref(cnt), _lib.ptr(root)))
    nb = nodes.tobytes()
    return [nb[90 * i:90 * (i + 1)] for i in range(cnt.value)], root.tobytes()


def axis_root(ctx, cells, square_size):
    flat = np.frombuffer(b"".join(cells), dtype=np.uint8)
    root = np.zeros(90, dtype=np.uint8)
    ctx.check(ctx.lib.cda_nmt_axis_root(ctx.h, _lib.ptr(flat), len(cells[0]), len(cells), square_size, 0, _lib.ptr(root)))
    return root.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("cell_len,counts", [(512, (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)), (64, (5, 12))])
def test_non_power_of_two_trees(ctx, cell_len, counts):
    """The NMT half alone against cda_nmt_prove_range, trees of any leaf
    count (512-byte cells: the 29-byte leaf path; 64-byte cells: the generic one)."""
    ns = b"\x00" * 19 + b"\x07" * 10
    rnd = np.random.default_rng(11)
    cells = [ns + rnd.integers(0, 256, cell_len - 29, dtype=np.uint8).tobytes() for _ in range(13)]
    for n in counts:
        other = axis_root(ctx, cells[:n + 1], 8)
        for s in range(min(n, 8)):
            for e in range(s + 1, min(n, 8) + 1):
                nodes, root = prove_range(ctx, cells[:n], 8, s, e)
                assert root != other
                assert gpr.nmt_verify_inclusion(root, nodes, s, e, ns, cells[s:e], ctx) is True, (n, s, e)
                assert gpr.nmt_verify_inclusion(other, nodes, s, e, ns, cells[s:e], ctx) is False, (n, s, e)


@pytest.mark.gpu
@pytest.mark.parametrize("ns_len", [13, 14])
def test_byte_node_padding_edges(ctx, ns_len):
    """The byte-addressed path (any namespace length) at the SHA-256 padding
    edges: 41-byte shares under a 13- / 14-byte namespace give leaf messages of
    55 / 56 bytes (the 0x80 and bit count fit the block / spill into a second)
    and node messages 0x01 || l || r of 117 / 121 bytes (two blocks / a
    third).  Trees of 5 and 8 leaves built with the oracle's hashers, every
    range: the verdicts of the oracle for the proof and for the proof with one
    byte of one node flipped."""
    nid = bytes(range(0x30, 0x30 + ns_len))
    rnd = np.random.default_rng(ns_len)
    shares = [rnd.integers(0, 256, 41, dtype=np.uint8).tobytes() for _ in range(8)]
    leaf_nodes = [opr._nmt_leaf(ns_len, nid + s) for s in shares]
    assert len(nid + shares[0]) + 1 == 42 + ns_len and 2 * len(leaf_nodes[0]) + 1 == (117, 121)[ns_len - 13]

    for n in (5, 8):
        def subtree(lo, hi):
            if hi - lo == 1:
                return leaf_nodes[lo]
            k = opr.split_point(hi - lo)
            return opr._nmt_node(ns_len, subtree(lo, lo + k), subtree(lo + k, hi))

        def prove(lo, hi, s, e, out):
            if hi <= s or lo >= e:
                out.append(subtree(lo, hi))
            elif hi - lo > 1:
                k = opr.split_point(hi - lo)
                prove(lo, lo + k, s, e, out)
                prove(lo + k, hi, s, e, out)
            return out

        root = subtree(0, n)
        for s in range(n):
            for e in range(s + 1, n + 1):
                nodes = prove(0, n, s, e, [])
                want = opr.nmt_verify_inclusion(root, nodes, s, e, nid, shares[s:e])
                assert want is True, (n, s, e)
                assert gpr.nmt_verify_inclusion(root, nodes, s, e, nid, shares[s:e], ctx) is want, (n, s, e)
                if not nodes:
                    continue
                q = (s + e) % len(nodes)
                bad = nodes[:q] + [flip(nodes[q], (7 * s + 3 * e) % len(nodes[q]), e % 8)] + nodes[q + 1:]
                want = opr.nmt_verify_inclusion(root, bad, s, e, nid, shares[s:e])
                assert want is False, (n, s, e)
                assert gpr.nmt_verify_inclusion(root, bad, s, e, nid, shares[s:e], ctx) is want, (n, s, e)


def raw_call(ctx, b):
    verdict = np.full(4, 255, dtype=np.uint8)
    rc = ctx.lib.cda_share_proofs_verify(ctx.h, C.byref(b), _lib.ptr(verdict))
    return rc, ctx.lib.cda_last_error(ctx.h).decode(), verdict


@pytest.mark.gpu
def test_width_bound_and_invalid_batches(ctx):
    """CDA_VERIFY_MAX_LEAVES: a 2 048-leaf row verifies; past it, and for
    inconsistent offsets / counts, the call is CDA_ERR_INVALID, never a verdict."""
    ns = b"\x00" * 19 + b"\x09" * 10
    rnd = np.random.default_rng(5)
    shares = [rnd.integers(0, 256, 512, dtype=np.uint8).tobytes() for _ in range(2048)]
    leaf_nodes = [pyref.nmt_hash_leaf(ns + s) for s in shares]
    root = pyref.nmt_root_from_nodes(leaf_nodes)
    nodes = opr.nmt_range_proof(leaf_nodes, 1024, 2048)
    assert gpr.nmt_verify_inclusion(root, nodes, 1024, 2048, ns, shares[1024:], ctx) is True
    assert gpr.nmt_verify_inclusion(root, nodes, 1024, 2048, ns, shares[1025:] + shares[:1], ctx) is False

    nodes0 = opr.nmt_range_proof(leaf_nodes, 0, 1)

    def batch():   # two proofs of one row each
        entries = [(ns, None, [(0, 1, nodes0, root, None)], shares[:1]),
                   (ns, None, [(1024, 2048, nodes, root, None)], shares[1024:])]
        return gpr._build_batch(29, 512, entries, rows=False, nmt=True)

    b, keep = batch()
    rc, msg, verdict = raw_call(ctx, b)
    assert (rc, msg, verdict.tolist()) == (_lib.CDA_OK, "", [0, 0, 255, 255])
    for field, where, mut in [
        ("nmt_end", "proof 1", lambda b: b.nmt_end.__setitem__(1, 2049)),
        ("node_off", "proof 1", lambda b: b.node_off.__setitem__(1, b.node_off[2] + 1)),   # [0, 13, 12]: decreasing
        ("n_shares", "", lambda b: setattr(b, "n_shares", b.n_shares - 1)),
        ("ns_len", "", lambda b: setattr(b, "ns_len", 0)),
    ]:
        b, keep = batch()
        mut(b)
        rc, msg, verdict = raw_call(ctx, b)
        assert rc == _lib.CDA_ERR_INVALID and field in msg and where in msg, (field, rc, msg)
        assert verdict.tolist() == [255] * 4, field
    del keep


@pytest.mark.gpu
def test_empty_batch(ctx):
    rc, msg, verdict = raw_call(ctx, _lib.ShareProofBatch())
    assert (rc, msg) == (_lib.CDA_OK, "") and verdict.tolist() == [255] * 4
