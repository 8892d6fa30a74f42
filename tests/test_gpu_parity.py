"""GPU parity: libcda.so (HIP, gfx950) against the CPU oracle and the
reference's golden vectors.  Bit-exact for every byte (integer path)."""
import hashlib

import numpy as np
import pytest

import coracle
import pyref
from celestia_da import PushOrderError, da, rsmt2d

pytestmark = pytest.mark.gpu

GOLDEN_K2 = "b56e4d251ac266f4b91cc5464b3fc7efcbdc888064647496d13133f0dc65ac25"
GOLDEN_K128 = "0bd3abeeacfbb0b92dfbdac4a154868e3c4e79666f7fcf6c620bb90dd3a0dcf0"
GOLDEN_MIN = "3d96b7d238e7e0456f6af8e7cdf0a67bd6cf9c2089ecb559c659dcaa1f880353"


def test_min_dah_golden(ctx):
    # pkg/da/data_availability_header_test.go:27-32
    dah = da.min_data_availability_header()
    assert dah.hash().hex() == GOLDEN_MIN
    dah.validate_basic()
    assert dah.square_size() == 1


@pytest.mark.parametrize("k,expected", [(2, GOLDEN_K2), (128, GOLDEN_K128)])
def test_new_dah_golden(ctx, k, expected):
    # pkg/da/data_availability_header_test.go:34-68 (constant shares)
    shares = pyref.constant_shares(k * k)
    eds = da.extend_shares(shares)
    dah = da.new_data_availability_header(eds)
    assert len(dah.row_roots) == 2 * k and len(dah.column_roots) == 2 * k
    assert dah.hash().hex() == expected


def test_nil_dah_hash(ctx):
    assert da.DataAvailabilityHeader().hash().hex() == hashlib.sha256(b"").hexdigest()


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 32, 64, 128])
def test_random_square_parity(ctx, k):
    ods = coracle.random_square(k, k)
    eds = da.extend_shares(ods)
    dah = da.new_data_availability_header(eds)
    e_eds, e_rows, e_cols, e_root = coracle.cpu_baseline(ods, 8) if k >= 64 else coracle.extend_dah(ods)
    assert np.array_equal(eds.array().reshape(-1, 512), e_eds)
    assert dah.row_roots == [bytes(r) for r in e_rows]
    assert dah.column_roots == [bytes(c) for c in e_cols]
    assert dah.hash() == e_root


@pytest.mark.parametrize("k", [256, 512])
def test_gf16_square_parity(ctx, k):
    ods = coracle.random_square(k, 1)
    eds = da.extend_shares(ods)
    dah = da.new_data_availability_header(eds)
    e_eds, e_rows, e_cols, e_root = coracle.cpu_baseline(ods, 16)
    assert np.array_equal(eds.array().reshape(-1, 512), e_eds)
    assert dah.hash() == e_root
    assert dah.row_roots == [bytes(r) for r in e_rows]


def test_batch_matches_single(ctx):
    k, n = 32, 6
    ods = np.stack([coracle.random_square(k, i) for i in range(n)])
    eds, rows, cols, roots, status = da.extend_dah_batch(ods)
    assert (status == 0).all()
    for i in range(n):
        e_eds, e_rows, e_cols, e_root = coracle.extend_dah(ods[i])
        assert np.array_equal(eds[i].reshape(-1, 512), e_eds)
        assert np.array_equal(rows[i], e_rows) and np.array_equal(cols[i], e_cols)
        assert roots[i].tobytes() == e_root


@pytest.mark.parametrize("k", [2, 4, 8, 16, 32, 64, 128, 256, 512])
@pytest.mark.parametrize("length", [64, 512, 1024])
def test_codec_encode(ctx, k, length):
    rng = np.random.default_rng(k * 7 + length)
    data = rng.integers(0, 256, (k, length), dtype=np.uint8)
    got = rsmt2d.LeoRSCodec().encode(data)
    assert np.array_equal(got, coracle.leopard_encode(data))


def test_codec_chunk_size_error(ctx):
    with pytest.raises(Exception, match="multiple of 64"):
        rsmt2d.LeoRSCodec().encode(np.zeros((4, 100), dtype=np.uint8))


def test_extend_shares_errors(ctx):
    # pkg/da/data_availability_header_test.go:70-99
    with pytest.raises(ValueError, match="not a power of 2"):
        da.extend_shares(pyref.constant_shares(129 * 129))
    with pytest.raises(ValueError, match="not a power of 2"):
        da.extend_shares(pyref.constant_shares(5))
    # a power of two that is not a square passes ExtendShares' check and fails
    # in rsmt2d's newDataSquare -- in the Python mirror and in the C ABI
    with pytest.raises(ValueError, match="number of chunks must be a square number"):
        da.extend_shares(pyref.constant_shares(8))
    from celestia_da._lib import CDA_ERR_INVALID, CDA_ERR_NOT_POW2, ptr
    eds = np.empty(16 * 512, dtype=np.uint8)
    for n, code, text in [(8, CDA_ERR_INVALID, "number of chunks must be a square number"),
                          (5, CDA_ERR_NOT_POW2, "number of shares is not a power of 2: got 5")]:
        ods = np.frombuffer(b"".join(pyref.constant_shares(n)), dtype=np.uint8).copy()
        assert ctx.lib.cda_extend_shares(ctx.h, ptr(ods), n, ptr(eds)) == code
        assert ctx.lib.cda_last_error(ctx.h).decode() == text


def test_push_order_error(ctx):
    k = 8
    ods = coracle.random_square(k, 3).reshape(k, k, 512).copy()
    ods[2, 5, :29], ods[2, 6, :29] = ods[2, 6, :29].copy(), ods[2, 5, :29].copy()   # break row 2
    eds = da.extend_shares(ods.reshape(-1, 512))
    with pytest.raises(PushOrderError, match="lexicographically ordered"):
        da.new_data_availability_header(eds)
    axis, idx, pos = ctx.push_order_detail()
    assert (axis, idx, pos) == (0, 2, 6)
    # the EDS itself is still produced (ExtendShares does not check order)
    assert np.array_equal(eds.array().reshape(-1, 512), coracle.extend(ods.reshape(-1, 512)))


def _first_violation(ods):
    """Brute-force nmt push-order check of the Q0 rows and columns: the
    smallest (axis, index, position) whose namespace is below its
    predecessor's (rows before columns), as cda_push_order_detail reports."""
    k = ods.shape[0]
    ns = [[bytes(ods[r, c, :29]) for c in range(k)] for r in range(k)]
    bad = [(0, r, c) for r in range(k) for c in range(1, k) if ns[r][c] < ns[r][c - 1]]
    bad += [(1, c, r) for c in range(k) for r in range(1, k) if ns[r][c] < ns[r - 1][c]]
    return min(bad) if bad else None


@pytest.mark.parametrize("case", ["row_last_pair", "col_last_row", "row_first_pair", "row_and_col", "last_col"])
def test_push_order_edges(ctx, case):
    """Round 5 moved the Q0 push-order check to the leaf kernel's first chunk:
    violations at the square's edges (first / last Q0 row and column, the
    boundary to the parity half) and several at once report the same first
    violation as a brute-force check, and the EDS is unchanged."""
    k = 16
    ods = coracle.random_square(k, 31).reshape(k, k, 512).copy()

    def swap(a, b):
        ods[a][:29], ods[b][:29] = ods[b][:29].copy(), ods[a][:29].copy()

    if case == "row_last_pair":
        swap((k - 1, k - 2), (k - 1, k - 1))
    elif case == "col_last_row":
        ods[k - 1, 0, :29] = ods[0, 0, :29]          # below its upper neighbour only
    elif case == "row_first_pair":
        swap((0, 0), (0, 1))
    elif case == "row_and_col":
        ods[k - 1, 0, :29] = ods[0, 0, :29]
        swap((5, 9), (5, 10))
    else:
        ods[1, k - 1, :29] = ods[0, 0, :29]          # last Q0 column, row 1
    want = _first_violation(ods)
    if want is None:
        pytest.skip("perturbation left the square ordered (equal namespaces)")
    eds = da.extend_shares(ods.reshape(-1, 512))
    with pytest.raises(PushOrderError):
        da.new_data_availability_header(eds)
    assert ctx.push_order_detail() == want
    assert np.array_equal(eds.array().reshape(-1, 512), coracle.extend(ods.reshape(-1, 512)))


def test_block408_on_gpu(ctx):
    """Mainnet block 408 (k=32): GPU data root == header.data_hash."""
    import gzip, json, os
    here = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(here, "golden", "golden.json")))["block408"]
    with gzip.open(os.path.join(here, "golden", "block408_ods.bin.gz")) as f:
        ods = np.frombuffer(f.read(), dtype=np.uint8).reshape(-1, 512).copy()
    eds = da.extend_shares(ods)
    dah = da.new_data_availability_header(eds)
    assert dah.hash().hex() == g["data_hash"]
    assert hashlib.sha256(eds.array().tobytes()).hexdigest() == g["eds_sha256"]


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 32, 64, 128])
def test_random_fixtures_on_gpu(ctx, k):
    import json, os
    here = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(here, "golden", "golden.json")))["random_squares"][str(k)]
    from celestia_da import testfactory
    ods = testfactory.random_square(k, g["seed_index"])
    assert hashlib.sha256(ods.tobytes()).hexdigest() == g["ods_sha256"]
    eds = da.extend_shares(ods)
    dah = da.new_data_availability_header(eds)
    assert hashlib.sha256(eds.array().tobytes()).hexdigest() == g["eds_sha256"]
    rows = np.array([np.frombuffer(r, dtype=np.uint8) for r in dah.row_roots])
    cols = np.array([np.frombuffer(c, dtype=np.uint8) for c in dah.column_roots])
    assert hashlib.sha256(rows.tobytes()).hexdigest() == g["row_roots_sha256"]
    assert hashlib.sha256(cols.tobytes()).hexdigest() == g["col_roots_sha256"]
    assert dah.hash().hex() == g["data_root"]


@pytest.mark.parametrize("k,parts", [(4, 2), (16, 4), (128, 8), (512, 8), (512, 2), (1024, 8), (1024, 2)])
def test_split_square_loopback_on_gpu(ctx, k, parts):
    """Config 5 kernels (row block -> column block -> subtree combine) on one
    GPU with `parts` virtual ranks: bit-exact EDS columns, roots, data root.
    k = 1024 (the widest square; its 4 096-root data root takes the two-launch
    form) runs square 0 against the oracle's digests in tests/golden/k1024.json."""
    import torch
    from celestia_da import dist as cdist
    ods = coracle.random_square(k, 0 if k == 1024 else 9)
    dev = torch.device("cuda", 0)
    ops = cdist.GpuSplitOps(ctx, dev)
    cols_eds, (rows, cols, root, err) = cdist.extend_dah_split_loopback(torch.from_numpy(ods).to(dev), k, parts, ops)
    torch.cuda.synchronize()
    if k == 1024:
        import json, os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1024.json")) as f:
            want = json.load(f)["squares"]["0"]
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
        assert int(err.item()) == 0xFFFFFFFF
        assert sha(ods) == want["ods_sha256"] and sha(cols_eds.cpu().numpy()) == want["eds_sha256"]
        assert sha(rows.cpu().numpy()) == want["row_roots_sha256"] and sha(cols.cpu().numpy()) == want["col_roots_sha256"]
        assert root.cpu().numpy().tobytes().hex() == want["data_root"]
        return
    e_eds, e_rows, e_cols, e_root = coracle.cpu_baseline(ods, 16) if k >= 64 else coracle.extend_dah(ods)
    assert int(err.item()) == 0xFFFFFFFF
    assert np.array_equal(cols_eds.cpu().numpy().reshape(-1, 512), e_eds)
    assert np.array_equal(cols.cpu().numpy(), e_cols)
    assert np.array_equal(rows.cpu().numpy(), e_rows)
    assert root.cpu().numpy().tobytes() == e_root


def test_split_push_order_on_gpu(ctx):
    import torch
    from celestia_da import dist as cdist
    k = 16
    ods = coracle.random_square(k, 4).reshape(k, k, 512).copy()
    ods[5, 9, :29], ods[5, 10, :29] = ods[5, 10, :29].copy(), ods[5, 9, :29].copy()
    dev = torch.device("cuda", 0)
    _, (_, _, _, err) = cdist.extend_dah_split_loopback(torch.from_numpy(ods.reshape(-1, 512)).to(dev), k, 4,
                                                         cdist.GpuSplitOps(ctx, dev))
    assert int(err.item()) == (0 << 24) | (5 << 12) | 10


@pytest.mark.parametrize("k,n", [(1, 2), (2, 3), (16, 2), (64, 2), (128, 3), (256, 1), (512, 1)])
def test_inplace_device_matches_device_entry(ctx, k, n):
    """cda_extend_dah_inplace_device (ODS already in Q0 of the EDS, no copy)
    gives the same EDS, roots, data roots and status as cda_extend_dah_device
    on the same squares; the last square is checked against the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    W = 2 * k
    ods = np.stack([coracle.random_square(k, 40 + i) for i in range(n)])
    if n > 1 and k >= 2:   # one square out of namespace order -> status set, bytes still equal
        sq = ods[0].reshape(k, k, 512)
        sq[0, 0, :29], sq[0, 1, :29] = sq[0, 1, :29].copy(), sq[0, 0, :29].copy()
    d_ods = torch.from_numpy(ods.reshape(n, k * k * 512)).to(dev)

    def outs():
        return (torch.zeros(n, W * W * 512, dtype=torch.uint8, device=dev),
                torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                torch.empty(n, 32, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev))

    stream = torch.cuda.current_stream(dev).cuda_stream
    a = outs()
    ctx.extend_dah_device(d_ods.data_ptr(), k, n, *[t.data_ptr() for t in a], stream)
    b = outs()
    b[0].view(n, W, W, 512)[:, :k, :k] = d_ods.view(n, k, k, 512)
    ctx.extend_dah_inplace_device(k, n, *[t.data_ptr() for t in b], stream)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if k <= 128:
        e_eds, e_rows, e_cols, e_root = coracle.extend_dah(ods[-1])
        assert np.array_equal(b[0][-1].cpu().numpy().reshape(-1, 512), e_eds)
        assert b[3][-1].cpu().numpy().tobytes() == e_root
    status = b[4].cpu().numpy()
    assert (status[1:] == 0).all()
    if n > 1 and k >= 2:
        assert status[0] != 0


def test_two_streams_share_context_scratch(ctx):
    """Two device calls on two streams of one context, enqueued back to back
    with no host sync: the context's scratch (leaf/level slots, digests, error
    words) is shared, so the second call's GPU work must wait for the first
    (Engine::order_begin / order_end).  Both results equal the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    k, n = 64, 3
    W = 2 * k
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    sets = []
    for base in (100, 200):
        ods = np.stack([coracle.random_square(k, base + i) for i in range(n)])
        sets.append((ods, torch.from_numpy(ods.reshape(n, -1)).to(dev),
                     torch.empty(n, W * W * 512, dtype=torch.uint8, device=dev),
                     torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                     torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                     torch.empty(n, 32, dtype=torch.uint8, device=dev)))
    torch.cuda.synchronize()
    for (ods, o, e, r, c, g), s in zip(sets, (s1, s2)):
        ctx.extend_dah_device(o.data_ptr(), k, n, e.data_ptr(), r.data_ptr(), c.data_ptr(), g.data_ptr(), None,
                              s.cuda_stream)
    torch.cuda.synchronize()
    for ods, o, e, r, c, g in sets:
        for i in range(n):
            e_eds, e_rows, e_cols, e_root = coracle.extend_dah(ods[i])
            assert np.array_equal(r[i].cpu().numpy().reshape(W, 90), e_rows)
            assert np.array_equal(c[i].cpu().numpy().reshape(W, 90), e_cols)
            assert g[i].cpu().numpy().tobytes() == e_root


def test_last_error_is_per_thread(ctx):
    """cda_last_error is the calling thread's message: two threads failing
    different calls on ONE context in a loop each read their own text."""
    import threading
    errs = []

    def worker(kind):
        for _ in range(40):
            try:
                if kind == 0:
                    rsmt2d.LeoRSCodec(ctx).encode(np.zeros((4, 100), dtype=np.uint8))
                else:
                    ctx.check(ctx.lib.cda_extend_shares(ctx.h, None, 5, None))
            except Exception as e:
                msg = str(e)
                ok = "multiple of 64" in msg if kind == 0 else "not a power of 2: got 5" in msg
                if not ok:
                    errs.append((kind, msg))
            else:
                errs.append((kind, "no error"))

    ts = [threading.Thread(target=worker, args=(i % 2,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert errs == []


def test_k512_matches_committed_oracle_digest(ctx):
    """Config 3 square 0 and 1 against tests/golden/k512.json (oracle digests,
    oracle/gen_config4.py --k 512)."""
    import json, os
    from celestia_da import testfactory
    here = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(here, "golden", "k512.json")))["squares"]
    for i in (0, 1):
        ods = testfactory.random_square(512, i)
        eds = da.extend_shares(ods)
        dah = da.new_data_availability_header(eds)
        assert hashlib.sha256(eds.array().tobytes()).hexdigest() == g[str(i)]["eds_sha256"]
        assert dah.hash().hex() == g[str(i)]["data_root"]


def test_k512_batch_of_32_matches_committed_oracle_digest(ctx):
    """32 k = 512 squares in ONE in-place submission (16 GiB EDS arena): the
    batch shape whose NMT levels run as a fused subtree launch down to the
    roots (no tree top) -- squares 0 and 1 of tests/golden/k512.json
    alternating, every data root and two whole EDSs against the oracle digests."""
    import json, os
    import torch
    from celestia_da import testfactory
    here = os.path.dirname(os.path.abspath(__file__))
    g = json.load(open(os.path.join(here, "golden", "k512.json")))["squares"]
    k, n = 512, 32
    W = 2 * k
    dev = torch.device("cuda", 0)
    eds = torch.empty((n, W, W, 512), dtype=torch.uint8, device=dev)
    for i in (0, 1):
        q0 = torch.from_numpy(testfactory.random_square(k, i)).to(dev).view(k, k, 512)
        eds[i::2, :k, :k] = q0
    rows = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    cols = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    roots = torch.empty(n, 32, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.extend_dah_inplace_device(k, n, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                  status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    dr = roots.cpu().numpy()
    assert [dr[p].tobytes().hex() for p in range(n)] == [g[str(p % 2)]["data_root"] for p in range(n)]
    for p in (0, n - 1):
        assert hashlib.sha256(eds[p].cpu().numpy().tobytes()).hexdigest() == g[str(p % 2)]["eds_sha256"], p
    del eds
    torch.cuda.empty_cache()


def test_k32_batch_of_1024_whole_tree_subtrees_match_single_squares(ctx):
    """1024 k = 32 squares in one in-place submission -- the shape whose NMT
    levels run as ONE subtree launch of whole 64-leaf trees that writes the
    roots itself (no tree top) -- against the same squares extended one at a
    time (tree-top path) and, for two of them, the C oracle."""
    import torch
    from celestia_da import testfactory
    k, n, distinct = 32, 1024, 64
    W = 2 * k
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    ods = [torch.from_numpy(testfactory.random_square(k, i)).to(dev).view(k, k, 512) for i in range(distinct)]

    def run(m, fill):
        eds = torch.zeros((m, W, W, 512), dtype=torch.uint8, device=dev)
        for p in range(m):
            eds[p, :k, :k] = fill(p)
        rows = torch.empty(m, W * 90, dtype=torch.uint8, device=dev)
        cols = torch.empty(m, W * 90, dtype=torch.uint8, device=dev)
        roots = torch.empty(m, 32, dtype=torch.uint8, device=dev)
        status = torch.empty(m, dtype=torch.int32, device=dev)
        ctx.extend_dah_inplace_device(k, m, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                      status.data_ptr(), s)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        return roots.cpu().numpy(), rows.cpu().numpy(), cols.cpu().numpy()

    batch = run(n, lambda p: ods[p % distinct])
    for i in range(distinct):
        one = run(1, lambda p: ods[i])
        for p in range(i, n, distinct):
            assert batch[0][p].tobytes() == one[0][0].tobytes(), (i, p)
            assert batch[1][p].tobytes() == one[1][0].tobytes(), (i, p)
            assert batch[2][p].tobytes() == one[2][0].tobytes(), (i, p)
    for i in (0, distinct - 1):
        _, wrows, wcols, wroot = coracle.extend_dah(testfactory.random_square(k, i))
        assert batch[0][i].tobytes() == wroot, i
        assert batch[1][i].tobytes() == wrows.tobytes() and batch[2][i].tobytes() == wcols.tobytes(), i


@pytest.mark.parametrize("k", [3, 5, 6, 7, 12, 100, 200])
def test_codec_encode_non_power_of_two(ctx, k):
    """rsmt2d Codec.Encode of a non-power-of-two shard count (klauspost pads
    the IFFT input to ceilPow2(k) with zeros, m = ceilPow2(k))."""
    rng = np.random.default_rng(k)
    data = rng.integers(0, 256, (k, 128), dtype=np.uint8)
    assert np.array_equal(rsmt2d.LeoRSCodec(ctx).encode(data), pyref.leopard_encode(data))


def test_split_rows_send_layout_on_gpu(ctx):
    """cda_split_rows_send writes the row block straight in the all-to-all
    send layout [parts][R][C][512] (no host-side regrouping copies)."""
    import torch
    dev = torch.device("cuda", 0)
    k, parts, R = 32, 4, 8
    W, C = 2 * k, 2 * k // 4
    ods = coracle.random_square(k, 12).reshape(k, k, 512)
    rows = torch.from_numpy(ods[8:16].copy()).to(dev)
    err1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
    err2 = torch.full((1,), -1, dtype=torch.int32, device=dev)
    blk = torch.empty((R, W, 512), dtype=torch.uint8, device=dev)
    send = torch.empty((parts, R, C, 512), dtype=torch.uint8, device=dev)
    ctx.split_rows(rows.data_ptr(), k, R, 8, blk.data_ptr(), err1.data_ptr())
    ctx.split_rows_send(rows.data_ptr(), k, R, 8, parts, send.data_ptr(), err2.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(send, blk.view(R, parts, C, 512).permute(1, 0, 2, 3))
    eds = coracle.extend(ods.reshape(-1, 512)).reshape(W, W, 512)
    assert np.array_equal(blk.cpu().numpy(), eds[8:16])


@pytest.mark.parametrize("k", [16, 512])
def test_rccl_split_world1_on_gpu(ctx, k):
    """Config 5 through the library's own RCCL communicator, world size 1
    (RCCL self send/recv for the all-to-all and the gathers): EDS columns,
    roots and data root equal the single-GPU path and the oracle."""
    import torch
    from celestia_da import _lib, dist as cdist, testfactory
    dev = torch.device("cuda", 0)
    c = _lib.Context(0)
    c.comm_init(0, 1, _lib.comm_unique_id())
    try:
        ods = testfactory.random_square(k, 0 if k == 512 else 3)
        d_ods = torch.from_numpy(ods).to(dev)
        block, (rows, cols, root, err) = cdist.extend_dah_split_rccl(c, d_ods, k, 0, 1)
        torch.cuda.synchronize()
        assert int(err.item()) == 0xFFFFFFFF
        W = 2 * k
        e = torch.empty(W * W * 512, dtype=torch.uint8, device=dev)
        r1 = torch.empty(W * 90, dtype=torch.uint8, device=dev)
        c1 = torch.empty(W * 90, dtype=torch.uint8, device=dev)
        g1 = torch.empty(32, dtype=torch.uint8, device=dev)
        ctx.extend_dah_device(d_ods.data_ptr(), k, 1, e.data_ptr(), r1.data_ptr(), c1.data_ptr(), g1.data_ptr(),
                              None, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(block.view(-1), e)
        assert torch.equal(rows.view(-1), r1) and torch.equal(cols.view(-1), c1) and torch.equal(root, g1)
        if k == 512:
            import json, os
            g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k512.json")))
            assert root.cpu().numpy().tobytes().hex() == g["squares"]["0"]["data_root"]
        else:
            assert root.cpu().numpy().tobytes() == coracle.extend_dah(ods)[3]
    finally:
        c.comm_destroy()
        c.close()


def test_extend_dah_multi_contexts(ctx):
    """cda_extend_dah_multi (config 4 dispatcher): a host batch split over
    two contexts (on the one GPU of the test box) equals the single-context
    batch and the oracle."""
    from celestia_da import _lib
    k, n = 32, 5
    ods = np.stack([coracle.random_square(k, 60 + i) for i in range(n)])
    ctxs = [_lib.Context(0), _lib.Context(0)]
    try:
        eds, rows, cols, roots, status = _lib.extend_dah_multi(ctxs, ods)
    finally:
        for c in ctxs:
            c.close()
    e2, r2, c2, g2, s2 = da.extend_dah_batch(ods)
    assert (status == 0).all()
    assert np.array_equal(eds, e2) and np.array_equal(rows, r2) and np.array_equal(cols, c2)
    assert np.array_equal(roots, g2)
    for i in range(n):
        assert roots[i].tobytes() == coracle.extend_dah(ods[i])[3]


@pytest.mark.parametrize("k", [8, 128])
def test_torch_split_world1_rows_send_on_gpu(ctx, k):
    """celestia_da.dist.extend_dah_split at one rank with the GPU ops: the row
    encode writes straight into the column block (cda_split_rows_send), no
    collective runs; result equals the oracle."""
    import torch
    from celestia_da import dist as cdist
    dev = torch.device("cuda", 0)
    ods = coracle.random_square(k, 21)
    send, block, (rows, cols, root, err) = cdist.extend_dah_split(torch.from_numpy(ods).to(dev), k,
                                                                   cdist.GpuSplitOps(ctx, dev), 0, 1)
    torch.cuda.synchronize()
    e_eds, e_rows, e_cols, e_root = coracle.extend_dah(ods) if k < 64 else coracle.cpu_baseline(ods, 8)
    assert int(err.item()) == 0xFFFFFFFF
    assert np.array_equal(block.cpu().numpy().reshape(-1, 512), e_eds)
    assert np.array_equal(rows.cpu().numpy(), e_rows) and np.array_equal(cols.cpu().numpy(), e_cols)
    assert root.cpu().numpy().tobytes() == e_root


@pytest.mark.parametrize("k", [128, 512])
def test_extension_is_linear_full_size(ctx, k):
    """Size-independent property at the bench sizes (configs 2-4 and 3): the
    extension is GF(2)-linear, EDS(a ^ b) == EDS(a) ^ EDS(b), and the ODS
    comes back unchanged in Q0 (any bytes: extension never checks namespaces)."""
    rng = np.random.default_rng(k + 11)
    a = rng.integers(0, 256, (k * k, 512), dtype=np.uint8)
    b = rng.integers(0, 256, (k * k, 512), dtype=np.uint8)
    ea = da.extend_shares(a).array().reshape(2 * k, 2 * k, 512)
    eb = da.extend_shares(b).array().reshape(2 * k, 2 * k, 512)
    ex = da.extend_shares(a ^ b).array().reshape(2 * k, 2 * k, 512)
    assert np.array_equal(ea[:k, :k].reshape(-1, 512), a)
    assert np.array_equal(ex, ea ^ eb)
    # idempotence: a second extension of the same ODS gives the same bytes
    assert np.array_equal(da.extend_shares(a).array().reshape(2 * k, 2 * k, 512), ea)


def test_threads_and_streams_on_one_context(ctx):
    """Six host threads, each with its own stream, enqueue device calls of
    different shapes (single squares: lane-pair tree tops; batches: wide
    levels) on ONE context with no host sync in between -- the cgo situation
    of several goroutines sharing a device context.  Every data root and
    every row/column root equals the oracle."""
    import threading
    import torch
    dev = torch.device("cuda", 0)
    shapes = [(16, 1), (32, 3), (64, 1), (128, 1), (64, 2), (8, 5)]
    jobs = []
    for j, (k, n) in enumerate(shapes):
        W = 2 * k
        ods = np.stack([coracle.random_square(k, 500 + 10 * j + i) for i in range(n)])
        jobs.append(dict(k=k, n=n, ods=ods, o=torch.from_numpy(ods.reshape(n, -1)).to(dev),
                         e=torch.empty(n, W * W * 512, dtype=torch.uint8, device=dev),
                         r=torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                         c=torch.empty(n, W * 90, dtype=torch.uint8, device=dev),
                         g=torch.empty(n, 32, dtype=torch.uint8, device=dev),
                         s=torch.cuda.Stream(dev)))
    torch.cuda.synchronize()
    errs = []
    go = threading.Barrier(len(jobs))

    def worker(jb):
        try:
            go.wait()
            for _ in range(3):
                ctx.extend_dah_device(jb["o"].data_ptr(), jb["k"], jb["n"], jb["e"].data_ptr(), jb["r"].data_ptr(),
                                      jb["c"].data_ptr(), jb["g"].data_ptr(), None, jb["s"].cuda_stream)
        except Exception as ex:  # reported below
            errs.append(repr(ex))

    ts = [threading.Thread(target=worker, args=(jb,)) for jb in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert errs == []
    for jb in jobs:
        W = 2 * jb["k"]
        for i in range(jb["n"]):
            e_eds, e_rows, e_cols, e_root = (coracle.cpu_baseline(jb["ods"][i], 8) if jb["k"] >= 64
                                             else coracle.extend_dah(jb["ods"][i]))
            assert np.array_equal(jb["r"][i].cpu().numpy().reshape(W, 90), e_rows), (jb["k"], i)
            assert np.array_equal(jb["c"][i].cpu().numpy().reshape(W, 90), e_cols), (jb["k"], i)
            assert jb["g"][i].cpu().numpy().tobytes() == e_root, (jb["k"], i)


@pytest.mark.parametrize("k,n,bad", [(64, 9, (0, 4, 8)), (128, 5, (3,)), (256, 3, (1, 2))])
def test_push_order_detail_at_every_square(ctx, k, n, bad):
    """cda_push_order_detail_at after an in-place device batch: the squares in
    `bad` carry a Q0 namespace violation (two of them at k = 256, on the
    GF(2^16) path; k = 64 / 128 batches of < 64 squares hash on two streams),
    each reports the brute-force first violation, every other square (-1, 0,
    0) with its oracle data root; a square index past the batch is an error."""
    import torch
    from celestia_da import CdaError
    W = 2 * k
    dev = torch.device("cuda", 0)
    sq = [coracle.random_square(k, 500 + i).reshape(k, k, 512).copy() for i in range(n)]
    want = {}
    for j, i in enumerate(bad):
        r, c = (7 * j + 3) % k, (5 * j + 11) % k
        if c == 0:
            c = 1
        sq[i][r, c, :29] = sq[i][0, 0, :29]
        want[i] = _first_violation(sq[i])
        assert want[i] is not None
    eds = torch.zeros((n, W, W, 512), dtype=torch.uint8, device=dev)
    for i in range(n):
        eds[i, :k, :k] = torch.from_numpy(sq[i]).to(dev)
    rows = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    cols = torch.empty(n, W * 90, dtype=torch.uint8, device=dev)
    roots = torch.empty(n, 32, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.extend_dah_inplace_device(k, n, eds.data_ptr(), rows.data_ptr(), cols.data_ptr(), roots.data_ptr(),
                                  status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    for i in range(n):
        if i in want:
            assert st[i] == -3 and ctx.push_order_detail_at(i) == want[i], i
        else:
            assert st[i] == 0 and ctx.push_order_detail_at(i) == (-1, 0, 0), i
            assert bytes(roots[i].cpu().numpy()) == coracle.extend_dah(sq[i].reshape(-1, 512))[3], i
    with pytest.raises(CdaError, match="last device batch"):
        ctx.push_order_detail_at(n)
