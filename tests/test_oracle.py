"""CPU tests of the oracle (the checker): pinned against the reference's own
golden vectors and fixtures before anything is compared with the GPU."""
import base64
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import coracle
import pyref
import square

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))


def block408_ods():
    with gzip.open(os.path.join(HERE, "golden", "block408_ods.bin.gz")) as f:
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(-1, 512).copy()


def test_nil_hash():
    assert pyref.merkle_root([]).hex() == GOLDEN["reference_golden"]["nil_dah"]


def test_min_dah_k1():
    ods = np.frombuffer(pyref.tail_padding_share(), dtype=np.uint8).reshape(1, 512)
    for impl in (lambda o: coracle.extend_dah(o)[3], lambda o: pyref.extend_and_dah(o.reshape(1, 1, 512))[3]):
        assert impl(ods).hex() == GOLDEN["reference_golden"]["min_dah_k1"]


@pytest.mark.parametrize("k,key", [(2, "constant_k2"), (128, "constant_k128")])
def test_constant_goldens(k, key):
    ods = pyref.constant_shares(k * k)
    root = coracle.cpu_baseline(ods, 8)[3] if k > 8 else coracle.extend_dah(ods)[3]
    assert root.hex() == GOLDEN["reference_golden"][key]
    if k <= 8:
        assert pyref.extend_and_dah(pyref.ods_from_shares(ods))[3].hex() == GOLDEN["reference_golden"][key]


def test_block408_data_root():
    """Real-data pin of Leopard GF(2^8) + NMT + DAH (k=32)."""
    ods = block408_ods()
    g = GOLDEN["block408"]
    assert hashlib.sha256(ods.tobytes()).hexdigest() == g["ods_sha256"]
    eds, rows, cols, root = coracle.extend_dah(ods)
    assert root.hex() == g["data_hash"]
    assert hashlib.sha256(eds.tobytes()).hexdigest() == g["eds_sha256"]


def block408():
    """The block's txs, square size and header.data_hash: the data of the
    reference fixture x/blob/test/testdata/block_response.json, stored by
    oracle/gen_golden.py."""
    with gzip.open(os.path.join(HERE, "golden", "block408_txs.json.gz"), "rt") as f:
        d = json.load(f)
    return [base64.b64decode(t) for t in d["txs"]], d["square_size"], bytes.fromhex(d["data_hash"])


def test_square_construction_reproduces_fixture():
    txs, k, data_hash = block408()
    ods = np.frombuffer(b"".join(square.construct(txs, k)), dtype=np.uint8).reshape(-1, 512)
    assert np.array_equal(ods, block408_ods())
    assert data_hash.hex() == GOLDEN["block408"]["data_hash"]


@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 32])
def test_random_square_fixtures(k):
    g = GOLDEN["random_squares"][str(k)]
    ods = coracle.random_square(k, g["seed_index"])
    assert hashlib.sha256(ods.tobytes()).hexdigest() == g["ods_sha256"]
    eds, rows, cols, root = coracle.extend_dah(ods)
    assert hashlib.sha256(eds.tobytes()).hexdigest() == g["eds_sha256"]
    assert root.hex() == g["data_root"]


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_c_oracle_matches_python(k):
    a = coracle.random_square(k, 11)
    b = pyref.random_namespaced_square(k, 11)
    assert np.array_equal(a, b)
    e1, r1, c1, root1 = coracle.extend_dah(a)
    e2, r2, c2, root2 = pyref.extend_and_dah(pyref.ods_from_shares(b))
    assert np.array_equal(e1, e2.reshape(-1, 512)) and root1 == root2


def _gf_mul(F, a, b):
    if a == 0 or b == 0:
        return 0
    return F.exp[F.add_mod(F.log[a], F.log[b])]


def _lagrange(F, data):
    """parity[j] = P(j), P of degree < k through (k+i, data[i])."""
    k = len(data)
    xs = [k + i for i in range(k)]
    inv = lambda a: F.exp[(F.mod - F.log[a]) % F.mod]
    out = []
    for x in range(k):
        acc = 0
        for i in range(k):
            num = den = 1
            for j in range(k):
                if j != i:
                    num = _gf_mul(F, num, x ^ xs[j])
                    den = _gf_mul(F, den, xs[i] ^ xs[j])
            acc ^= _gf_mul(F, data[i], _gf_mul(F, num, inv(den)))
        out.append(acc)
    return out


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_fft_equals_lagrange(bits, k):
    """Independent cross-check of the additive-FFT skew/layer order."""
    F = pyref.gf8() if bits == 8 else pyref.gf16()
    rng = np.random.default_rng(bits * 100 + k)
    d = [int(v) for v in rng.integers(0, F.order, k)]
    w = pyref._encode_symbols(F, np.array(d, dtype=np.int64).reshape(k, 1))[:, 0].tolist()
    assert w == _lagrange(F, d)


@pytest.mark.parametrize("k", [128, 256])
def test_mds_any_k_of_2k(k):
    """Any k of the 2k codeword symbols determine the data (MDS): re-encoding
    the parity as data of the inverse map is not available, so check the
    weaker, size-independent property that a single non-zero data symbol
    yields all-non-zero parity (minimum distance k+1)."""
    F = pyref.field_for(k)
    for pos in (0, k // 2, k - 1):
        d = np.zeros((k, 1), dtype=np.int64)
        d[pos, 0] = 1
        par = pyref._encode_symbols(F, d)[:, 0]
        assert (par != 0).all()


def test_c_and_python_tables_agree():
    for bits, F in ((8, pyref.gf8()), (16, pyref.gf16())):
        assert np.array_equal(coracle.table(bits, "log"), np.array(F.log))
        assert np.array_equal(coracle.table(bits, "exp"), np.array(F.exp))
        assert np.array_equal(coracle.table(bits, "skew"), np.array(F.skew))


def test_gf16_codec_c_matches_python():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, (256, 128), dtype=np.uint8)
    assert np.array_equal(coracle.leopard_encode(data), pyref.leopard_encode(data))


@pytest.mark.parametrize("k", [16, 64, 256])
def test_cpu_baseline_equals_scalar_oracle(k):
    """The baseline path (SHA-NI + AVX2 nibble-table RS, threads) is bit-equal
    to the scalar checker, GF(2^8) and GF(2^16)."""
    ods = coracle.random_square(k, 3)
    a = coracle.extend_dah(ods)
    b = coracle.cpu_baseline(ods, 4)
    assert np.array_equal(a[0], b[0]) and a[3] == b[3]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_sha_ni_block_matches_portable():
    import ctypes as C
    L = coracle.lib()
    L.oracle_sha256_block_test.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_int]
    rng = np.random.default_rng(1)
    for _ in range(64):
        blk = rng.integers(0, 256, 64, dtype=np.uint8)
        st = rng.integers(0, 2**32, 8, dtype=np.uint64).astype(np.uint32)
        a, b = st.copy(), st.copy()
        L.oracle_sha256_block_test(a.ctypes.data_as(C.POINTER(C.c_uint32)), blk.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
        L.oracle_sha256_block_test(b.ctypes.data_as(C.POINTER(C.c_uint32)), blk.ctypes.data_as(C.POINTER(C.c_uint8)), 1)
        assert np.array_equal(a, b)


def test_push_order_detected_by_oracle():
    k = 4
    ods = coracle.random_square(k, 2).reshape(k, k, 512).copy()
    ods[1, 2, :29], ods[1, 3, :29] = ods[1, 3, :29].copy(), ods[1, 2, :29].copy()
    with pytest.raises(coracle.PushOrderError):
        coracle.extend_dah(ods.reshape(-1, 512))
    with pytest.raises(pyref.PushOrderError):
        pyref.extend_and_dah(ods)


def _lagrange_at(F, d, xs_eval):
    """Vectorised SURVEY A.4 check: P(x) for x in xs_eval, P of degree < k
    through (k+i, d[i]) over the Cantor-basis field; d is (k, n_symbols)."""
    k = d.shape[0]
    mod, log, exp = F.mod, F.log_np, F.exp_np
    xs = np.arange(k, 2 * k)
    diff = xs[:, None] ^ xs[None, :]
    np.fill_diagonal(diff, 1)                        # log 1 = 0 drops j == i
    den = log[diff].sum(axis=1) % mod               # log prod_{j != i} (xs_i ^ xs_j)
    nz = d != 0
    ld = np.where(nz, log[d], 0)
    out = []
    for x in xs_eval:
        lx = log[x ^ xs]                            # x is not a data point: all non-zero
        lnum = (lx.sum() - lx) % mod                # log prod_{j != i} (x ^ xs_j)
        coef = (lnum - den) % mod                   # log L_i(x)
        terms = np.where(nz, exp[(ld + coef[:, None]) % mod], 0)
        out.append(np.bitwise_xor.reduce(terms, axis=0))
    return np.array(out)


@pytest.mark.parametrize("k", [256, 512, 1024])
def test_gf16_encoder_equals_lagrange_full_size(k):
    """The GF(2^16) restatement at the sizes the path uses (config 3, k=512,
    and the widest accepted square, k=1024),
    in the real lo/hi shard layout, equals Lagrange interpolation at sampled
    parity positions: no reference vector exists for GF(2^16),
    so this is its full-size intrinsic pin; the GPU is pinned to the same
    restatement by test_gpu_parity.py."""
    F = pyref.gf16()
    rng = np.random.default_rng(k)
    data = rng.integers(0, 256, (k, 64), dtype=np.uint8)
    par = coracle.leopard_encode(data)
    sym = lambda b: b[:, :32].astype(np.int64) | (b[:, 32:].astype(np.int64) << 8)   # symbol i = b[i] | b[i+32] << 8
    xs_eval = [0, 1, 2, k // 2 - 1, k // 2, k - 1]
    want = _lagrange_at(F, sym(data), xs_eval)
    got = sym(par)[xs_eval]
    assert np.array_equal(got, want)


def _clmul_mod(a, b, bits, poly):
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> bits:
            a ^= poly
    return r


@pytest.mark.parametrize("bits,poly,basis", [(8, 0x11D, pyref.CANTOR8), (16, 0x1002D, pyref.CANTOR16)])
def test_cantor_basis_and_polynomial_are_self_consistent(bits, poly, basis):
    """Intrinsic pin of the recalled Leopard field constants (klauspost
    reedsolomon v1.12.1 leopard.go / leopard8.go): the
    generator polynomial is primitive (x has order 2^bits - 1), and the basis
    is a Cantor basis of that field, beta_0 = 1 and beta_i^2 + beta_i =
    beta_(i-1).  A mis-recalled constant or polynomial fails this with
    probability ~1 - 2^-bits per entry.  GF(2^8) is additionally pinned by
    mainnet block 408 (test_block408_data_root); GF(2^16) has no reference
    vector, so this and the Lagrange check are its pins."""
    order = (1 << bits) - 1
    x, n = 2, 1
    while x != 1:
        x = _clmul_mod(x, 2, bits, poly)
        n += 1
    assert n == order
    assert basis[0] == 1 and len(basis) == bits
    for i in range(1, bits):
        b = basis[i]
        assert _clmul_mod(b, b, bits, poly) ^ b == basis[i - 1]
    # the basis spans the field: the log table built on it is a permutation
    F = pyref.gf8() if bits == 8 else pyref.gf16()
    assert sorted(F.log[:order + 1]) == list(range(order + 1))
