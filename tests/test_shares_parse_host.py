"""cda_shares_parse_plan / cda_shares_parse, the host-only C restatement of the
share parser, through ctypes against tests/share_parse_ref.py: block 408, the
builder's squares for seeds 1..8, the hand-made edge squares, every error class
with its text and untouched outputs, NULL outputs, and the empty input.  No GPU.
"""
import ctypes as C

import numpy as np
import pytest

import guarded
import share_parse_ref as ref
import share_parse_squares as sqs
import square as osq
from celestia_da import SquareError, _lib, blobfactory, shares
from test_share_parse_ref import block408

OUT_FIELDS = [n for n, _ in _lib.ParseOut._fields_]


def ref_arrays(p: ref.Parsed) -> dict:
    """The reference's answer in cda_parse_out's layout."""
    units = p.txs + p.pfbs
    u8 = lambda b: np.frombuffer(bytes(b), dtype=np.uint8)   # noqa: E731
    return dict(
        blob_start=np.array([b[3] for b in p.blobs], dtype=np.uint32),
        blob_shares=np.array([b[4] for b in p.blobs], dtype=np.uint32),
        blob_namespace=u8(b"".join(b[0] for b in p.blobs)),
        blob_share_version=np.array([b[1] for b in p.blobs], dtype=np.uint8),
        blob_off=np.cumsum([0] + [len(b[2]) for b in p.blobs]).astype(np.uint64),
        blob_data=u8(b"".join(b[2] for b in p.blobs)),
        unit_off=np.cumsum([0] + [len(u[0]) for u in units]).astype(np.uint64),
        unit_data=u8(b"".join(u[0] for u in units)),
        unit_start=np.array([u[1] for u in units], dtype=np.uint32),
        unit_end=np.array([u[2] for u in units], dtype=np.uint32))


def guarded_out(want: dict, skip=()):
    """A cda_parse_out over guarded host buffers of exactly the expected sizes."""
    bufs, o = {}, _lib.ParseOut()
    for name, t in _lib.ParseOut._fields_:
        if name in skip:
            continue
        a = want[name]
        align = min(8, a.dtype.itemsize) if name != "blob_data" else 1
        bufs[name] = guarded.alloc(a.nbytes, align=align, name=name)
        setattr(o, name, C.cast(bufs[name].ptr, t))
    return bufs, o


def check_case(raw: bytes):
    L = _lib.load()
    want = ref.parse(raw)
    a = np.frombuffer(raw, dtype=np.uint8)
    p = _lib.ParsePlanT()
    assert L.cda_shares_parse_plan(_lib.ptr(a), len(raw) // 512, C.byref(p)) == 0, L.cda_last_error(None)
    assert shares.plan_dict(p) == want.plan
    arrays = ref_arrays(want)
    bufs, o = guarded_out(arrays)
    assert L.cda_shares_parse(_lib.ptr(a), len(raw) // 512, C.byref(o)) == 0, L.cda_last_error(None)
    for name, g in bufs.items():
        g.assert_written(arrays[name])
        g.assert_guards()
    return want


def test_block408():
    _, ods = block408()
    want = check_case(ods)
    assert want.plan == dict(n_blobs=1, n_txs=273, n_pfbs=1, n_padding_shares=307, blob_bytes=169275,
                             unit_bytes=sum(len(u[0]) for u in want.txs + want.pfbs))


@pytest.mark.parametrize("seed", range(1, 9))
def test_builder_squares(seed):
    txs = blobfactory.random_block(seed, n_normal=5 + seed, n_blob_txs=6 * seed, blob_size=(1, 3000))
    check_case(b"".join(osq.builder(txs, 32)[0]))


@pytest.mark.parametrize("name", sorted(sqs.edge_squares()))
def test_edge_squares(name):
    check_case(b"".join(sqs.edge_squares()[name]))


def test_k1_is_one_padding_share():
    assert shares.parse_plan(b"".join(sqs.k1())) == dict(n_blobs=0, n_txs=0, n_pfbs=0, n_padding_shares=1,
                                                        blob_bytes=0, unit_bytes=0)


@pytest.mark.parametrize("name", sorted(sqs.invalid_squares()))
def test_errors_name_the_share_and_leave_outputs_untouched(name):
    square, text = sqs.invalid_squares()[name]
    raw = b"".join(square)
    with pytest.raises(ref.ParseError) as e:
        ref.parse(raw)
    assert str(e.value) == text
    L = _lib.load()
    a = np.frombuffer(raw, dtype=np.uint8)
    p = _lib.ParsePlanT(7, 7, 7, 7, 7, 7)
    assert L.cda_shares_parse_plan(_lib.ptr(a), 16, C.byref(p)) == _lib.CDA_ERR_SQUARE
    assert L.cda_last_error(None).decode() == text
    assert shares.plan_dict(p) == dict.fromkeys(shares.plan_dict(p), 7)
    arrays = ref_arrays(ref.parse(b"".join(sqs.k4_boundary())))     # buffers of a valid square's sizes
    bufs, o = guarded_out(arrays)
    assert L.cda_shares_parse(_lib.ptr(a), 16, C.byref(o)) == _lib.CDA_ERR_SQUARE
    assert L.cda_last_error(None).decode() == text
    for g in bufs.values():
        g.assert_untouched()
    with pytest.raises(SquareError, match=text.split(":")[0]):
        shares.parse_shares(raw)


def test_null_outputs_are_accepted():
    raw = b"".join(sqs.k4_boundary())
    a = np.frombuffer(raw, dtype=np.uint8)
    L = _lib.load()
    arrays = ref_arrays(ref.parse(raw))
    assert L.cda_shares_parse(_lib.ptr(a), 16, C.byref(_lib.ParseOut())) == 0
    for keep in OUT_FIELDS:
        bufs, o = guarded_out(arrays, skip=[n for n in OUT_FIELDS if n != keep])
        assert L.cda_shares_parse(_lib.ptr(a), 16, C.byref(o)) == 0
        bufs[keep].assert_written(arrays[keep])
        bufs[keep].assert_guards()
    assert L.cda_shares_parse(_lib.ptr(a), 16, None) == _lib.CDA_ERR_INVALID
    assert L.cda_shares_parse_plan(_lib.ptr(a), 16, None) == _lib.CDA_ERR_INVALID


def test_no_shares():
    L = _lib.load()
    p = _lib.ParsePlanT(7, 7, 7, 7, 7, 7)
    assert L.cda_shares_parse_plan(None, 0, C.byref(p)) == 0
    assert shares.plan_dict(p) == dict.fromkeys(shares.plan_dict(p), 0)
    off = np.full(2, 9, dtype=np.uint64)
    o = _lib.ParseOut()
    o.blob_off = off[:1].ctypes.data_as(C.POINTER(C.c_uint64))
    o.unit_off = off[1:].ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.cda_shares_parse(None, 0, C.byref(o)) == 0
    assert list(off) == [0, 0]
    assert shares.parse_shares(b"").blobs == []


def test_python_mirror():
    txs, ods = block408()
    p = shares.parse_shares(ods)
    assert p.txs == txs[:273] and len(p.pfbs) == 1 and p.blob_starts == [368] and p.n_padding_shares == 307
    inner, idx = shares.unmarshal_index_wrapper(p.pfbs[0])
    assert idx == [368] and osq.marshal_index_wrapper(inner, idx) == p.pfbs[0]
    assert osq.unmarshal_blob_tx(txs[273])[0] == inner
    sq = sqs.k4_boundary()
    assert [len(b.data) for b in shares.parse_blobs(b"".join(sq[3:12]))] == list(sqs.BOUNDARY_LENGTHS)
    assert [len(u) for u in shares.parse_txs(b"".join(sq[0:2]))] == [100, 30, 60]
    with pytest.raises(SquareError, match="compact sequence at share 0"):
        shares.parse_blobs(b"".join(sq))
    with pytest.raises(SquareError, match="sparse sequence at share 3"):
        shares.parse_txs(b"".join(sq))
    with pytest.raises(SquareError, match="4 padding shares"):
        shares.parse_shares(b"".join(sq[12:]), ignore_padding=False)
    with pytest.raises(ValueError):
        shares.unmarshal_index_wrapper(txs[0])
