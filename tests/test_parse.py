"""cda_square_parse_plan / cda_square_parse on the GPU: a resident square's Q0
back into transactions, IndexWrappers and blobs.

Expected values come from tests/share_parse_ref.py (the pure-Python
restatement, itself pinned to block 408 and the builder by
test_share_parse_ref.py) and from oracle.square's share writers.  Every output
of every call lies in a guarded buffer (tests/guarded.py): the payload must equal
the reference byte for byte and the guards must be intact.  Squares have k <= 32.
"""
import ctypes as C

import numpy as np
import pytest

import share_parse_ref as ref
import share_parse_squares as sqs
import square as osq
from celestia_da import CdaError, SquareError, _lib, blob, blobfactory, inclusion, proof, shares
from test_share_parse_ref import block408
from test_shares_parse_host import OUT_FIELDS, guarded_out, ref_arrays

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)


def resident(square_shares, ctx):
    raw = b"".join(square_shares) if not isinstance(square_shares, bytes) else square_shares
    return proof.ResidentSquare(np.frombuffer(raw, dtype=np.uint8), ctx), raw


def range_args(ranges):
    if ranges is None:
        return None, None, 0, None
    r = np.array(ranges, dtype=np.uint32).reshape(-1, 2)
    st, en = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    return st.ctypes.data_as(U32P), en.ctypes.data_as(U32P), len(r), (st, en)


def check_square(sq, raw, ranges=None):
    """Plan and every output of cda_square_parse against the reference, in guarded buffers."""
    want = ref.parse(raw, ranges)
    assert sq.parse_plan(ranges) == want.plan
    arrays = ref_arrays(want)
    bufs, o = guarded_out(arrays)
    st, en, n, keep = range_args(ranges)
    sq.ctx.check(sq.ctx.lib.cda_square_parse(sq.h, st, en, n, C.byref(o)))
    for name, g in bufs.items():
        g.assert_written(arrays[name], name=name)
        g.assert_guards()
    return want


def test_k1_is_one_tail_padding_share(ctx):
    sq, raw = resident(sqs.k1(), ctx)
    assert raw[:29] == osq.TAIL_PADDING_NS and sq.k == 1
    want = check_square(sq, raw)
    assert want.plan == dict(n_blobs=0, n_txs=0, n_pfbs=0, n_padding_shares=1, blob_bytes=0, unit_bytes=0)
    p = sq.parse()
    assert (p.txs, p.pfbs, p.blobs, p.n_padding_shares) == ([], [], [], 1)


def test_k4_boundary_lengths(ctx):
    sq, raw = resident(sqs.k4_boundary(), ctx)
    want = check_square(sq, raw)
    assert [len(b[2]) for b in want.blobs] == list(sqs.BOUNDARY_LENGTHS)
    assert [b[4] for b in want.blobs] == [1, 1, 2, 2, 3] and want.n_padding == 5
    p = sq.parse()
    assert [len(b.data) for b in p.blobs] == list(sqs.BOUNDARY_LENGTHS)
    assert [b.namespace for b in p.blobs] == [sqs.ns(i + 1) for i in range(5)]
    assert (len(p.txs), len(p.pfbs), p.tx_ranges, p.pfb_ranges) == (2, 1, [(0, 1), (0, 1)], [(1, 2)])


def test_k4_blob_crossing_rows(ctx):
    sq, raw = resident(sqs.k4_row_crossing(), ctx)
    want = check_square(sq, raw)
    assert [(b[3], b[4]) for b in want.blobs] == [(3, 6)]
    assert want.blobs[0][2] == sqs.data(478 + 482 * 4 + 100, 5)


@pytest.mark.parametrize("full", [True, False], ids=["filled_to_the_last_byte", "one_byte_in_it"])
def test_k4_blob_ending_in_the_last_share(ctx, full):
    sq, raw = resident(sqs.k4_last_share(full), ctx)
    want = check_square(sq, raw)
    assert [(b[3], b[4]) for b in want.blobs] == [(13, 3)]
    assert len(want.blobs[0][2]) == (478 + 482 * 2 if full else 478 + 482 + 1)


def test_k8_every_output_alignment(ctx):
    sq, raw = resident(sqs.k8_alignment(), ctx)
    want = check_square(sq, raw)
    off = np.cumsum([0] + [len(b[2]) for b in want.blobs])
    assert {int(off[i]) % 8 for i, b in enumerate(want.blobs) if b[4] == 3} == set(range(8))


def test_compact_edges(ctx):
    sq, raw = resident(sqs.k4_compact_edges(), ctx)
    want = check_square(sq, raw)
    assert raw[511] >= 0x80                                   # the prefix of unit 1 straddles shares 0 and 1
    assert [len(u[0]) for u in want.txs] == list(sqs.COMPACT_TX_UNITS)
    assert [(s, e) for _, s, e in want.txs] == [(0, 1), (0, 2), (1, 2), (2, 5), (4, 5)]
    assert [(len(u), s, e) for u, s, e in want.pfbs] == [(300, 5, 6), (400, 5, 7)]     # PFBs right behind the txs
    p = sq.parse()
    assert p.txs == [u for u, _, _ in want.txs] and p.pfbs == [u for u, _, _ in want.pfbs]


def block_cases():
    return ["block408"] + list(range(1, 9))


def block_txs(case):
    if case == "block408":
        txs, ods = block408()
        return txs, ods, 128
    txs = blobfactory.random_block(case, n_normal=5 + case, n_blob_txs=6 * case, blob_size=(1, 3000))
    return txs, b"".join(osq.builder(txs, 32)[0]), 32


@pytest.mark.parametrize("case", block_cases(), ids=str)
def test_blocks(ctx, case):
    txs, ods, max_square = block_txs(case)
    sq, raw = resident(ods, ctx)
    assert sq.k * sq.k * 512 == len(ods) and sq.k <= 32 and not sq.push_order_error
    check_square(sq, raw)
    p = sq.parse()
    # the units' share ranges are the builder's (equal txs all report the last copy's range there)
    normal = [t for t in txs if osq.unmarshal_blob_tx(t) is None]
    assert p.txs == normal and len(p.pfbs) == len(txs) - len(normal)
    ranges = proof.tx_share_ranges(txs, list(range(len(txs))), max_square)
    units = p.txs + p.pfbs
    got = p.tx_ranges + p.pfb_ranges
    for i, (s, e, _) in enumerate(ranges):
        if units.count(units[i]) == 1:
            assert got[i] == (s, e), i
    # every PFB's share indexes are starts of parsed blobs, and together they are all of them
    idx = [i for u in p.pfbs for i in shares.unmarshal_index_wrapper(u)[1]]
    assert sorted(idx) == p.blob_starts
    # commitments: from the parsed bytes, and from the cached row trees at the parsed positions
    commits = inclusion.create_commitments(p.blobs, ctx=ctx)
    assert commits == sq.blob_commitments(p.blob_starts, p.blob_share_lens)
    if case == "block408":
        inner, _ = shares.unmarshal_index_wrapper(p.pfbs[0])
        assert proof.pfb_share_commitments(inner) == commits and len(commits) == 1
    # the proof builder fed from the square gives what the one fed from the txs gives
    from_square = proof.new_blob_commitment_proofs_from_square(sq)
    assert [c for _, c in from_square] == [c for tx in txs for _, c in (proof.blob_tx_blobs(tx) or [])]
    assert [pr.share_len for pr, _ in from_square] == [dict(zip(p.blob_starts, p.blob_share_lens))[i] for i in idx]
    if case == "block408":
        assert [c for _, c in from_square] == commits


def namespace_square():
    """k = 8: blob namespaces 1..6; namespace 3 holds two blobs and spans rows 0 and 1."""
    sq = osq.compact_shares(osq.TX_NS, [sqs.data(40, 1)]) + [osq.padding_share(osq.PRIMARY_RESERVED_PADDING_NS)]
    sq += osq.sparse_shares(sqs.ns(1), sqs.data(700, 2))                 # shares 2-3
    sq += osq.sparse_shares(sqs.ns(2), sqs.data(33, 3))                  # 4
    sq += osq.sparse_shares(sqs.ns(3), sqs.data(1500, 4))                # 5-8: crosses into row 1
    sq += osq.sparse_shares(sqs.ns(3), sqs.data(9, 5))                   # 9
    sq += osq.sparse_shares(sqs.ns(6), sqs.data(2000, 6))                # 10-14
    assert len(sq) == 15 and sq[7][:29] == sq[8][:29] == sqs.ns(3)
    return sqs.fill(sq, 8)


def test_get_all_and_get(ctx):
    sq, raw = resident(namespace_square(), ctx)
    absent = sqs.ns(4)
    assert all(raw[i * 512:i * 512 + 29] != absent for i in range(64))
    assert blob.namespace_ranges(sq, [sqs.ns(3), absent, sqs.ns(1)]) == [(2, 4), (5, 10)]
    got = blob.get_all(sq, [sqs.ns(3), absent, sqs.ns(1)])
    assert [(b.namespace, b.data) for b in got] == [(sqs.ns(1), sqs.data(700, 2)), (sqs.ns(3), sqs.data(1500, 4)),
                                                    (sqs.ns(3), sqs.data(9, 5))]
    assert blob.get_all(sq, [absent]) == []
    check_square(sq, raw, [(2, 4), (5, 10)])
    commitment = inclusion.create_commitment(inclusion.Blob(sqs.ns(3), sqs.data(9, 5)), ctx=ctx)
    hit = blob.get(sq, sqs.ns(3), commitment)
    assert (hit.namespace, hit.data) == (sqs.ns(3), sqs.data(9, 5))
    with pytest.raises(blob.BlobNotFoundError):
        blob.get(sq, sqs.ns(1), commitment)
    with pytest.raises(blob.BlobNotFoundError):
        blob.get(sq, absent, commitment)


def expect_error(sq, ranges, code, text, sizes_of):
    """cda_square_parse_plan and cda_square_parse fail with the text; outputs keep their pattern."""
    st, en, n, keep = range_args(ranges)
    p = _lib.ParsePlanT(7, 7, 7, 7, 7, 7)
    lib = sq.ctx.lib
    assert lib.cda_square_parse_plan(sq.h, st, en, n, C.byref(p)) == code
    assert lib.cda_last_error(sq.ctx.h).decode() == text
    assert shares.plan_dict(p) == dict.fromkeys(shares.plan_dict(p), 7)
    bufs, o = guarded_out(sizes_of)
    assert lib.cda_square_parse(sq.h, st, en, n, C.byref(o)) == code
    assert lib.cda_last_error(sq.ctx.h).decode() == text
    for g in bufs.values():
        g.assert_untouched()


def test_ranges_that_cut_a_sequence(ctx):
    sq, raw = resident(namespace_square(), ctx)
    sizes = ref_arrays(ref.parse(raw))
    for ranges, text in (([(5, 8)], "sequence at share 5: length 1500 needs 4 shares, found 3"),
                         ([(2, 4), (6, 9)], "share 6: the first share of range 1 is a continuation share")):
        with pytest.raises(ref.ParseError) as e:
            ref.parse(raw, ranges)
        assert str(e.value) == text
        expect_error(sq, ranges, _lib.CDA_ERR_SQUARE, text, sizes)
    expect_error(sq, [(4, 9), (8, 10)], _lib.CDA_ERR_INVALID, "range 1: start 8 is below the end 9 of the range before it",
                 sizes)
    expect_error(sq, [(60, 65)], _lib.CDA_ERR_INVALID, "range 0: end 65 is beyond the 64 shares of the original square",
                 sizes)
    with pytest.raises(SquareError, match="sequence at share 5"):
        sq.parse([(5, 8)])


@pytest.mark.parametrize("name", sorted(sqs.invalid_squares()))
def test_invalid_squares(ctx, name):
    square, text = sqs.invalid_squares()[name]
    sq, raw = resident(square, ctx)      # cda_square_create does not look at share format
    expect_error(sq, None, _lib.CDA_ERR_SQUARE, text, ref_arrays(ref.parse(b"".join(sqs.k4_boundary()))))


def test_unordered_square_parses_like_any_other(ctx):
    square = sqs.k4_boundary()
    square[1], square[2] = square[2], square[1]          # row 0: the reserved padding share before the PFB share
    assert square[1][:29] > square[2][:29]
    sq, raw = resident(square, ctx)
    assert sq.push_order_error
    want = check_square(sq, raw)
    assert [len(b[2]) for b in want.blobs] == list(sqs.BOUNDARY_LENGTHS) and [(s, e) for _, s, e in want.pfbs] == [(2, 3)]


def test_null_outputs_and_handles(ctx):
    sq, raw = resident(sqs.k4_boundary(), ctx)
    arrays = ref_arrays(ref.parse(raw))
    lib = sq.ctx.lib
    sq.ctx.check(lib.cda_square_parse(sq.h, None, None, 0, C.byref(_lib.ParseOut())))
    for keep in ("blob_data", "unit_data", "blob_namespace"):
        bufs, o = guarded_out(arrays, skip=[n for n in OUT_FIELDS if n != keep])
        sq.ctx.check(lib.cda_square_parse(sq.h, None, None, 0, C.byref(o)))
        bufs[keep].assert_written(arrays[keep])
        bufs[keep].assert_guards()
    assert lib.cda_square_parse(sq.h, None, None, 0, None) == _lib.CDA_ERR_INVALID
    assert lib.cda_square_parse(None, None, None, 0, C.byref(_lib.ParseOut())) == _lib.CDA_ERR_INVALID
    with pytest.raises(CdaError, match="no share range given"):
        sq.parse([])
