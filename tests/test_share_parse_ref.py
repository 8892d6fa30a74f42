"""Pins tests/share_parse_ref.py, the pure-Python restatement of the share
parser's rules, to what is known independently of it: mainnet block 408 (its
ODS and its txs are both in tests/golden/) and oracle.square's builder, which
the data roots pin.  No GPU, no product code.
"""
import base64
import gzip
import json
import os

import pytest

import share_parse_ref as ref
import square as osq
from celestia_da import blobfactory

HERE = os.path.dirname(os.path.abspath(__file__))


def block408():
    with gzip.open(os.path.join(HERE, "golden", "block408_txs.json.gz"), "rt") as f:
        d = json.load(f)
    with gzip.open(os.path.join(HERE, "golden", "block408_ods.bin.gz")) as f:
        ods = f.read()
    return [base64.b64decode(t) for t in d["txs"]], ods


def test_block408():
    txs, ods = block408()
    p = ref.parse(ods)
    tail = sum(ods[i * 512:i * 512 + 29] == ref.TAIL_PADDING_NS for i in range(32 * 32))
    reserved = sum(ods[i * 512:i * 512 + 29] == ref.RESERVED_PADDING_NS for i in range(32 * 32))
    assert (tail, reserved, p.n_padding) == (304, 3, 307)
    assert [u for u, _, _ in p.txs] == txs[:273] and len(p.txs) == 273
    inner, blobs = osq.unmarshal_blob_tx(txs[273])
    assert [u for u, _, _ in p.pfbs] == [osq.marshal_index_wrapper(inner, [368])]
    assert len(p.blobs) == 1
    namespace, version, data, start, shares = p.blobs[0]
    assert (len(data), start, version) == (169275, 368, 0)
    assert data == blobs[0]["data"] and namespace == bytes([blobs[0]["namespace_version"]]) + blobs[0]["namespace_id"]
    assert shares == osq.sparse_share_count(169275)


@pytest.mark.parametrize("seed", range(1, 9))
def test_builder_round_trip(seed):
    txs = blobfactory.random_block(seed, n_normal=5 + seed, n_blob_txs=6 * seed, blob_size=(1, 3000))
    shares, k, kept, share_idx = osq.builder(txs, 32)
    assert kept == list(range(len(txs)))
    p = ref.parse(b"".join(shares))
    normal = [t for t in txs if osq.unmarshal_blob_tx(t) is None]
    assert [u for u, _, _ in p.txs] == normal
    want_pfbs, want_blobs, at = [], {}, 0
    for t in txs:
        bt = osq.unmarshal_blob_tx(t)
        if bt is None:
            continue
        inner, bl = bt
        idx = share_idx[at:at + len(bl)]
        at += len(bl)
        want_pfbs.append(osq.marshal_index_wrapper(inner, idx))
        for i, b in zip(idx, bl):
            want_blobs[i] = (bytes([b["namespace_version"]]) + b["namespace_id"], 0, b["data"], i,
                             osq.sparse_share_count(len(b["data"])))
    assert [u for u, _, _ in p.pfbs] == want_pfbs
    assert p.blobs == [want_blobs[i] for i in sorted(want_blobs)]
    assert 11 <= len(p.blobs) <= 102
    if seed >= 2:
        assert {len(b[2]) % 8 for b in p.blobs} == set(range(8))
    # the units' share ranges are the builder's own (compact_share_ranges keys equal units by their bytes)
    n_tx = len(osq.compact_shares(osq.TX_NS, normal))
    if len(set(normal)) == len(normal):
        assert [(s, e) for _, s, e in p.txs] == osq.compact_share_ranges(normal)
    if len(set(want_pfbs)) == len(want_pfbs):
        assert [(s - n_tx, e - n_tx) for _, s, e in p.pfbs] == osq.compact_share_ranges(want_pfbs)
