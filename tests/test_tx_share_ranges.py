"""cda_square_tx_share_ranges: builder.FindTxShareRange for many transactions
with the square laid out once (what new_tx_inclusion_proofs looks its ranges
up with).  Host only, no GPU: every answer equals cda_square_tx_share_range's
for the same index, on the blocks of test_tx_proofs.py.
"""
import ctypes as C

import numpy as np
import pytest

from celestia_da import CdaError, SquareError, _lib, blobfactory
from celestia_da import proof as gpr
from celestia_da import square as gsq
from test_tx_proofs import _blocks


@pytest.mark.parametrize("name", list(_blocks()))
def test_equals_the_single_look_up(name):
    txs = _blocks()[name]
    idx = list(range(len(txs)))
    want = [gpr.tx_share_range(txs, i) for i in idx]
    assert gpr.tx_share_ranges(txs, idx) == want
    # any order, repeats
    pick = idx[::-1] + idx[:3]
    assert gpr.tx_share_ranges(txs, pick) == [want[i] for i in pick]
    assert gpr.tx_share_ranges(txs, []) == []


def test_errors_leave_the_outputs_untouched():
    txs = _blocks()["repeated"]
    with pytest.raises(CdaError, match="txIndex 5 out of range") as e:
        gpr.tx_share_ranges(txs, [0, 5, 1])
    assert e.value.code == _lib.CDA_ERR_INVALID
    buf, off = gsq._flatten(txs)
    idx = np.array([0, 7], dtype=np.uint32)
    s, e_, pfb = np.full(2, 0xAAAAAAAA, dtype=np.uint32), np.full(2, 0xAAAAAAAA, dtype=np.uint32), \
        np.full(2, 0xAA, dtype=np.uint8)
    u32p = C.POINTER(C.c_uint32)
    L = _lib.load()
    rc = L.cda_square_tx_share_ranges(None, gsq.ptr(buf), gsq._u64p(off), len(txs), 128, 64, idx.ctypes.data_as(u32p),
                                      2, s.ctypes.data_as(u32p), e_.ctypes.data_as(u32p), gsq.ptr(pfb))
    assert rc == _lib.CDA_ERR_INVALID and L.cda_last_error(None).decode() == "txIndex 7 out of range"
    assert (s == 0xAAAAAAAA).all() and (e_ == 0xAAAAAAAA).all() and (pfb == 0xAA).all()
    # is_pfb may be NULL
    idx[1] = 1
    rc = L.cda_square_tx_share_ranges(None, gsq.ptr(buf), gsq._u64p(off), len(txs), 128, 64, idx.ctypes.data_as(u32p),
                                      2, s.ctypes.data_as(u32p), e_.ctypes.data_as(u32p), None)
    assert rc == _lib.CDA_OK and [(int(a), int(b)) for a, b in zip(s, e_)] == [gpr.tx_share_range(txs, i)[:2]
                                                                                for i in (0, 1)]
    rng = np.random.default_rng(3)
    bad = blobfactory.random_block(12, 1, 2) + [blobfactory.normal_tx(rng, 100)]
    with pytest.raises(SquareError, match="normal transaction at index 3"):
        gpr.tx_share_ranges(bad, [0])
