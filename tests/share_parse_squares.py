"""Hand-made squares for the share parser's tests (test_shares_parse_host.py on
the CPU, test_parse.py on the GPU): every layout is built from oracle.square's
share writers, and every builder asserts that its square has the property it
is named for.  Squares are lists of k*k shares; namespaces ascend, so a square
can be made resident without a push-order error unless a case says otherwise.
"""
from __future__ import annotations

import square as osq

SHARE = 512
TX_NS, PFB_NS = osq.TX_NS, osq.PFB_NS
RESERVED, TAIL = osq.PRIMARY_RESERVED_PADDING_NS, osq.TAIL_PADDING_NS
PARITY_NS = b"\xff" * 29


def ns(i: int) -> bytes:
    """Blob namespace number i: version 0, above every reserved namespace."""
    return bytes(19) + b"\x01" + i.to_bytes(9, "big")


def data(n: int, salt: int) -> bytes:
    """n bytes that differ by position and salt, never a run of zeros."""
    return bytes((37 * j + 11 * salt + (j >> 8) + 1) % 251 + 1 for j in range(n))


def fill(shares: list, k: int) -> list:
    assert len(shares) <= k * k, (len(shares), k)
    return shares + [osq.padding_share(TAIL)] * (k * k - len(shares))


def k1():
    return [osq.padding_share(TAIL)]


BOUNDARY_LENGTHS = (1, 478, 479, 960, 961)


def k4_boundary():
    """tx share, PFB share, reserved padding, blobs of 1, 478, 479, 960 and 961 bytes, a namespace-padding
    share, tail padding: the one- and two-share boundaries exactly."""
    sq = osq.compact_shares(TX_NS, [data(100, 1), data(30, 2)]) + osq.compact_shares(PFB_NS, [data(60, 3)])
    sq.append(osq.padding_share(RESERVED))
    counts = []
    for i, n in enumerate(BOUNDARY_LENGTHS):
        sh = osq.sparse_shares(ns(i + 1), data(n, 10 + i))
        counts.append(len(sh))
        sq += sh
    assert counts == [1, 1, 2, 2, 3]
    sq.append(osq.padding_share(ns(len(BOUNDARY_LENGTHS))))
    assert len(sq) == 13
    return fill(sq, 4)


def k4_row_crossing():
    """A 6-share blob starting at share 3: rows 0, 1 and 2 of a k = 4 square."""
    blob = osq.sparse_shares(ns(1), data(478 + 482 * 4 + 100, 5))
    assert len(blob) == 6
    sq = [osq.padding_share(RESERVED)] * 3 + blob
    assert {i // 4 for i in range(3, 9)} == {0, 1, 2}
    return fill(sq, 4)


def k4_last_share(full: bool):
    """A 3-share blob that ends in the square's last share: filling it to its last byte, or with 1 byte in it."""
    n = 478 + 482 * 2 if full else 478 + 482 + 1
    blob = osq.sparse_shares(ns(1), data(n, 6))
    assert len(blob) == 3
    sq = [osq.padding_share(RESERVED)] * 13 + blob
    assert len(sq) == 16
    if full:
        assert sq[-1][511] != 0
    else:
        assert sq[-1][30] != 0 and sq[-1][31:] == bytes(481)
    return sq


ALIGN_LENGTHS = (961,) * 8 + (1442, 1000, 965)


def k8_alignment():
    """3-share blobs whose packed start offsets take every residue mod 8 (961 = 1 mod 8), with 1-share blobs
    of odd lengths between some of them."""
    sq, off, residues, i = [], 0, set(), 1
    for j, n in enumerate(ALIGN_LENGTHS):
        sh = osq.sparse_shares(ns(i), data(n, 20 + j))
        assert len(sh) == 3
        residues.add(off % 8)
        sq += sh
        off += n
        i += 1
        if j >= 8:
            sq += osq.sparse_shares(ns(i), data(3 + j, 40 + j))
            off += 3 + j
            i += 1
    assert residues == set(range(8)), residues
    return fill(sq, 8)


COMPACT_TX_UNITS = (471, 200, 275, 1200, 50)


def k4_compact_edges():
    """A TX sequence of five shares and a PFB sequence behind it:
    unit 1's two-byte length prefix straddles shares 0 and 1 (byte 511 of share 0 is its first byte, >= 0x80);
    unit 2 ends exactly at share 1's end, so share 2's reserved bytes are 34;
    unit 3 has 1 200 bytes, so share 3, which it covers, has reserved bytes 0."""
    txs = [data(n, 50 + i) for i, n in enumerate(COMPACT_TX_UNITS)]
    tx_sh = osq.compact_shares(TX_NS, txs)
    pfb_sh = osq.compact_shares(PFB_NS, [data(300, 60), data(400, 61)])
    assert len(tx_sh) == 5 and len(pfb_sh) == 2
    res = lambda s, first: int.from_bytes(s[34:38] if first else s[30:34], "big")   # noqa: E731
    assert tx_sh[0][511] >= 0x80 and tx_sh[0][511] == (200 & 0x7F) | 0x80 and tx_sh[1][34] == 200 >> 7
    assert res(tx_sh[0], True) == 38 and res(tx_sh[2], False) == 34 and res(tx_sh[3], False) == 0
    assert res(tx_sh[4], False) == 34 + (474 + 478 + 1202 - (474 + 3 * 478))
    assert res(pfb_sh[0], True) == 38
    return fill(tx_sh + pfb_sh, 4)


def edge_squares():
    return {"k1": k1(), "k4_boundary": k4_boundary(), "k4_row_crossing": k4_row_crossing(),
            "k4_last_full": k4_last_share(True), "k4_last_one": k4_last_share(False), "k8_alignment": k8_alignment(),
            "k4_compact_edges": k4_compact_edges()}


def _patch(share: bytes, at: int, new: bytes) -> bytes:
    return share[:at] + new + share[at + len(new):]


def invalid_squares():
    """{name: (k = 4 square, the error text)}: one square per error class, each a valid square with one change."""
    out = {}
    base = k4_boundary()      # 0 tx, 1 pfb, 2 reserved, 3 blob(1), 4 blob(478), 5-6 blob(479), 7-8 blob(960), 9-11 blob(961)
    s = list(base)
    s[0] = _patch(s[0], 29, b"\x00")
    out["first_is_continuation"] = (s, "share 0: the first share of the input is a continuation share")
    s = list(base)
    s[6] = _patch(s[6], 28, b"\x7f")
    out["continuation_namespace"] = (s, "share 6: continuation share's namespace differs from that of its "
                                        "sequence's start share 5")
    s = list(base)
    s[4] = _patch(s[4], 29, b"\x03")
    out["share_version"] = (s, "share 4: unsupported share version 1")
    s = list(base)
    s[13] = PARITY_NS + s[13][29:]
    out["parity_namespace"] = (s, "share 13: parity-namespace share")
    s = list(base)
    s[11] = osq.padding_share(ns(5))            # the 961-byte blob loses its third share
    out["too_few_shares"] = (s, "sequence at share 9: length 961 needs 3 shares, found 2")
    s = list(base)
    s[4] = _patch(s[4], 29, b"\x00")             # the 478-byte blob becomes a continuation of the 1-byte one
    s[4] = s[3][:29] + s[4][29:]
    out["too_many_shares"] = (s, "sequence at share 3: length 1 needs 1 shares, found 2")
    s = list(base)
    s[0] = _patch(s[0], 30, (475).to_bytes(4, "big"))
    out["compact_count"] = (s, "sequence at share 0: length 475 needs 2 shares, found 1")
    s = list(base)
    s[13] = _patch(s[12], 29, b"\x00")           # a continuation behind the namespace-padding share, in its namespace
    out["padding_continued"] = (s, "sequence at share 12: length 0 needs 1 shares, found 2")
    s = list(base)
    s[1] = _patch(s[1], 38, b"\xff" * 10)
    out["malformed_prefix"] = (s, "share 1: malformed unit length prefix")
    s = list(base)
    s[1] = _patch(s[1], 38, b"\x50")             # 80 bytes claimed, 60 left of L = 61
    out["unit_past_length"] = (s, "share 1: unit of 80 bytes runs past the sequence length 61")
    s = list(base)
    s[0] = _patch(s[0], 34, (39).to_bytes(4, "big"))
    out["reserved_bytes"] = (s, "share 0: reserved bytes 39, expected 38")
    return out
