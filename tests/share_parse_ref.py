"""Shares back into transactions and blobs -- a pure-Python restatement of the
rules of include/cda.h ("Shares back into transactions and blobs"), TEST
INFRASTRUCTURE ONLY.  It shares no code with the product: the rules are written
out again from the issue's text and specs/src/specs/shares.md.

    parse(raw, ranges=None) -> Parsed      (raises ParseError with the product's text)

raw: the shares, concatenated (bytes).  ranges: [(start, end)] share ranges, each
an input of its own; None = the whole input.  Indexes reported are indexes into
raw's shares.
"""
from __future__ import annotations

from dataclasses import dataclass, field

SHARE = 512
NS = 29
TX_NS = bytes(28) + b"\x01"
PFB_NS = bytes(28) + b"\x04"
RESERVED_PADDING_NS = bytes(28) + b"\xff"
TAIL_PADDING_NS = b"\xff" * 28 + b"\xfe"
PARITY_NS = b"\xff" * 29


class ParseError(ValueError):
    pass


@dataclass
class Parsed:
    n_padding: int = 0
    blobs: list = field(default_factory=list)        # (namespace, share_version, data, start, shares)
    txs: list = field(default_factory=list)          # (unit bytes, start share, end share)
    pfbs: list = field(default_factory=list)

    @property
    def plan(self):
        return dict(n_blobs=len(self.blobs), n_txs=len(self.txs), n_pfbs=len(self.pfbs),
                    n_padding_shares=self.n_padding, blob_bytes=sum(len(b[2]) for b in self.blobs),
                    unit_bytes=sum(len(u[0]) for u in self.txs + self.pfbs))


def sparse_needed(L: int) -> int:
    return 1 if L <= 478 else 1 + -(-(L - 478) // 482)


def compact_needed(L: int) -> int:
    return 1 if L <= 474 else 1 + -(-(L - 474) // 478)


def _sequences(raw: bytes, ranges, whole: bool):
    """[(start index, share count, L, class)] of the non-padding sequences, and the padding count."""
    seqs, n_padding = [], 0
    for r, (lo, hi) in enumerate(ranges):
        cur = None      # [start, count, L, cls, ns]

        def close():
            nonlocal cur, n_padding
            if cur is None:
                return
            start, cnt, L, cls, _ = cur
            need = 1 if cls == "padding" else compact_needed(L) if cls in ("tx", "pfb") else sparse_needed(L)
            if cnt != need:
                raise ParseError(f"sequence at share {start}: length {L} needs {need} shares, found {cnt}")
            if cls == "padding":
                n_padding += 1
            else:
                seqs.append((start, cnt, L, cls))
            cur = None

        for i in range(lo, hi):
            sh = raw[i * SHARE:(i + 1) * SHARE]
            ns, info = sh[:NS], sh[NS]
            if ns == PARITY_NS:
                raise ParseError(f"share {i}: parity-namespace share")
            if info >> 1:
                raise ParseError(f"share {i}: unsupported share version {info >> 1}")
            if info & 1:
                close()
                L = int.from_bytes(sh[30:34], "big")
                if L == 0 or ns in (TAIL_PADDING_NS, RESERVED_PADDING_NS):
                    cur = [i, 1, 0, "padding", ns]
                else:
                    cur = [i, 1, L, "tx" if ns == TX_NS else "pfb" if ns == PFB_NS else "blob", ns]
            else:
                if cur is None:
                    which = "the input" if whole else f"range {r}"
                    raise ParseError(f"share {i}: the first share of {which} is a continuation share")
                if ns != cur[4]:
                    raise ParseError(f"share {i}: continuation share's namespace differs from that of its "
                                     f"sequence's start share {cur[0]}")
                cur[1] += 1
        close()
    return seqs, n_padding


def _stream_share(p: int) -> int:
    return 0 if p < 474 else 1 + (p - 474) // 478


def _stream_offset(p: int) -> int:
    return 38 + p if p < 474 else 34 + (p - 474) % 478


def _units(raw: bytes, start: int, cnt: int, L: int):
    stream = b"".join(raw[(start + j) * SHARE + (38 if j == 0 else 34):(start + j + 1) * SHARE] for j in range(cnt))[:L]
    units, first_unit, p = [], {}, 0
    while p < L:
        p0, v, nb = p, 0, 0
        while True:
            if p >= L or (nb == 9 and stream[p] > 1):
                raise ParseError(f"share {start + _stream_share(p0)}: malformed unit length prefix")
            c = stream[p]
            p += 1
            v |= (c & 0x7F) << (7 * nb)
            nb += 1
            if c < 0x80:
                break
        if v == 0:
            break
        if p + v > L:
            raise ParseError(f"share {start + _stream_share(p0)}: unit of {v} bytes runs past the sequence length {L}")
        first_unit.setdefault(_stream_share(p0), _stream_offset(p0))
        units.append((stream[p:p + v], start + _stream_share(p0), start + _stream_share(p + v - 1) + 1))
        p += v
    for j in range(cnt):
        at = (start + j) * SHARE + (34 if j == 0 else 30)
        got, want = int.from_bytes(raw[at:at + 4], "big"), first_unit.get(j, 0)
        if got != want:
            raise ParseError(f"share {start + j}: reserved bytes {got}, expected {want}")
    return units


def parse(raw: bytes, ranges=None) -> Parsed:
    raw = bytes(raw)
    assert len(raw) % SHARE == 0
    n = len(raw) // SHARE
    whole = ranges is None or (len(ranges) == 1 and ranges[0][0] == 0)
    if ranges is None:
        ranges = [(0, n)] if n else []
    seqs, n_padding = _sequences(raw, ranges, whole)
    out = Parsed(n_padding=n_padding)
    for cls, dst in (("tx", out.txs), ("pfb", out.pfbs)):
        for start, cnt, L, c in seqs:
            if c == cls:
                dst += _units(raw, start, cnt, L)
    for start, cnt, L, c in seqs:
        if c != "blob":
            continue
        data = b"".join(raw[(start + j) * SHARE + (34 if j == 0 else 30):(start + j + 1) * SHARE] for j in range(cnt))[:L]
        out.blobs.append((raw[start * SHARE:start * SHARE + NS], raw[start * SHARE + NS] >> 1, data, start, cnt))
    return out
