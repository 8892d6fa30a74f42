"""Mirror of go-square v1.1.0 ``shares.ParseShares`` / ``ParseTxs`` /
``ParseBlobs`` over libcda.so: a square's shares back into its transactions,
IndexWrappers and blobs (include/cda.h, "Shares back into transactions and
blobs"; the rules are restated from the published algorithms and
specs/src/specs/shares.md).

The functions here take host shares and run the library's host-only calls
(cda_shares_parse_plan / cda_shares_parse); proof.ResidentSquare.parse runs the
same parse over a resident square on the GPU and returns the same ParsedSquare.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import SHARE_SIZE, ptr
from .inclusion import Blob

NAMESPACE_SIZE = 29


@dataclass
class ParsedSquare:
    """What a parse returns.  Share indexes are row-major indexes of the
    original square (of the input, for the host functions)."""
    txs: list = field(default_factory=list)            # the TX namespace's units
    pfbs: list = field(default_factory=list)           # the PFB namespace's units: raw IndexWrapper bytes
    blobs: list = field(default_factory=list)          # inclusion.Blob (data empty for a table-only parse)
    blob_starts: list = field(default_factory=list)    # first share of each blob
    blob_share_lens: list = field(default_factory=list)
    blob_off: list = field(default_factory=list)       # n_blobs + 1 offsets into the packed blob bytes
    tx_ranges: list = field(default_factory=list)      # (start, end) shares of each tx, length prefix included
    pfb_ranges: list = field(default_factory=list)
    n_padding_shares: int = 0


def plan_dict(p: _lib.ParsePlanT) -> dict:
    return {n: getattr(p, n) for n, _ in _lib.ParsePlanT._fields_}


class ParseBuffers:
    """Host arrays of a plan's sizes and the cda_parse_out that points at them."""

    def __init__(self, plan: _lib.ParsePlanT, blob_data: bool = True):
        nb, nu = plan.n_blobs, plan.n_txs + plan.n_pfbs
        self.plan = plan
        self.blob_start = np.zeros(max(1, nb), dtype=np.uint32)
        self.blob_shares = np.zeros(max(1, nb), dtype=np.uint32)
        self.blob_namespace = np.zeros(max(1, nb) * NAMESPACE_SIZE, dtype=np.uint8)
        self.blob_share_version = np.zeros(max(1, nb), dtype=np.uint8)
        self.blob_off = np.zeros(nb + 1, dtype=np.uint64)
        self.blob_data = np.zeros(max(1, plan.blob_bytes), dtype=np.uint8) if blob_data else None
        self.unit_off = np.zeros(nu + 1, dtype=np.uint64)
        self.unit_data = np.zeros(max(1, plan.unit_bytes), dtype=np.uint8)
        self.unit_start = np.zeros(max(1, nu), dtype=np.uint32)
        self.unit_end = np.zeros(max(1, nu), dtype=np.uint32)

    def out_struct(self) -> _lib.ParseOut:
        o = _lib.ParseOut()
        for name, ctype in _lib.ParseOut._fields_:
            a = getattr(self, name)
            setattr(o, name, None if a is None else a.ctypes.data_as(ctype))
        return o

    def parsed(self) -> ParsedSquare:
        p = self.plan
        nb, nt, nu = p.n_blobs, p.n_txs, p.n_txs + p.n_pfbs
        uo, ud = [int(x) for x in self.unit_off], self.unit_data.tobytes()
        units = [ud[uo[i]:uo[i + 1]] for i in range(nu)]
        ranges = [(int(self.unit_start[i]), int(self.unit_end[i])) for i in range(nu)]
        bo, ns = [int(x) for x in self.blob_off], self.blob_namespace.tobytes()
        bd = self.blob_data.tobytes() if self.blob_data is not None else None
        blobs = [Blob(ns[i * NAMESPACE_SIZE:(i + 1) * NAMESPACE_SIZE], bd[bo[i]:bo[i + 1]] if bd is not None else b"",
                      int(self.blob_share_version[i])) for i in range(nb)]
        return ParsedSquare(txs=units[:nt], pfbs=units[nt:], blobs=blobs,
                            blob_starts=[int(x) for x in self.blob_start[:nb]],
                            blob_share_lens=[int(x) for x in self.blob_shares[:nb]], blob_off=bo,
                            tx_ranges=ranges[:nt], pfb_ranges=ranges[nt:], n_padding_shares=p.n_padding_shares)


def _shares_array(raw) -> np.ndarray:
    if isinstance(raw, (list, tuple)):
        raw = b"".join(bytes(s) for s in raw)
    a = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    if a.size % SHARE_SIZE:
        raise ValueError(f"{a.size} bytes are not a whole number of {SHARE_SIZE}-byte shares")
    return a


def _check(L, rc: int):
    if rc != _lib.CDA_OK:
        msg = L.cda_last_error(None).decode()
        raise (_lib.SquareError if rc == _lib.CDA_ERR_SQUARE else _lib.CdaError)(rc, msg)


def parse_plan(raw) -> dict:
    """cda_shares_parse_plan: the counts and byte sizes of what `raw` parses to."""
    a, L, p = _shares_array(raw), _lib.load(), _lib.ParsePlanT()
    _check(L, L.cda_shares_parse_plan(ptr(a) if a.size else None, a.size // SHARE_SIZE, C.byref(p)))
    return plan_dict(p)


def parse_shares(raw, ignore_padding: bool = True) -> ParsedSquare:
    """shares.ParseShares over the shares of `raw` (bytes, an array, or a list
    of 512-byte shares): every sequence, as a ParsedSquare.  The parse skips
    and counts padding; ignore_padding=False is for a caller that expects
    payload only and raises SquareError naming the count if there is any."""
    a, L, p = _shares_array(raw), _lib.load(), _lib.ParsePlanT()
    src, n = (ptr(a) if a.size else None), a.size // SHARE_SIZE
    _check(L, L.cda_shares_parse_plan(src, n, C.byref(p)))
    if not ignore_padding and p.n_padding_shares:
        raise _lib.SquareError(_lib.CDA_ERR_SQUARE, f"{p.n_padding_shares} padding shares in the input")
    buf = ParseBuffers(p)
    o = buf.out_struct()
    _check(L, L.cda_shares_parse(src, n, C.byref(o)))
    return buf.parsed()


def parse_txs(raw) -> list:
    """shares.ParseTxs: the units of compact shares (TX namespace units, then
    the PFB namespace's); raises SquareError if a sparse sequence is present."""
    p = parse_shares(raw)
    if p.blobs:
        raise _lib.SquareError(_lib.CDA_ERR_SQUARE, f"sparse sequence at share {p.blob_starts[0]} among compact shares")
    return p.txs + p.pfbs


def parse_blobs(raw) -> list:
    """shares.ParseBlobs: the blobs of sparse shares as inclusion.Blob; raises
    SquareError if a compact sequence is present."""
    p = parse_shares(raw)
    if p.txs or p.pfbs:
        at = (p.tx_ranges + p.pfb_ranges)[0][0]
        raise _lib.SquareError(_lib.CDA_ERR_SQUARE, f"compact sequence at share {at} among sparse shares")
    return p.blobs


def _uvarint(buf: bytes, i: int):
    v = shift = 0
    while True:
        if i >= len(buf) or shift > 63:
            raise ValueError("malformed varint")
        c = buf[i]
        i += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if c < 0x80:
            return v, i


def unmarshal_index_wrapper(unit: bytes):
    """(tx, share_indexes) of an IndexWrapper{tx = 1, share_indexes = 2 (packed
    or not), type_id = 3 == "INDX"}: the inverse of what the square writes for
    a blob tx.  ValueError if `unit` is not one."""
    tx, idx, type_id, i = b"", [], b"", 0
    unit = bytes(unit)
    while i < len(unit):
        key, i = _uvarint(unit, i)
        fn, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _uvarint(unit, i)
            if fn == 2:
                idx.append(v)
        elif wt == 2:
            n, i = _uvarint(unit, i)
            if i + n > len(unit):
                raise ValueError("field beyond the message")
            v, i = unit[i:i + n], i + n
            if fn == 1:
                tx = v
            elif fn == 2:
                j = 0
                while j < len(v):
                    x, j = _uvarint(v, j)
                    idx.append(x)
            elif fn == 3:
                type_id = v
        elif wt in (1, 5):
            i += 8 if wt == 1 else 4
        else:
            raise ValueError(f"wire type {wt}")
    if type_id != b"INDX":
        raise ValueError("not an IndexWrapper: type_id is not INDX")
    return tx, idx
