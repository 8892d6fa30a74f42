"""Guarded buffers: a caller-owned buffer placed inside a larger allocation,
so that what a call writes next to the place it was told to write shows.

One allocation holds lead | payload | trail.  Lead and trail are at least 4096
bytes and at least one element stride of the output (one square's W*90 roots,
one share row, ...), so a stride wrong by one element still lands inside them.
The payload address is congruent, modulo 256, to the alignment asked for (256
itself meaning 0) and to nothing larger, so an argument can be placed at
exactly the minimum alignment include/cda.h documents for it.  The whole
allocation, payload included, holds a position-dependent byte pattern: a call
that writes zeros, a constant, or leaves stale memory differs from it.

Two backends with one interface: "numpy" (host buffers; the payload is never
page-aligned, because several entry points register the caller's pages) and
"torch" (a uint8 device tensor; guards and payload are compared on the device
against a regenerated pattern, nothing is downloaded but the bytes of a
failure report).

    g = guarded.alloc(n * W * 90, stride=W * 90, align=2, backend="torch", name="d_row_roots")
    call(..., g.ptr, ...)
    g.assert_written(expected)          # payload == expected, byte for byte
    g.assert_guards()                   # lead and trail still hold the pattern

    i = guarded.from_data(ods, align=16, backend="torch", name="d_ods")   # a const input
    i.assert_unchanged()                # payload and guards

The module imports without a GPU; torch is imported when a device buffer is
made.
"""
from __future__ import annotations

import numpy as np

GUARD_MIN = 4096
MODULUS = 256


def pattern_bytes(lo: int, hi: int) -> np.ndarray:
    """Bytes [lo, hi) of the fill pattern, by position in the allocation.  Odd
    multiplier: consecutive bytes all differ; the higher terms break the
    256-byte period, so two shares or two root arrays never hold equal fill."""
    i = np.arange(lo, hi, dtype=np.uint64)
    return ((131 * i + 7 + 29 * (i >> np.uint64(8)) + 3 * (i >> np.uint64(16))) & np.uint64(0xFF)).astype(np.uint8)


def _pattern_torch(lo: int, hi: int, device):
    import torch
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    return ((131 * i + 7 + 29 * (i >> 8) + 3 * (i >> 16)) & 0xFF).to(torch.uint8)


class GuardError(AssertionError):
    pass


class Guarded:
    """One guarded buffer; make it with alloc() or from_data()."""

    def __init__(self, size: int, stride: int = 0, align: int = MODULUS, backend: str = "numpy", name: str = "buffer",
                 device=None):
        assert backend in ("numpy", "torch"), backend
        assert 1 <= align <= MODULUS and align & (align - 1) == 0, align
        self.size, self.align, self.backend, self.name = int(size), align, backend, name
        guard = max(GUARD_MIN, int(stride))
        total = guard + 2 * MODULUS + self.size + guard
        if backend == "numpy":
            self._raw = np.empty(total, dtype=np.uint8)
            base = self._raw.ctypes.data
        else:
            import torch
            self._device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
            self._raw = torch.empty(total, dtype=torch.uint8, device=self._device)
            base = self._raw.data_ptr()
        off = guard + (align % MODULUS - (base + guard)) % MODULUS
        if backend == "numpy" and (base + off) % 4096 == 0:
            off += MODULUS     # host payloads are never page-aligned
        self.lead, self.trail = off, total - off - self.size
        assert self.lead >= guard and self.trail >= guard
        self.ptr = base + off
        assert self.ptr % MODULUS == align % MODULUS
        self._total = total
        self._saved = None
        self.refill()

    # ------------------------------------------------------------------ contents
    def refill(self):
        """The pattern over the whole allocation again (before a second run)."""
        if self.backend == "numpy":
            self._raw[:] = pattern_bytes(0, self._total)
        else:
            self._raw.copy_(_pattern_torch(0, self._total, self._device))
        self._saved = None

    def payload(self):
        """The payload, a view (numpy array or device tensor of uint8)."""
        return self._raw[self.lead:self.lead + self.size]

    def payload_host(self) -> np.ndarray:
        """A host copy of the payload."""
        p = self.payload()
        return p.copy() if self.backend == "numpy" else p.cpu().numpy()

    def pattern(self, lo: int = 0, hi: int | None = None) -> np.ndarray:
        """The fill of payload bytes [lo, hi): what the contract's untouched parts must still hold."""
        hi = self.size if hi is None else hi
        return pattern_bytes(self.lead + lo, self.lead + hi)

    def set(self, data):
        """Fill the payload with `data` (an input buffer) and remember it for assert_unchanged()."""
        a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert a.size == self.size, (self.name, a.size, self.size)
        if self.backend == "numpy":
            self.payload()[:] = a
        else:
            import torch
            self.payload().copy_(torch.from_numpy(a.copy()).to(self._device))
        self._saved = a.copy()
        return self

    # ------------------------------------------------------------------ checks
    def _first_diff(self, lo: int, hi: int, want: np.ndarray):
        """(offset in [lo, hi) of the first byte of the allocation that differs from want, got, want) or None."""
        if self.backend == "numpy":
            got = self._raw[lo:hi]
            if np.array_equal(got, want):
                return None
            o = int(np.nonzero(got != want)[0][0])
            return o, int(got[o]), int(want[o])
        import torch
        want = np.ascontiguousarray(want)
        w = torch.from_numpy(want if want.flags.writeable else want.copy()).to(self._device)
        got = self._raw[lo:hi]
        if torch.equal(got, w):
            return None
        o = int((got != w).nonzero()[0])
        return o, int(got[o]), int(w[o])

    def _guard_diff(self, lo: int, hi: int):
        if self.backend == "numpy":
            return self._first_diff(lo, hi, pattern_bytes(lo, hi))
        import torch
        w = _pattern_torch(lo, hi, self._device)
        got = self._raw[lo:hi]
        if torch.equal(got, w):
            return None
        o = int((got != w).nonzero()[0])
        return o, int(got[o]), int(w[o])

    def assert_guards(self, name: str | None = None):
        """Lead and trail still hold the pattern; the failure names the buffer, the side, and the offset (from
        the payload's start before it, from its end after it) and value of the first changed byte."""
        name = name or self.name
        d = self._guard_diff(0, self.lead)
        if d is not None:
            raise GuardError(f"{name}: guard before the payload changed at offset {d[0] - self.lead} "
                             f"(payload start = 0): holds 0x{d[1]:02x}, pattern 0x{d[2]:02x}")
        end = self.lead + self.size
        d = self._guard_diff(end, self._total)
        if d is not None:
            raise GuardError(f"{name}: guard after the payload changed at offset +{d[0]} past the end "
                             f"(payload size {self.size}): holds 0x{d[1]:02x}, pattern 0x{d[2]:02x}")

    def assert_written(self, expected, written=None, name: str | None = None):
        """The payload equals `expected` wherever the contract says the call writes (`written`: a boolean mask
        over the payload's bytes, None = all of it) and the pattern everywhere else.  A differing byte that
        still holds the pattern is reported as not written."""
        name = name or self.name
        e = np.ascontiguousarray(expected).reshape(-1).view(np.uint8)
        assert e.size == self.size, (name, e.size, self.size)
        pat = self.pattern()
        if written is None:
            want, mask = e, None
        else:
            mask = np.ascontiguousarray(written).reshape(-1).astype(bool)
            assert mask.size == self.size, (name, mask.size, self.size)
            want = np.where(mask, e, pat)
        d = self._first_diff(self.lead, self.lead + self.size, want)
        if d is None:
            return
        o, got, w = d
        if mask is not None and not mask[o]:
            raise GuardError(f"{name}: payload byte {o} is outside what the call may write and changed: "
                             f"holds 0x{got:02x}, pattern 0x{w:02x}")
        if got == int(pat[o]):
            raise GuardError(f"{name}: payload byte {o} was not written: still the pattern 0x{got:02x}, "
                             f"expected 0x{w:02x}")
        raise GuardError(f"{name}: payload byte {o} holds 0x{got:02x}, expected 0x{w:02x}")

    def assert_untouched(self, name: str | None = None):
        """Payload and guards all still hold the pattern (an output of a call that must write nothing)."""
        self.assert_written(self.pattern(), np.zeros(self.size, bool), name)
        self.assert_guards(name)

    def assert_unchanged(self, name: str | None = None):
        """An input filled by set(): payload byte-identical, guards intact."""
        name = name or self.name
        assert self._saved is not None, f"{name}: assert_unchanged() needs set() first"
        d = self._first_diff(self.lead, self.lead + self.size, self._saved)
        if d is not None:
            raise GuardError(f"{name}: const input changed at byte {d[0]}: holds 0x{d[1]:02x}, was 0x{d[2]:02x}")
        self.assert_guards(name)


def alloc(size: int, stride: int = 0, align: int = MODULUS, backend: str = "numpy", name: str = "buffer", device=None):
    return Guarded(size, stride, align, backend, name, device)


def from_data(data, stride: int = 0, align: int = MODULUS, backend: str = "numpy", name: str = "input", device=None):
    a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    return Guarded(a.size, stride, align, backend, name, device).set(a)
