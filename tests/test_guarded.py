"""tests/guarded.py checks itself: a one-byte change planted in either guard of
a numpy-backed buffer is reported with the buffer's name, the side, the offset
and the value; a payload left as pattern is reported as not written; the
placement rules (guard size, alignment residue, no page-aligned host payload)
hold.  CPU only."""
import numpy as np
import pytest

import guarded


def test_layout_rules():
    for size, stride, align in [(1, 0, 1), (90 * 4, 90 * 4, 2), (32 * 3, 32, 4), (512 * 16, 4 * 512, 16),
                                (8192, 5000, 8), (100, 0, 256)]:
        g = guarded.alloc(size, stride=stride, align=align)
        assert g.lead >= max(4096, stride) and g.trail >= max(4096, stride)
        assert g.ptr % 256 == align % 256            # this alignment and nothing larger (below 256)
        assert g.ptr % 4096 != 0                     # host payloads are never page-aligned
        assert g.ptr == g.payload().ctypes.data and g.payload().size == size
        g.assert_guards()
        g.assert_untouched()


def test_pattern_is_position_dependent():
    p = guarded.pattern_bytes(0, 1 << 17)
    assert (p[1:] != p[:-1]).all()                   # no run of equal bytes: no constant fill hides in it
    assert not np.array_equal(p[:512], p[512:1024])  # and no share-sized period
    assert not np.array_equal(p[:256], p[256:512])
    assert len(set(p[:256].tolist())) == 256
    g = guarded.alloc(300, align=2)
    assert np.array_equal(g.payload(), g.pattern()) and np.array_equal(g.pattern(10, 20), g.pattern()[10:20])


@pytest.mark.parametrize("where", ["lead-1", "size", "last trail byte", "first lead byte"])
def test_planted_guard_byte_is_reported(where):
    g = guarded.alloc(180, stride=180, align=2, name="row_roots")
    g.assert_written(g.pattern(), np.zeros(180, bool))
    raw = g._raw
    at = {"lead-1": g.lead - 1, "size": g.lead + g.size, "last trail byte": raw.size - 1, "first lead byte": 0}[where]
    old = int(raw[at])
    raw[at] = old ^ 0x5A
    with pytest.raises(guarded.GuardError) as e:
        g.assert_guards()
    text = str(e.value)
    assert text.startswith("row_roots: guard ")
    if at < g.lead:
        assert f"before the payload changed at offset {at - g.lead} " in text
    else:
        assert f"after the payload changed at offset +{at - g.lead - g.size} " in text
    assert f"holds 0x{old ^ 0x5A:02x}, pattern 0x{old:02x}" in text
    # the payload itself is not blamed
    g.assert_written(g.pattern(), np.zeros(180, bool))
    raw[at] = old
    g.assert_guards()
    with pytest.raises(guarded.GuardError, match="^other name: guard "):
        raw[at] = old ^ 1
        g.assert_guards("other name")


def test_unwritten_payload_is_reported():
    g = guarded.alloc(64, align=4, name="data_roots")
    want = np.arange(64, dtype=np.uint8)
    want[want == g.pattern()] ^= 0x80              # an expectation that differs from the fill everywhere
    with pytest.raises(guarded.GuardError, match=r"^data_roots: payload byte 0 was not written: still the pattern"):
        g.assert_written(want)
    g.payload()[:] = want
    g.assert_written(want)
    g.payload()[40] = g.pattern()[40]              # one byte the call skipped
    with pytest.raises(guarded.GuardError, match=r"payload byte 40 was not written"):
        g.assert_written(want)
    g.payload()[40] = want[40] ^ 1                 # one wrong byte
    if g.payload()[40] == g.pattern()[40]:
        g.payload()[40] = want[40] ^ 2
    with pytest.raises(guarded.GuardError, match=rf"payload byte 40 holds 0x{int(g.payload()[40]):02x}, expected"):
        g.assert_written(want)


def test_written_mask_keeps_the_rest_as_pattern():
    g = guarded.alloc(100, align=1, name="nodes")
    want = np.full(100, 0xEE, dtype=np.uint8)
    mask = np.zeros(100, bool)
    mask[:30] = True
    g.payload()[:30] = 0xEE
    g.assert_written(want, mask)
    with pytest.raises(guarded.GuardError, match="payload byte 30 was not written"):
        g.assert_written(want)                     # all of it was expected
    g.payload()[77] ^= 0xFF                        # a store past what the call reported
    with pytest.raises(guarded.GuardError, match="nodes: payload byte 77 is outside what the call may write"):
        g.assert_written(want, mask)
    with pytest.raises(guarded.GuardError, match="payload byte 0 is outside"):
        g.assert_untouched()


def test_inputs_are_compared_with_what_was_set():
    data = np.arange(1000, dtype=np.uint16)
    g = guarded.from_data(data, align=16, name="ods")
    assert g.size == 2000 and g.ptr % 256 == 16
    assert np.array_equal(g.payload_host().view(np.uint16), data)
    g.assert_unchanged()
    g.payload()[1999] ^= 1
    with pytest.raises(guarded.GuardError, match="^ods: const input changed at byte 1999"):
        g.assert_unchanged()
    g.payload()[1999] ^= 1
    g._raw[g.lead + g.size] ^= 1
    with pytest.raises(guarded.GuardError, match=r"^ods: guard after the payload changed at offset \+0 "):
        g.assert_unchanged()
    g.refill()
    with pytest.raises(AssertionError, match="needs set"):
        g.assert_unchanged()
