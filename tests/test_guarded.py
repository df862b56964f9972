"""The guarded-buffer helper itself (tests/guarded.py), on host tensors."""
import numpy as np
import pytest
import torch

from guarded import ALIGN, GUARD, Arena, GuardError, Plain


def _offset(arena, view):
    return view.data_ptr() - arena._buf.data_ptr()


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_payloads_are_aligned_exact_and_hold_the_fill(fill):
    a = Arena("cpu", fill, capacity=1 << 20)
    x = a.put(np.arange(7, dtype=np.int32), "x")
    o = a.out((3, 5), torch.float16, "o")
    r = a.raw(1001, "r")
    e = a.raw(0, "empty")
    k = a.out((4,), torch.int64, "k")
    assert x.dtype == torch.int32 and x.tolist() == list(range(7))
    assert (o.shape, o.dtype, o.numel() * o.element_size()) == ((3, 5), torch.float16, 30)
    assert r.numel() == 1001 and r.dtype == torch.uint8 and e.numel() == 0
    for v in (x, o, r, k):
        assert v.data_ptr() % ALIGN == 0
    assert bool((o.view(torch.uint8) == fill).all()) and bool((r == fill).all()) and bool((k.view(torch.uint8) == fill).all())
    # 64 KiB of guard before every payload, and guard from the first byte past its end
    offs = [(_offset(a, v), v.numel() * v.element_size()) for v in (x, o, r)] + [(_offset(a, k), 32)]
    assert offs[0][0] >= GUARD
    for (lo0, n0), (lo1, _) in zip(offs, offs[1:]):
        assert lo1 - (lo0 + n0) >= GUARD
    assert a._buf.numel() - (offs[-1][0] + offs[-1][1]) >= GUARD
    a.check()
    for v in (o, r, k):
        a.untouched(v)


def test_one_byte_overrun_names_the_payload():
    a = Arena("cpu", 0xFF, capacity=1 << 20)
    a.put(np.zeros(3, np.float32), "first")
    r = a.raw(1001, "victim")          # ends 1 byte past an odd address: the guard starts there, not at the next aligned byte
    a.out((8,), torch.int32, "last")
    a.check()
    lo = _offset(a, r)
    a._buf[lo + 1001] = 0              # a torch write one byte past the end
    with pytest.raises(GuardError) as e:
        a.check()
    msg = str(e.value)
    assert "'victim'" in msg and "AFTER" in msg and "first at +0, last at +0" in msg
    assert "'first'" not in msg and "'last'" not in msg
    # the same value as the fill is invisible in this arena and visible in the other one: hence two fills
    b = Arena("cpu", 0x00, capacity=1 << 20)
    rb = b.raw(1001, "victim")
    b._buf[_offset(b, rb) + 1001] = 0
    b.check()
    b._buf[_offset(b, rb) + 1001] = 0xFF
    with pytest.raises(GuardError):
        b.check()


def test_underrun_and_far_overrun_are_reported():
    a = Arena("cpu", 0x00, capacity=1 << 20)
    a.raw(10, "p0")
    r = a.out((16,), torch.float32, "p1")
    lo = _offset(a, r)
    a._buf[lo - 4:lo] = 7
    with pytest.raises(GuardError) as e:
        a.check()
    assert "'p1'" in str(e.value) and "BEFORE" in str(e.value) and "first at -4, last at -1" in str(e.value)
    a._buf[lo - 4:lo] = 0
    a.check()
    a._buf[lo + 64 + GUARD - 1] = 1    # the last guard byte of the last payload
    with pytest.raises(GuardError) as e:
        a.check()
    assert "'p1'" in str(e.value) and "AFTER" in str(e.value) and f"+{GUARD - 1}" in str(e.value)
    # the first payload's front guard
    c = Arena("cpu", 0x00, capacity=1 << 20)
    f = c.raw(5, "front")
    c._buf[_offset(c, f) - GUARD] = 9
    with pytest.raises(GuardError) as e:
        c.check()
    assert "'front'" in str(e.value) and "BEFORE" in str(e.value)


def test_untouched_sees_payloads_slices_and_pitched_columns():
    a = Arena("cpu", 0xFF, capacity=1 << 20)
    y = a.out((6, 24), torch.float16, "y")
    a.untouched(y)
    y[:, :16] = 1.0                    # live columns written, the gap columns c .. pitch-1 left alone
    a.untouched(y[:, 16:])
    a.untouched(y[4:, 16:])
    with pytest.raises(GuardError) as e:
        a.untouched(y)
    assert "'y'" in str(e.value)
    y[5, 23] = 0.0
    with pytest.raises(GuardError):
        a.untouched(y[:, 16:])
    a.untouched(y[:5, 16:])
    a.untouched(y[0:0])
    a.check()                          # writes inside a payload never trip the guards


def test_short_workspace_and_plain_interface():
    a = Arena("cpu", 0xFF, capacity=1 << 20, short=1)
    ws, n = a.ws(4096)
    assert (n, ws.numel()) == (4095, 4095) and a.ws_sizes == [("ws", 4096)]
    ws0, n0 = a.ws(0, "none")
    assert n0 == 0 and ws0.numel() == 0
    p = Plain("cpu")
    x = p.put(np.arange(4, dtype=np.int64))
    assert x.tolist() == [0, 1, 2, 3] and p.out((2, 3), torch.float32).shape == (2, 3)
    ws, n = p.ws(100)
    assert n == 100 and ws.numel() == 100
    p.check()
    p.untouched(x)


def test_arena_refuses_to_overflow():
    a = Arena("cpu", 0, capacity=4 * GUARD)
    a.raw(GUARD, "a")
    with pytest.raises(MemoryError):
        a.raw(2 * GUARD, "b")
