"""Guarded buffers for the C ABI tests: payloads of an exact byte length inside one pre-filled arena.

`Arena(device, fill)` owns ONE uint8 tensor filled with the byte `fill` and hands out views of it.  Every payload starts at a
256-byte aligned offset (what the library's own carver and torch give the kernels), has GUARD bytes of fill in front of it, and
GUARD bytes of fill that begin AT ITS FIRST BYTE PAST THE END — not at the next aligned address — so that a store one byte
beyond a buffer, or a read of a byte the call never wrote, is visible: `check()` compares every guard byte with the fill and
`untouched(view)` does the same for a payload or a slice of one.  Works on host tensors as well (its own unit tests run there).

`Plain(device)` has the same interface over ordinary torch allocations: the reference side of a comparison.
"""
import numpy as np
import torch

GUARD = 64 * 1024
ALIGN = 256


def _as_tensor(a):
    if isinstance(a, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(a))
    return a.detach().contiguous()


def _nbytes(shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    return n


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, device, fill, capacity=32 << 20, short=0):
        self.device = torch.device(device)
        self.fill = int(fill) & 0xFF
        self.short = int(short)          # bytes that `ws()` withholds from the size it is asked for
        self.ws_sizes = []               # (name, published bytes) of every `ws()` payload
        self.outs = []                   # every `out()` payload: what a refused call must leave alone
        self._buf = torch.full((capacity,), self.fill, dtype=torch.uint8, device=self.device)
        base = self._buf.data_ptr()
        self._skew = (-base) % ALIGN     # torch allocations are at least 256-byte aligned on a device; host ones need not be
        self._top = 0                    # first byte (relative to the skewed base) that no payload or guard owns yet
        self._items = []                 # (name, start, nbytes), offsets into _buf

    # ---- allocation ----
    def _take(self, nbytes, name):
        nbytes = int(nbytes)
        start = self._top + GUARD
        start += (-start) % ALIGN
        lo = self._skew + start
        if lo + nbytes + GUARD > self._buf.numel():
            raise MemoryError(f"arena of {self._buf.numel()} bytes is full at payload {name!r} ({nbytes} bytes)")
        self._top = start + nbytes       # the next payload's front guard begins right behind this payload's last byte
        name = name or f"#{len(self._items)}"
        self._items.append((name, lo, nbytes))
        return self._buf[lo:lo + nbytes]

    def raw(self, nbytes, name=None):
        """uint8 payload of exactly nbytes, holding the fill."""
        return self._take(nbytes, name)

    def out(self, shape, dtype, name=None):
        """Payload of exactly shape x dtype, holding the fill."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        v = self._take(_nbytes(shape, dtype), name).view(dtype).view(shape)
        self.outs.append(v)
        return v

    def put(self, array, name=None):
        """Copy a numpy array or tensor in; the view covers exactly its bytes."""
        t = _as_tensor(array)
        v = self._take(_nbytes(tuple(t.shape), t.dtype), name).view(t.dtype).view(tuple(t.shape))
        v.copy_(t)
        return v

    def ws(self, published, name="ws"):
        """Scratch for the entry under test: `published - short` bytes holding the fill; returns (view, its byte count)."""
        published = int(published)
        self.ws_sizes.append((name, published))
        n = max(published - self.short, 0)
        return self._take(n, name), n

    # ---- checks ----
    def _damage(self, lo, hi):
        seg = self._buf[lo:hi]
        bad = (seg != self.fill).nonzero()
        if bad.numel() == 0:
            return None
        return int(bad[0]), int(bad[-1]), int(bad.numel())

    def check(self):
        """Every guard byte still equals the fill; names the payload, the side and the first / last damaged offsets."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        problems = []
        items = self._items
        for i in range(len(items) + 1):
            # gap i lies between payload i-1 and payload i: at least GUARD bytes, all of them guard
            prev_end = items[i - 1][1] + items[i - 1][2] if i else max(items[0][1] - GUARD, 0) if items else 0
            nxt = items[i][1] if i < len(items) else min(prev_end + GUARD, self._buf.numel())
            d = self._damage(prev_end, nxt)
            if d is None:
                continue
            first, last, cnt = d
            mid = (nxt - prev_end) // 2
            if i > 0 and (first < mid or i == len(items)):
                name, _, n = items[i - 1]
                problems.append(f"payload {name!r} ({n} bytes): guard AFTER it damaged, {cnt} bytes, first at +{first}, last at "
                                f"+{last} past its end")
            if i < len(items) and (last >= mid or i == 0):
                name, _, n = items[i]
                gap = nxt - prev_end
                problems.append(f"payload {name!r} ({n} bytes): guard BEFORE it damaged, {cnt} bytes, first at {first - gap}, last "
                                f"at {last - gap} from its start")
        if problems:
            raise GuardError("; ".join(problems))

    def _locate(self, view):
        a = view.data_ptr() - self._buf.data_ptr()
        for name, lo, n in self._items:
            if lo <= a <= lo + n:
                return name, a - lo
        return "?", a

    def untouched(self, view):
        """The payload, or the slice of one, still holds the fill."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if view.numel() == 0:
            return
        flat = view.contiguous().view(-1).view(torch.uint8) if not view.is_contiguous() else view.reshape(-1).view(torch.uint8)
        bad = (flat != self.fill).nonzero()
        if bad.numel():
            name, off = self._locate(view)
            raise GuardError(f"payload {name!r}: region at byte {off} was written: {int(bad.numel())} of {flat.numel()} bytes "
                             f"differ from the fill, first at +{int(bad[0])}, last at +{int(bad[-1])}")


class Plain:
    """The same interface over ordinary allocations (no guards, no fill): what the rest of the suite hands the library."""
    short = 0

    def __init__(self, device):
        self.device = torch.device(device)
        self.fill = None
        self.ws_sizes = []
        self.outs = []

    def raw(self, nbytes, name=None):
        return torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)

    def out(self, shape, dtype, name=None):
        v = torch.empty(shape, dtype=dtype, device=self.device)
        self.outs.append(v)
        return v

    def put(self, array, name=None):
        return _as_tensor(array).to(self.device).clone()

    def ws(self, published, name="ws"):
        self.ws_sizes.append((name, int(published)))
        return self.raw(published), int(published)

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def untouched(self, view):
        pass
