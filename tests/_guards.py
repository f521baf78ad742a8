"""Test helper: device buffers placed inside larger, guarded allocations.

Every tensor torch allocates is sized exactly and 256-byte aligned, so a kernel that stores one row past `n`, spills a [T, N] row into
row t + 1 or sums a load of row `n` usually lands in allocator slack or reads zeros, and no test sees it.  A `Guards` arena places
each argument of a call at a chosen byte offset inside an allocation of its own, with at least 256 bytes in front and behind:
  * inputs: the data in the middle, the guards filled with POISON (NaN with a payload for floats, 0x01 / 0xFF for u8 flags,
    INT32_MAX for i32): a read of a guard turns into a NaN or an absurd count in the result;
  * outputs: the whole allocation prefilled with a CANARY bit pattern no kernel produces (a NaN with payload 0x7FC0DEAD ...);
  * in-out buffers (parameters and moments updated in place): the data in the middle, poisoned guards.
`check()` then asserts (i) every guard byte is unchanged, (ii) no canary is left where the contract says an output is written
(and, where given, that the canary is still there where it says nothing is written).  `run_both()` makes the call at two
placements -- every buffer at a 256-byte boundary, and every buffer at EXACTLY the minimum alignment the ABI allows for it (the
offset is that alignment plus a multiple of 256, so the pointer is not aligned any further) -- and asserts (iii) the outputs are
bit-identical.  The kernels add partial sums in a fixed order, so (iii) is exact.  No unguarded exact-size tensor is ever handed
out: a kernel that reads or writes one row too far stays inside memory the test allocated."""
import ctypes as C

import torch

GUARD = 256   # bytes of guard in front of and behind every placed buffer (at least)

# bit patterns, little-endian element values
_POISON = {torch.float32: 0x7FA0BAD1, torch.float16: 0x7E01, torch.float64: 0x7FF4BAD1BAD1BAD1, torch.int32: 0x7FFFFFFF,
           torch.uint8: None}   # u8: 0x01 / 0xFF alternating
_CANARY = {torch.float32: 0x7FC0DEAD, torch.float16: 0x7DEA, torch.float64: 0x7FF8DEAD0000DEAD, torch.int32: 0x7EADC0DE,
           torch.uint8: 0xA5}
_ITYPE = {torch.float32: torch.int32, torch.float16: torch.int16, torch.float64: torch.int64, torch.int32: torch.int32,
          torch.uint8: torch.uint8}


def _pattern(dtype, nbytes, device, canary):
    """`nbytes` bytes of the poison / canary pattern of `dtype` (nbytes a multiple of the element size)."""
    es = torch.empty((), dtype=dtype).element_size()
    n = nbytes // es
    if dtype == torch.uint8 and not canary:
        return torch.tensor([0x01, 0xFF], dtype=torch.uint8, device=device).repeat((n + 1) // 2)[:n]
    v = (_CANARY if canary else _POISON)[dtype]
    it = _ITYPE[dtype]
    if v >= 1 << (8 * es - 1):
        v -= 1 << (8 * es)
    return torch.full((n,), v, dtype=it, device=device).view(torch.uint8)


def canary_of(dtype):
    """The canary as a one-element tensor of `dtype` (CPU)."""
    return _pattern(dtype, torch.empty((), dtype=dtype).element_size(), "cpu", True).view(dtype)


def is_canary(t):
    """Elementwise: does `t` hold the canary bit pattern of its dtype?"""
    it = _ITYPE[t.dtype]
    c = canary_of(t.dtype).view(it).to(t.device)
    return t.contiguous().view(it) == c


class _Placed:
    def __init__(self, kind, buf, lo, nbytes, dtype, shape, written, untouched):
        self.kind, self.buf, self.lo, self.nbytes, self.dtype, self.shape = kind, buf, lo, nbytes, dtype, shape
        self.written, self.untouched = written, untouched
        self.view = buf[lo:lo + nbytes].view(dtype).view(shape)
        self.front0 = buf[:lo].clone()
        self.back0 = buf[lo + nbytes:].clone()


class Guards:
    """One placement of all buffers of a call.  minimal=False: every buffer at a 256-byte boundary; minimal=True: every buffer at
    exactly the alignment passed for it (the ABI's minimum for that argument)."""

    def __init__(self, device, minimal=False):
        self.device, self.minimal = torch.device(device), minimal
        self.placed = []

    def _place(self, kind, shape, dtype, align, fill, written=None, untouched=None):
        es = torch.empty((), dtype=dtype).element_size()
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * es
        assert align >= es and align & (align - 1) == 0 and align <= GUARD
        lo = GUARD + (align % GUARD if self.minimal else 0)
        back = GUARD + (-(lo + nbytes + GUARD)) % GUARD
        total = lo + nbytes + back
        total += (-total) % 8
        # the allocation itself, started at a 256-byte boundary: buf.data_ptr() + lo then has exactly the wanted alignment
        raw = torch.empty(total + GUARD, dtype=torch.uint8, device=self.device)
        base = (-raw.data_ptr()) % GUARD
        buf = raw[base:base + total]
        if kind in ("out", "scratch"):
            buf.copy_(_pattern(dtype, total, self.device, True))
        else:   # (lo, nbytes and total are multiples of the element size)
            buf[:lo].copy_(_pattern(dtype, lo, self.device, False))
            buf[lo + nbytes:].copy_(_pattern(dtype, total - lo - nbytes, self.device, False))
            buf[lo:lo + nbytes].copy_(fill.contiguous().view(-1).view(torch.uint8))
        p = _Placed(kind, buf, lo, nbytes, dtype, shape, written, untouched)
        assert (p.view.data_ptr() % align == 0) and (not self.minimal or align == GUARD or p.view.data_ptr() % (2 * align) != 0)
        self.placed.append(p)
        return p.view

    def inp(self, t, align):
        """A guarded copy of input `t`; poisoned guards."""
        return self._place("in", t.shape, t.dtype, align, t.to(self.device))

    def io(self, t, align):
        """A guarded copy of in-out buffer `t` (updated in place by the call); poisoned guards."""
        return self._place("io", t.shape, t.dtype, align, t.to(self.device))

    def out(self, shape, dtype, align, written=None, untouched=None):
        """A guarded output prefilled with the canary.  written: bool mask (broadcastable to `shape`) of the elements the contract
        says the call writes (None = all); untouched: mask of elements it must NOT write (they keep the canary)."""
        return self._place("out", shape, dtype, align, None, written, untouched)

    def scratch(self, nbytes, align):
        """A guarded scratch buffer (workspace): canary-filled, its guards checked, its contents neither required nor compared."""
        return self._place("scratch", (nbytes,), torch.uint8, align, None)

    def check(self, what=""):
        """(i) guards unchanged bit for bit; (ii) no canary left in the written part of an output, canary kept where nothing is written."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for i, p in enumerate(self.placed):
            tag = f"{what} buffer #{i} ({p.kind}, {p.dtype}, {p.shape}, offset {p.lo})"
            assert torch.equal(p.buf[:p.lo], p.front0), f"{tag}: front guard changed"
            back = p.buf[p.lo + p.nbytes:]
            if not torch.equal(back, p.back0):
                first = int((back != p.back0).nonzero()[0])
                raise AssertionError(f"{tag}: back guard changed (first changed byte {first} past the end)")
            if p.kind == "out":
                can = is_canary(p.view)
                w = torch.ones_like(can) if p.written is None else torch.as_tensor(p.written, device=can.device).expand_as(can)
                left = can & w
                assert not bool(left.any()), f"{tag}: {int(left.sum())} written element(s) still hold the canary"
                if p.untouched is not None:
                    u = torch.as_tensor(p.untouched, device=can.device).expand_as(can)
                    assert bool(can[u].all()), f"{tag}: {int((~can & u).sum())} element(s) written that the contract leaves alone"

    def outputs(self):
        """Bytes of every output / in-out view, for the comparison between placements."""
        return [p.buf[p.lo:p.lo + p.nbytes].clone() for p in self.placed if p.kind in ("out", "io")]


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def assert_same_outputs(a, b, what=""):
    """(iii): the outputs of two placements bit-identical."""
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if not torch.equal(x, y):
            k = int((x != y).nonzero()[0])
            raise AssertionError(f"{what}: output #{i} differs between the 256-byte and the minimum-alignment placement "
                                 f"(first at byte {k})")


def run_both(device, call, what=""):
    """call(g) places its buffers through the Guards g, makes the call and returns whatever the test needs.  Runs at both
    placements, checks the guards after each, compares the outputs bit for bit; returns the 256-byte placement's result."""
    res, outs = [], []
    for minimal in (False, True):
        g = Guards(device, minimal)
        r = call(g)
        g.check(f"{what} ({'minimum alignment' if minimal else '256-byte'} placement)")
        res.append(r)
        outs.append(g.outputs())
    assert_same_outputs(outs[0], outs[1], what)
    return res[0]
