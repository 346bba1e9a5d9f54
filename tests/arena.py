"""Guarded arenas: memory the TEST owns around every device tensor an entry reads or writes (tests/test_gpu_placement.py; the
helper itself is shown to fail on broken stand-ins in tests/test_arena.py, on CPU tensors).

A block is `guard + shift + n + guard` elements of the tensor's own dtype.  The body - what the entry sees - is the `n` elements
behind the first `guard + shift`; everything else is guard and holds one fixed bit pattern, which `check_guards` compares as
integers afterwards.  `shift` = 1 moves a float64 body to 8 mod 16 bytes (a view with an odd storage offset, which every
`is_contiguous()` check of backend.py accepts); `shift` = 0 leaves it on a 16-byte boundary.

    arena.empty   stand-in for `torch.empty` (`monkeypatch.setattr(torch, "empty", arena.empty)`: backend.py resolves the name
                  at call time, so every output and state buffer it allocates is guarded): the WHOLE block, body included,
                  holds the sentinel, so `assert_written` finds an element the entry left alone
    arena.place   an input copied into a block whose guards hold one of two poisons - the sentinel (a NaN for float64) or a
                  finite value (1e300 / -1) - so a read past an input either poisons the result or changes its bits

The sentinels are values no kernel of the library produces: for float64 a quiet NaN with a payload (NaN rows hold the canonical
NaN 0x7FF8000000000000, which compares unequal as an integer), for the integer types a fixed odd pattern (lists hold -1 or an
index, states small counts).

What this does NOT see: a write farther from the body than `guard` elements (the default, 4096 doubles = 32 KiB on either side,
is more than 64 lanes times the longest per-sample record an entry writes, 35 doubles at N = 12), a write that stores the
sentinel itself, and a read past an input whose value does not reach a result."""
import numpy as np
import torch

_REAL_EMPTY = torch.empty                    # (taken before anybody patches the name)

SENTINEL = {torch.float64: 0x7FF8DEADBEEFCAFE, torch.int64: 0x5A5AC3C35A5AC3C3, torch.int32: 0x5A5AC3C3}
_FINITE = {torch.float64: int(np.float64(1e300).view(np.int64)), torch.int64: -1, torch.int32: -1}
_BITS = {torch.float64: torch.int64, torch.int64: torch.int64, torch.int32: torch.int32}      # the integer type of the same width
FILLS = ("sentinel", "finite")


class _Block:
    def __init__(self, name, raw, front, n, fill):
        self.name, self.raw, self.front, self.n, self.fill = name, raw, front, n, fill        # raw: the block as integers


class Arena:
    def __init__(self, guard=4096, shift=0, device=None):
        if shift not in (0, 1):
            raise ValueError("shift: 0 or 1")
        if guard < 2 or guard % 2:
            raise ValueError("guard: an even number of elements (the float64 body's 16-byte phase is `shift` alone)")
        self.guard, self.shift, self.device = int(guard), int(shift), device
        self.blocks = []

    # ---------------------------------------------------------------------------------------------------- allocation
    def _carve(self, shape, dtype, device, fill_bits, origin):
        n = 1
        for s in shape:
            n *= s
        front = self.guard + self.shift
        raw = _REAL_EMPTY(front + n + self.guard, dtype=_BITS[dtype], device=device)
        raw.fill_(fill_bits)
        body = raw.view(dtype)[front:front + n].view(shape)
        if dtype == torch.float64:               # (from the block's pointer: a body without elements has none of its own)
            assert (raw.data_ptr() + 8 * front) % 16 == 8 * self.shift, ("the block does not start on a 16-byte boundary", raw.data_ptr())
            assert n == 0 or body.data_ptr() == raw.data_ptr() + 8 * front
        name = f"#{len(self.blocks)} {origin} {str(dtype).replace('torch.', '')}{list(shape)}"
        self.blocks.append(_Block(name, raw, front, n, fill_bits))
        return body

    def empty(self, *size, **kw):
        """`torch.empty(*size, dtype=, device=)` for float64 / int32 / int64: the body of a block full of the sentinel.  Every
        other call (another dtype, `out=`, `memory_format`, `pin_memory`, ...) goes to the real `torch.empty`."""
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dtype = kw.get("dtype")
        if (set(kw) - {"dtype", "device"} or dtype not in SENTINEL or not size
                or not all(isinstance(s, int) and not isinstance(s, bool) and s >= 0 for s in shape)):
            return _REAL_EMPTY(*size, **kw)
        return self._carve(shape, dtype, kw.get("device"), SENTINEL[dtype], "empty")

    def place(self, x, fill="sentinel"):
        """A copy of `x` (NumPy array or tensor; float64, int32 or int64) on the arena's device - `x`'s own when the arena has
        none - between guards filled with `fill`: "sentinel" or "finite" (1e300 for float64, -1 for the integer types)."""
        if fill not in FILLS:
            raise ValueError(f"fill: one of {FILLS}")
        t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        if t.dtype not in SENTINEL:
            raise ValueError(f"place: float64, int32 or int64, got {t.dtype}")
        device = self.device if self.device is not None else t.device
        bits = SENTINEL[t.dtype] if fill == "sentinel" else _FINITE[t.dtype]
        body = self._carve(tuple(t.shape), t.dtype, device, bits, f"place({fill})")
        body.copy_(t)
        return body

    # ---------------------------------------------------------------------------------------------------- checks
    def _sync(self):
        if any(b.raw.is_cuda for b in self.blocks):
            torch.cuda.synchronize()

    def check_guards(self):
        """Every guard word of every block still holds its fill (compared as integers)."""
        self._sync()
        for b in self.blocks:
            for side, words in (("before", b.raw[:b.front].flip(0)), ("after", b.raw[b.front + b.n:])):   # nearest to the body first
                bad = words != b.fill
                nbad = int(bad.sum())
                if nbad:
                    first = int(torch.nonzero(bad)[0, 0])
                    raise AssertionError(f"guard overwritten: block {b.name}, {side} the body, {nbad} word(s) changed, the nearest "
                                         f"{first + 1} element(s) from the body (now {int(words[first]):#x}, shift {self.shift})")

    def assert_written(self, t, what=""):
        """No element of `t` - a tensor of `arena.empty`, or a view of one - still holds the sentinel."""
        if t.dtype not in SENTINEL:
            raise ValueError(f"assert_written: float64, int32 or int64, got {t.dtype}")
        if t.is_cuda:
            torch.cuda.synchronize()
        left = (t.view(_BITS[t.dtype]) == SENTINEL[t.dtype]).reshape(-1)
        nleft = int(left.sum())
        if nleft:
            first = int(torch.nonzero(left)[0, 0])
            raise AssertionError(f"unwritten: {nleft} of {t.numel()} element(s) of {what or 'the tensor'} "
                                 f"{str(t.dtype).replace('torch.', '')}{list(t.shape)} still hold the sentinel, the first at flat index {first}")
