"""TEST INFRASTRUCTURE: guard-band arena for the per-kernel tests (tests/test_guarded_ops_gpu.py, tests/test_arena_cpu.py).

Every other test hands the kernels tight, freshly allocated, 16-byte aligned tensors, so a kernel that stores a row, a vector
or a tile past its output -- or reads past an input and lets the value reach the result -- goes unnoticed: the bytes belong
to the caching allocator and nobody looks at them.  The arena owns one large buffer per element class, filled with a NaN bit
pattern, and hands out views into it:

  * fp32 / bf16 (and any other dtype of up to 4 bytes): the 16-bit pattern 0x7FC0, NaN read as bf16 or as fp32;
  * fp64: the quiet-NaN pattern 0x7FF8000000000000.

A view starts 16-byte aligned (or `misalign_bytes` off that) and has a guard of at least max(1 MiB, 256 rows of that tensor)
on both sides -- the largest row tile in the library is 256 rows.  `assert_untouched()` compares every byte outside the views
with the pattern.  Everything is ordinary owned memory: an overrun lands in a guard, not in an unmapped page, so nothing here
can fault a device and nothing is meant to.

`outputs_in(arena)` makes the result tensors mimic_amd.ops allocates (torch.empty / empty_like / zeros on the arena's device)
come out of the arena, by substituting the `torch` name the ops module sees with a forwarding proxy for the duration of the
block.  It is not a conftest and changes no default of ops.py."""
from __future__ import annotations

import contextlib
import math

import torch

POISON16 = 0x7FC0
POISON64 = 0x7FF8000000000000
_WORD = {"h": int.from_bytes(bytes([0xC0, 0x7F] * 4), "little", signed=True), "d": POISON64}
_BYTES = {"h": bytes([0xC0, 0x7F] * 4), "d": POISON64.to_bytes(8, "little")}
MIN_GUARD = 1 << 20
GUARD_ROWS = 256


class ArenaError(AssertionError):
    pass


class _View:
    def __init__(self, cls, start, nbytes, tensor, name):
        self.cls, self.start, self.end, self.tensor, self.name = cls, start, start + nbytes, tensor, name

    def describe(self):
        return f"view '{self.name}' {tuple(self.tensor.shape)} {str(self.tensor.dtype).replace('torch.', '')}"


class Arena:
    def __init__(self, device, capacity=512 << 20, capacity64=48 << 20):
        self.device = torch.device(device)
        self.raw = {"h": torch.empty(capacity, dtype=torch.uint8, device=self.device),
                    "d": torch.empty(capacity64, dtype=torch.uint8, device=self.device)}
        for cls, raw in self.raw.items():
            assert raw.data_ptr() % 16 == 0 and raw.numel() % 8 == 0
            raw.view(torch.int64).fill_(_WORD[cls])
        self.views = []
        self._cursor = {"h": 0, "d": 0}       # end of the last view of the class
        self._last_guard = {"h": 0, "d": 0}
        self._dirty = {"h": 0, "d": 0}        # bytes from 0 that reset() has to poison again

    # ---- placement -------------------------------------------------------------------------------------------------
    @staticmethod
    def _cls(dtype):
        return "d" if dtype in (torch.float64, torch.int64) else "h"

    @staticmethod
    def guard_bytes(shape, dtype):
        row = (shape[-1] if len(shape) else 1) * torch.empty((), dtype=dtype).element_size()
        return max(MIN_GUARD, GUARD_ROWS * row)

    def _carve(self, shape, dtype, misalign_bytes, name):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        assert misalign_bytes % item == 0 and 0 <= misalign_bytes < 16, "misalign_bytes: a multiple of the element size below 16"
        cls = self._cls(dtype)
        nbytes = math.prod(shape) * item
        guard = self.guard_bytes(shape, dtype)
        start = self._cursor[cls] + max(guard, self._last_guard[cls])
        start = -(-start // 16) * 16 + misalign_bytes
        raw = self.raw[cls]
        if start + nbytes + guard > raw.numel():
            raise ArenaError(f"arena full: {name} {shape} {dtype} needs {nbytes} bytes + {guard} of guard after offset {start}")
        t = raw[start:start + nbytes].view(dtype).view(shape)
        assert t.data_ptr() % 16 == misalign_bytes and t.is_contiguous()
        self.views.append(_View(cls, start, nbytes, t, name or f"#{len(self.views)}"))
        self._cursor[cls], self._last_guard[cls] = start + nbytes, guard
        self._dirty[cls] = max(self._dirty[cls], start + nbytes + guard)
        return t

    def place(self, t, misalign_bytes=0, name=None):
        """a contiguous view with t's shape, dtype and contents (t may live on any device)"""
        v = self._carve(t.shape, t.dtype, misalign_bytes, name)
        v.copy_(t)
        return v

    def new_output(self, shape, dtype, misalign_bytes=0, name=None, zero=False):
        """the same kind of view with poison as its contents (zero=True: zero-filled, for accumulators)"""
        v = self._carve(shape, dtype, misalign_bytes, name)
        if zero:
            v.zero_()
        return v

    def owns(self, t):
        return any(v.tensor.data_ptr() <= t.data_ptr() < v.tensor.data_ptr() + max(v.end - v.start, 1) for v in self.views)

    def reset(self):
        """forget every view and poison what they covered"""
        for cls, raw in self.raw.items():
            n = min(-(-self._dirty[cls] // 8) * 8, raw.numel())
            if n:
                raw[:n].view(torch.int64).fill_(_WORD[cls])
        self.views = []
        self._cursor = {"h": 0, "d": 0}
        self._last_guard = {"h": 0, "d": 0}
        self._dirty = {"h": 0, "d": 0}

    # ---- the check -------------------------------------------------------------------------------------------------
    def _first_bad(self, cls, a, b):
        """offset of the first byte in [a, b) that differs from the pattern, or None"""
        raw = self.raw[cls]
        a8, b8 = min(-(-a // 8) * 8, b), max(b // 8 * 8, a)
        pieces = []
        if a8 < b8:
            pieces = [(a, a8), (a8, b8), (b8, b)]
        else:
            pieces = [(a, b)]
        for lo, hi in pieces:
            if lo >= hi:
                continue
            if lo % 8 == 0 and hi % 8 == 0:
                words = raw[lo:hi].view(torch.int64)
                if bool((words == _WORD[cls]).all()):
                    continue
                w = int((words != _WORD[cls]).nonzero()[0])
                lo, hi = lo + 8 * w, lo + 8 * w + 8
            want = torch.tensor([_BYTES[cls][o % 8] for o in range(lo, hi)], dtype=torch.uint8)
            got = raw[lo:hi].cpu()
            if not torch.equal(got, want):
                return lo + int((got != want).nonzero()[0])
        return None

    def assert_untouched(self):
        """every byte outside the placed views still holds the pattern; names the first tampered offset relative to the
        nearest view"""
        for cls, raw in self.raw.items():
            edges, pos = [], 0
            for v in sorted((v for v in self.views if v.cls == cls), key=lambda v: v.start):
                edges.append((pos, v.start))
                pos = v.end
            edges.append((pos, raw.numel()))
            for a, b in edges:
                bad = self._first_bad(cls, a, b)
                if bad is None:
                    continue
                got = int(raw[bad])
                self._dirty[cls] = raw.numel()          # (the next reset() poisons the whole buffer again)
                near = [v for v in self.views if v.cls == cls]
                if not near:
                    raise ArenaError(f"arena ({'fp64' if cls == 'd' else 'fp32/bf16'} class) tampered at byte {bad} (value 0x{got:02x}); no view placed")
                v = min(near, key=lambda v: min(abs(bad - v.start), abs(bad - (v.end - 1))))
                where = (f"{v.start - bad} bytes before the start of" if bad < v.start else f"{bad - v.end} bytes past the end of")
                raise ArenaError(f"guard tampered: byte 0x{got:02x} found {where} {v.describe()} "
                                 f"({'fp64' if cls == 'd' else 'fp32/bf16'} class, arena offset {bad})")

    def is_poison(self, t):
        """does this arena view still hold nothing but the pattern? (an output no launch has written)"""
        v = next(v for v in self.views if v.tensor.data_ptr() == t.data_ptr())
        return self._first_bad(v.cls, v.start, v.end) is None


# ---- outputs of mimic_amd.ops out of the arena -------------------------------------------------------------------------
def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        return tuple(size[0])
    return tuple(int(s) for s in size)


class _TorchProxy:
    """stands in for the `torch` name inside mimic_amd.ops: empty / empty_like / zeros on the arena's device come out of the
    arena (zero-filled requests stay zero-filled), everything else is forwarded"""

    def __init__(self, arena, real):
        self._arena, self._real, self.allocated, self.zero_filled = arena, real, [], set()

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _mine(self, device):
        return device is not None and torch.device(device).type == self._arena.device.type

    def _new(self, shape, dtype, zero):
        t = self._arena.new_output(shape, dtype or torch.float32, name=f"ops output {len(self.allocated)}", zero=zero)
        self.allocated.append(t)
        if zero:
            self.zero_filled.add(t.data_ptr())
        return t

    def _no_extras(self, what, kw):
        # (an allocation the proxy cannot restate would leave the arena without notice: refused while the proxy is active)
        if kw:
            raise ArenaError(f"ops.torch.{what} with {sorted(kw)}: the arena proxy only understands a size / a tensor, dtype and device")

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return self._real.empty(*size, dtype=dtype, device=device, **kw)
        self._no_extras("empty", kw)
        return self._new(_shape_of(size), dtype, False)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return self._real.zeros(*size, dtype=dtype, device=device, **kw)
        self._no_extras("zeros", kw)
        return self._new(_shape_of(size), dtype, True)

    def empty_like(self, t, **kw):
        if not self._mine(t.device):
            return self._real.empty_like(t, **kw)
        self._no_extras("empty_like", kw)
        return self._new(t.shape, t.dtype, False)


class _LibLog:
    """forwards to the ctypes library and records which entry points were asked for"""

    def __init__(self, real, called):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_called", called)

    def __getattr__(self, name):
        if name.startswith("mopoe_"):
            self._called.add(name)
        return getattr(self._real, name)


CALLED_UNDER_ARENA = set()


@contextlib.contextmanager
def outputs_in(arena, ops=None):
    """inside the block the tensors mimic_amd.ops allocates for its results are arena views.  Yields the proxy: its
    `.allocated` lists them (`.zero_filled`: the data pointers of those requested as zeros).  The caller touches ops._workspace(device) and the latent workspaces before entering, so that they
    are not captured.  ops.torch (and the library handle, wrapped to record the entry points used) are restored on exit,
    also after an exception."""
    if ops is None:
        from mimic_amd import ops
    real_torch, real_lib = ops.torch, ops._lib
    proxy = _TorchProxy(arena, real_torch)
    ops.torch = proxy
    if real_lib is not None:
        ops._lib = _LibLog(real_lib, CALLED_UNDER_ARENA)
    try:
        yield proxy
    finally:
        ops.torch = real_torch
        if real_lib is not None:
            ops._lib = real_lib
