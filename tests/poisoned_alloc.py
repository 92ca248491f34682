"""Hands the package poisoned, guarded memory instead of whatever `torch.empty` would have found (test infrastructure,
not product; imported by test_poisoned_alloc_host.py and test_gpu_uninitialised.py only).

    with poison("ff") as p:
        out = _lib.segclf_forward(batch, weights, F, D, T)
        damaged = p.guards_intact()         # [] when every guard still holds the pattern

While the context is active the name `torch` in each of the package's allocating modules (MODULES) is a proxy.  It
forwards every attribute to the real torch except `empty` and `empty_like`, which for an allocation on one of
`devices` take one uint8 block of GUARD + body + GUARD bytes (body: the byte size rounded up to 8), fill ALL of it
with the pattern and return the body as a contiguous tensor of the requested shape and dtype that starts on a 512-byte
boundary.  The block, its size and the caller's file:line are kept until the context ends.  Allocations on other
devices, and calls with keywords the proxy does not know, go to the real function untouched; `torch.zeros` is never
touched: a wrapper that zero-fills because the ABI says "zero them first" is keeping the contract.

GUARD is a condition, not a measurement: at least 64 KiB on each side (more than any row or record stride of the
library, so an index of -1 or +1 read out of poisoned memory still lands in bytes the test owns) and a multiple of 512.

The patterns are chosen so that no poison value, read as an index of any width, leaves memory the test owns:
  "ff"   every byte 0xFF: float32 / float64 / bfloat16 NaN, int32 / int64 -1.  The guard check that counts
  "one"  the eight bytes of a little-endian int64 1, repeated: int64 1, int32 1, 0, 1, 0 ..., floats denormal or 0.
         Catches counters that start from the buffer's content and outputs whose legitimate value is -1, which "ff"
         cannot see; as a guard it misses an overrun that writes zeros into zero bytes
"""
import importlib
import sys

import torch as _torch

GUARD = 64 * 1024
ALIGN = 512
assert GUARD >= 64 * 1024 and GUARD % ALIGN == 0

PATTERNS = {"ff": bytes([0xFF] * 8), "one": (1).to_bytes(8, "little")}

# every module of gnn_fpga_amd that allocates (test_poisoned_alloc_host.py scans the sources for others)
MODULES = ("_lib", "model", "autograd", "plan_hip", "metrics", "hitgraph", "gcn", "batcher", "shard", "plan_device")

_KNOWN = {"dtype", "device"}


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class _Proxy:
    """`torch` with guarded, pattern-filled `empty` / `empty_like` on `devices`."""

    def __init__(self, owner):
        object.__setattr__(self, "_owner", owner)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def empty(self, *size, **kw):
        owner = self._owner
        if set(kw) - _KNOWN:
            return _torch.empty(*size, **kw)
        device = _torch.device(kw["device"]) if kw.get("device") is not None else _torch.empty(0).device
        if device.type not in owner.devices:
            return _torch.empty(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)) else size
        dtype = kw.get("dtype") or _torch.get_default_dtype()
        return owner._allocate(tuple(int(s) for s in shape), dtype, device, sys._getframe(1))

    def empty_like(self, t, **kw):
        owner = self._owner
        if set(kw) - _KNOWN:
            return _torch.empty_like(t, **kw)
        device = _torch.device(kw["device"]) if kw.get("device") is not None else t.device
        if device.type not in owner.devices or t.layout != _torch.strided:
            return _torch.empty_like(t, **kw)
        return owner._allocate(tuple(t.shape), kw.get("dtype") or t.dtype, device, sys._getframe(1))


class poison:
    """Context manager: see the module's docstring.  `modules`: module objects or names inside gnn_fpga_amd."""

    def __init__(self, pattern, modules=MODULES, devices=("cuda",)):
        self.pattern = pattern
        self.word = int.from_bytes(PATTERNS[pattern], "little", signed=True)
        self.modules = [importlib.import_module("gnn_fpga_amd." + m) if isinstance(m, str) else m for m in modules]
        self.devices = tuple(devices)
        self.records = []                   # (block, nbytes, "file:line")
        self.proxy = _Proxy(self)
        self._saved = None

    def __enter__(self):
        assert self._saved is None, "poison() is not re-entrant"
        self._saved = [(m, m.__dict__["torch"]) for m in self.modules if "torch" in m.__dict__]
        for m, _ in self._saved:
            m.torch = self.proxy
        return self

    def __exit__(self, *exc):
        for m, real in self._saved:
            m.torch = real
        self._saved = None
        self.records = []
        return False

    def _allocate(self, shape, dtype, device, frame):
        nbytes = _numel(shape) * _torch.empty(0, dtype=dtype).element_size()
        body = (nbytes + 7) // 8 * 8
        total = GUARD + body + GUARD
        raw = _torch.empty(total + ALIGN, dtype=_torch.uint8, device=device)
        off = -raw.data_ptr() % ALIGN       # (0 on the GPU: the caching allocator's blocks start on 512 bytes)
        block = raw[off:off + total]
        block.view(_torch.int64).fill_(self.word)
        self.records.append((block, nbytes, "%s:%d" % (frame.f_code.co_filename, frame.f_lineno)))
        return block[GUARD:GUARD + nbytes].view(dtype).reshape(shape)

    def guards_intact(self):
        """The file:line of every allocation whose guard bytes (both bands, and the body's round-up to 8) no longer
        hold the pattern, in allocation order; [] when all are intact.  Synchronises."""
        if _torch.cuda.is_available() and any(b.is_cuda for b, _, _ in self.records):
            _torch.cuda.synchronize()
        flags = []
        for block, nbytes, _ in self.records:
            words = block.view(_torch.int64)
            lo, hi = GUARD // 8, (GUARD + (nbytes + 7) // 8 * 8) // 8
            ok = (words[:lo] == self.word).all() & (words[hi:] == self.word).all()
            if nbytes % 8:                  # the pad bytes between the body's end and its round-up
                want = _torch.tensor(list(PATTERNS[self.pattern][nbytes % 8:]), dtype=_torch.uint8)
                ok = ok & (block[GUARD + nbytes:hi * 8] == want.to(block.device)).all()
            flags.append(ok.reshape(1))
        bad = [] if not flags else (~_torch.cat([f.to(flags[0].device) for f in flags])).nonzero().flatten().tolist()
        return [self.records[i][2] for i in bad]
