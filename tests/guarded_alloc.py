"""Guarded buffers for tests: every allocation sits between two guard zones, starts out poisoned, and is checked afterwards.

A block is one flat uint8 tensor ``[guard G][payload][guard G]``.  The guards hold a known byte, the payload starts as 0xFF bytes
(NaN in fp32 / bf16 / f16, -1 in the integer types), so that
  * a write past either end of what an op asked for changes a guard byte (``verify``),
  * an output element the op never writes stays NaN,
  * a read of never-written scratch yields NaN instead of whatever finite values a recycled block happened to hold.
``guarded_input`` puts a test input between NaN-valued guards: a read past either end shows up as NaN in the result unless the
kernel discards it.

G = 1 MiB covers a 128-row x 512-channel fp32 tile hanging over the end of a buffer and keeps the payload 512-byte aligned, as
torch's own allocations are.  tests/test_memory_contracts.py applies the allocator to hipdwc.ops with monkeypatch; this module
itself runs anywhere (tests/test_guarded_alloc.py exercises it on CPU blocks).
"""
import os
import sys

import torch

G = 1 << 20
GUARD_BYTE = 0x5A
POISON_BYTE = 0xFF


class GuardViolation(AssertionError):
    pass


def _channels_last_strides(shape):
    b, c, h, w = shape
    return (h * w * c, 1, w * c, c)


def _contiguous_strides(shape):
    strides, acc = [], 1
    for n in reversed(shape):
        strides.append(acc)
        acc *= max(int(n), 1)
    return tuple(reversed(strides))


class GuardedAllocator:
    """Hands out guarded tensors and remembers their raw blocks until the next ``verify()``."""

    def __init__(self):
        self.blocks = []          # (raw uint8 block, payload bytes, guard byte, label)
        self.sites = set()        # (file name, line) of the callers of ``workspace``
        self.handed = {}          # first word of a block's label ("workspace", "empty_cl", "torch.empty", "input", ...) -> blocks so far

    # ---- allocation -----------------------------------------------------------------------------------------------------------
    def _block(self, nbytes, device, guard_byte, label):
        raw = torch.empty(2 * G + nbytes, dtype=torch.uint8, device=device)
        raw[:G].fill_(guard_byte)
        raw[G:G + nbytes].fill_(POISON_BYTE)
        raw[G + nbytes:].fill_(guard_byte)
        self.blocks.append((raw, nbytes, guard_byte, label))
        kind = label.split("(")[0].split(" ")[0]
        self.handed[kind] = self.handed.get(kind, 0) + 1
        return raw

    def _view(self, raw, shape, dtype, channels_last):
        """The payload of ``raw`` as a tensor of its own (shares the storage; no autograd view relation to the block)."""
        shape = tuple(int(n) for n in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        strides = _channels_last_strides(shape) if channels_last else _contiguous_strides(shape)
        return torch.empty(0, dtype=dtype, device=raw.device).set_(raw.untyped_storage(), G // item, shape, strides)

    def guarded(self, shape, dtype, device, channels_last=False, label=None):
        """A poisoned (0xFF bytes) tensor of ``shape`` between two guards of ``GUARD_BYTE``."""
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(n) for n in shape)
        if channels_last and len(shape) != 4:
            raise ValueError("channels_last needs a 4-D shape")
        numel = 1
        for n in shape:
            numel *= n
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        raw = self._block(nbytes, device, GUARD_BYTE, label or "guarded %s %s" % (tuple(shape), dtype))
        return self._view(raw, shape, dtype, channels_last)

    def guarded_input(self, t, device=None, channels_last=None, label=None):
        """A copy of the test input ``t`` (on ``device``) whose neighbourhood reads as NaN: guards of 0xFF bytes.  4-D tensors are laid
        out channels-last unless told otherwise (the layout the kernels stream, so that no op makes an unguarded copy first)."""
        t = t.detach()
        device = t.device if device is None else torch.device(device)
        if channels_last is None:
            channels_last = t.dim() == 4
        nbytes = t.numel() * t.element_size()
        raw = self._block(nbytes, device, POISON_BYTE, label or "input %s %s" % (tuple(t.shape), t.dtype))
        out = self._view(raw, t.shape, t.dtype, channels_last)
        out.copy_(t)
        return out

    def empty_cl(self, b, c, h, w, device, dtype=torch.float32):
        """Stand-in for hipdwc.ops.empty_cl."""
        return self.guarded((b, c, h, w), dtype, device, channels_last=True, label="empty_cl %s" % ((b, c, h, w),))

    def workspace(self, nbytes, device):
        """Stand-in for hipdwc.ops.workspace: a FRESH scratch block of exactly ``nbytes`` (so ``ws.numel()`` is what the caller asked
        for), and a record of which call site asked."""
        f = sys._getframe(1)
        site = (os.path.basename(f.f_code.co_filename), f.f_lineno)
        self.sites.add(site)
        return self.guarded((int(nbytes),), torch.uint8, device, label="workspace(%d) at %s:%d" % ((int(nbytes),) + site))

    # ---- checking -------------------------------------------------------------------------------------------------------------
    def forget(self):
        self.blocks = []

    def verify(self):
        """Synchronise, then assert that every guard byte of every block handed out since the last call is intact; forget the
        blocks either way."""
        blocks, self.blocks = self.blocks, []
        if any(raw.is_cuda for raw, _, _, _ in blocks):
            torch.cuda.synchronize()
        if not blocks:
            return
        flags = [((raw[:G] != byte).any() | (raw[G + n:] != byte).any()).cpu() for raw, n, byte, _ in blocks]
        if not torch.stack(flags).any():
            return
        problems = []
        for raw, n, byte, label in blocks:
            for side, zone, base in (("before", raw[:G], -G), ("after", raw[G + n:], n)):
                bad = (zone != byte).nonzero().flatten()
                if bad.numel():
                    # offsets are relative to the payload: negative in front of it, >= its size behind it
                    problems.append("%s: guard %s the payload damaged, %d bytes, first at payload offset %d, last at %d (payload %d bytes)"
                                    % (label, side, bad.numel(), base + int(bad[0]), base + int(bad[-1]), n))
        raise GuardViolation("; ".join(problems))


class TorchProxy:
    """Stands in for the name ``torch`` inside a module: ``empty`` and ``empty_like`` return guarded tensors for the allocations
    ``wants(device)`` selects (by default: everything that is not on the CPU), everything else is the real ``torch``."""

    def __init__(self, alloc, wants=None):
        self.__dict__["_alloc"] = alloc
        self.__dict__["_wants"] = wants or (lambda device: device.type != "cpu")

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def empty(self, *size, dtype=None, device=None, memory_format=None, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dev = torch.device(device) if device is not None else None
        cl = memory_format is torch.channels_last
        if (kw or dev is None or not self._wants(dev) or (cl and len(shape) != 4)
                or memory_format not in (None, torch.contiguous_format, torch.channels_last)):
            if memory_format is not None:
                kw["memory_format"] = memory_format
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._alloc.guarded(shape, dtype or torch.get_default_dtype(), dev, channels_last=cl, label="torch.empty %s" % (shape,))

    def empty_like(self, t, **kw):
        if kw or not self._wants(t.device):
            return torch.empty_like(t, **kw)
        if t.is_contiguous():
            return self._alloc.guarded(t.shape, t.dtype, t.device, label="torch.empty_like %s" % (tuple(t.shape),))
        if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
            return self._alloc.guarded(t.shape, t.dtype, t.device, channels_last=True, label="torch.empty_like %s" % (tuple(t.shape),))
        return torch.empty_like(t)


# one allocator for the test session: the module-level functions are its methods
DEFAULT = GuardedAllocator()
guarded = DEFAULT.guarded
guarded_input = DEFAULT.guarded_input
verify = DEFAULT.verify
