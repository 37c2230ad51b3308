"""CPU self-test of the guarded allocator (tests/guarded_alloc.py): what tests/test_memory_contracts.py relies on when it observes
the HIP ops on the GPU -- poisoned payloads, channels-last views, and a ``verify`` that sees one byte written just outside."""
import pytest
import torch

import guarded_alloc as ga


@pytest.fixture
def alloc():
    return ga.GuardedAllocator()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_payload_is_nan_and_guards_hold(alloc, dtype):
    t = alloc.guarded((3, 5), dtype, "cpu")
    assert t.shape == (3, 5) and t.dtype == dtype and t.is_contiguous()
    assert torch.isnan(t).all()
    assert t.data_ptr() % 512 == alloc.blocks[0][0].data_ptr() % 512            # the payload keeps the block's alignment
    t.zero_()                                                                   # writing the whole payload is fine
    alloc.verify()
    assert alloc.blocks == []                                                   # verify forgets what it checked
    i = alloc.guarded(7, torch.int32, "cpu")
    assert i.shape == (7,) and bool((i == -1).all())
    s = alloc.guarded((), torch.float32, "cpu")
    assert s.shape == () and torch.isnan(s)
    e = alloc.guarded((0,), torch.uint8, "cpu")
    assert e.numel() == 0
    alloc.verify()


def test_channels_last_strides(alloc):
    t = alloc.guarded((2, 8, 3, 5), torch.float32, "cpu", channels_last=True)
    assert t.shape == (2, 8, 3, 5)
    assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
    assert t.stride() == torch.empty(2, 8, 3, 5).contiguous(memory_format=torch.channels_last).stride()
    u = alloc.empty_cl(2, 8, 3, 5, "cpu", torch.bfloat16)
    assert u.dtype == torch.bfloat16 and u.is_contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        alloc.guarded((2, 8), torch.float32, "cpu", channels_last=True)
    alloc.forget()


@pytest.mark.parametrize("side", ["before", "after"])
def test_one_byte_outside_is_reported(alloc, side):
    alloc.guarded((16,), torch.float32, "cpu", label="victim")
    other = alloc.guarded((4,), torch.float32, "cpu", label="bystander")
    raw, n = alloc.blocks[0][0], alloc.blocks[0][1]
    assert n == 64
    raw[ga.G - 1 if side == "before" else ga.G + n] = 0                         # a plain torch index just past the payload
    with pytest.raises(ga.GuardViolation) as e:
        alloc.verify()
    msg = str(e.value)
    assert "victim" in msg and "bystander" not in msg
    assert ("guard %s the payload" % side) in msg
    off = -1 if side == "before" else n
    assert ("first at payload offset %d, last at %d" % (off, off)) in msg
    assert alloc.blocks == []
    other.zero_()
    alloc.verify()                                                              # nothing left to complain about


def test_damage_extent_is_reported(alloc):
    alloc.guarded((8,), torch.uint8, "cpu", label="strip")
    raw = alloc.blocks[0][0]
    raw[ga.G + 8 + 100:ga.G + 8 + 356] = 1
    with pytest.raises(ga.GuardViolation, match=r"256 bytes, first at payload offset 108, last at 363 \(payload 8 bytes\)"):
        alloc.verify()


def test_guarded_input_copies_between_nan_guards(alloc):
    x = torch.arange(24, dtype=torch.float32).view(1, 2, 3, 4)
    t = alloc.guarded_input(x)
    assert torch.equal(t, x) and t.is_contiguous(memory_format=torch.channels_last)
    raw, n, byte, _ = alloc.blocks[0]
    assert byte == ga.POISON_BYTE and n == 96
    around = raw.view(torch.float32)
    assert torch.isnan(around[ga.G // 4 - 1]) and torch.isnan(around[ga.G // 4 + 24])
    v = alloc.guarded_input(torch.ones(5, 3))
    assert v.is_contiguous() and torch.equal(v, torch.ones(5, 3))
    assert alloc.guarded_input(x, channels_last=False).is_contiguous()
    g = alloc.guarded_input(x).requires_grad_(True)                             # a leaf like any other input
    (g * 2).sum().backward()
    assert g.is_leaf and torch.equal(g.grad, torch.full_like(x, 2.0))
    alloc.verify()


def test_workspace_is_exact_and_records_its_caller(alloc):
    import sys

    def caller():
        return alloc.workspace(100, "cpu"), sys._getframe().f_lineno

    ws, line = caller()
    assert ws.dtype == torch.uint8 and ws.numel() == 100
    assert alloc.sites == {("test_guarded_alloc.py", line)}
    alloc.forget()


def test_proxy_guards_empty_and_leaves_the_rest(alloc):
    proxy = ga.TorchProxy(alloc, wants=lambda device: True)
    assert proxy.zeros is torch.zeros
    assert proxy.autograd.Function is torch.autograd.Function
    assert proxy.float32 is torch.float32 and proxy.nn is torch.nn
    a = proxy.empty((2, 3), dtype=torch.float32, device="cpu")
    b = proxy.empty(4, dtype=torch.bfloat16, device=torch.device("cpu"))
    c = proxy.empty((), dtype=torch.float32, device="cpu")
    d = proxy.empty_like(torch.zeros(2, 4, 3, 3).contiguous(memory_format=torch.channels_last))
    e = proxy.empty_like(torch.zeros(3, 2))
    assert len(alloc.blocks) == 5 and alloc.handed == {"torch.empty": 3, "torch.empty_like": 2}
    assert a.shape == (2, 3) and b.shape == (4,) and c.shape == () and e.shape == (3, 2)
    assert d.is_contiguous(memory_format=torch.channels_last)
    assert all(torch.isnan(t).all() for t in (a, b, c, d, e))
    assert len(proxy.empty(3).shape) == 1 and len(alloc.blocks) == 5            # no device named: torch's own
    default = ga.TorchProxy(alloc)
    default.empty((2,), dtype=torch.float32, device="cpu")                      # CPU allocations are left to torch
    default.empty_like(torch.zeros(2))
    assert len(alloc.blocks) == 5
    with pytest.raises(AttributeError):
        proxy.empty = None
    alloc.verify()
