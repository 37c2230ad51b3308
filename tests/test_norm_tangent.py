"""The tangent of instance norm / MUNIT LayerNorm and its backward (csrc/norm_tangent.hip, hipdwc.normjvp).

Reference: float64 autograd of the restatement ``tangent_ref`` below, on the CPU.
Bounds and where they come from:
  * 1e-5 of each output's largest magnitude: the project's rule for fixed-order fp32 tree sums (tests/test_grad_penalty.py).  The
    kernels' own formulation (pivoted sums, per-group coefficients) in float32 on the CPU stays within 4.8e-6 at these shapes, the
    kernels themselves measured out <= 1.1e-6, dz <= 4.5e-6, dzdot <= 7.8e-7, dgamma <= 2.8e-7 on an MI355X;
  * z = 100 + randn: 1e-4.  z - mean loses log2(100) bits (about 6e-6 relative per factor) and the second-order term of dz multiplies
    three such factors; measured dz <= 2.2e-6 (the pivot keeps the offset out of every sum);
  * two launches on one input are bit-equal (per-chunk partials combined in a fixed order, no atomics).
"""
import pytest
import torch

from hipdwc import _lib, normjvp, ops          # noqa: E402

import guarded_alloc                            # noqa: E402  (tests/ is on the path: conftest)

DEV = "cuda:0"
KINDS = ("in", "ln")
SHAPES = [(3, 8, 5, 7),          # rows not a multiple of anything, a single chunk
          (2, 32, 2, 2),         # instance-norm groups of 4 values
          (2, 16, 16, 16),       # several chunks
          (2, 128, 32, 32),      # the discriminator's real second layer
          (1, 512, 4, 4)]        # batch-1 LayerNorm
EPS = 1e-5


def tangent_ref(z, zd, gamma, kind):
    """out = d/ds norm(z + s zd) at s = 0 without the shift, NCHW, in the dtype of the arguments."""
    dims = (2, 3) if kind == "in" else (1, 2, 3)
    M = z[0, 0].numel() if kind == "in" else z[0].numel()
    c = z - z.mean(dims, keepdim=True)
    cd = zd - zd.mean(dims, keepdim=True)
    if kind == "in":
        r = ((c * c).mean(dims, keepdim=True) + EPS) ** -0.5
        lam = r / M
    else:
        s = ((c * c).sum(dims, keepdim=True) / (M - 1)).sqrt()
        r = 1.0 / (s + EPS)
        lam = 1.0 / ((M - 1) * s)
    xh = r * c
    A = (xh * cd).sum(dims, keepdim=True)
    out = r * cd - lam * A * xh
    return out if gamma is None else out * gamma.reshape(1, -1, 1, 1)


def _case(kind, shape, offset=0.0):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * B + 10 * C + H + (7 if kind == "ln" else 0))
    z = offset + torch.randn(B, C, H, W, generator=gen)
    zd = torch.randn(B, C, H, W, generator=gen)
    dout = torch.randn(B, C, H, W, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.25 if kind == "ln" else None
    return z, zd, dout, gamma


def _reference(kind, z, zd, dout, gamma):
    leaves = [t.double().requires_grad_(True) for t in (z, zd)] + ([gamma.double().requires_grad_(True)] if gamma is not None else [])
    out = tangent_ref(leaves[0], leaves[1], leaves[2] if gamma is not None else None, kind)
    grads = torch.autograd.grad(out, leaves, dout.double())
    return [out.detach()] + list(grads)


def _launch(kind, z, zd, dout, gamma):
    leaves = [ops.cl(t.to(DEV)).requires_grad_(True) for t in (z, zd)] + ([gamma.to(DEV).requires_grad_(True)] if gamma is not None else [])
    out = normjvp.norm_tangent(leaves[0], leaves[1], leaves[2] if gamma is not None else None, kind, EPS)
    grads = torch.autograd.grad(out, leaves, ops.cl(dout.to(DEV)))
    torch.cuda.synchronize()
    return [out.detach()] + list(grads)


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


NAMES = ("out", "dz", "dzdot", "dgamma")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-C%d-%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_norm_tangent_vs_float64_autograd(kind, shape):
    z, zd, dout, gamma = _case(kind, shape)
    want = _reference(kind, z, zd, dout, gamma)
    first = _launch(kind, z, zd, dout, gamma)
    assert len(first) == len(want) == (4 if kind == "ln" else 3)
    for name, got, ref in zip(NAMES, first, want):
        assert torch.isfinite(got).all(), name
        err = rel_err(got, ref)
        print("%s %s %s: rel err %.3e" % (kind, shape, name, err))
        assert err <= 1e-5, (name, err)
    second = _launch(kind, z, zd, dout, gamma)
    for name, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), "%s differs between two launches" % name


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_norm_tangent_large_offset(kind):
    """z = 100 + randn: the statistics are taken about a pivot, so the mean does not eat the variance."""
    shape = (2, 16, 16, 16)
    z, zd, dout, gamma = _case(kind, shape, offset=100.0)
    want = _reference(kind, z, zd, dout, gamma)
    got = _launch(kind, z, zd, dout, gamma)
    for name, g, ref in zip(NAMES, got, want):
        err = rel_err(g, ref)
        print("%s offset 100 %s: rel err %.3e" % (kind, name, err))
        assert err <= 1e-4, (name, err)


def test_norm_tangent_refuses_unsupported_channels_before_any_launch():
    """No device is touched: the pointers are dummies, and every call must return DWC_EINVAL from the host-side checks."""
    lib = _lib.load()
    p = 4096
    for kind in (0, 1):
        for C in (0, 2, 12, 24, 2048):
            assert lib.dwc_norm_tangent_ws_bytes(kind, 2, 16, C) == 0, C
            assert lib.dwc_norm_tangent_fwd(p, p, None, p, p, kind, 2, 16, C, EPS, p, 1 << 30, None) == _lib.EINVAL, C
            assert lib.dwc_norm_tangent_bwd(p, p, p, None, p, p, p, None, kind, 2, 16, C, p, 1 << 30, None) == _lib.EINVAL, C
            assert not normjvp.supported_channels(C)
        assert lib.dwc_norm_tangent_ws_bytes(kind, 2, 16, 8) > 0 and normjvp.supported_channels(8)
        assert lib.dwc_norm_tangent_fwd(p, p, None, p, p, kind, 2, 16, 8, EPS, p, 16, None) == -2      # DWC_EWORKSPACE
    assert lib.dwc_norm_tangent_ws_bytes(2, 2, 16, 8) == 0                                                  # unknown kind
    assert lib.dwc_norm_tangent_fwd(p, p, p, p, p, 0, 2, 16, 8, EPS, p, 1 << 30, None) == _lib.EINVAL      # gamma with kind IN
    assert lib.dwc_norm_tangent_fwd(p, p, None, p, p, 1, 1, 1, 1, EPS, p, 1 << 30, None) == _lib.EINVAL
    assert lib.dwc_norm_tangent_stats_elems(0, 3, 8) == 6 * 24 and lib.dwc_norm_tangent_stats_elems(1, 3, 8) == 6 * 3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 8, 5, 7), (2, 16, 16, 16)], ids=lambda s: "B%d-C%d-%dx%d" % s)
@pytest.mark.parametrize("kind", KINDS)
def test_norm_tangent_under_guarded_buffers(kind, shape, monkeypatch):
    """Every output, the statistics and the scratch between guard zones and poisoned with NaN: no guard byte changes, no NaN comes
    out (so nothing is read that was not written), forward and backward."""
    alloc = guarded_alloc.GuardedAllocator()
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    monkeypatch.setattr(normjvp, "torch", guarded_alloc.TorchProxy(alloc))
    z, zd, dout, gamma = _case(kind, shape)
    zg, zdg, dg = (alloc.guarded_input(t, DEV).requires_grad_(req) for t, req in ((z, True), (zd, True), (dout, False)))
    gg = alloc.guarded_input(gamma, DEV).requires_grad_(True) if gamma is not None else None
    out = normjvp.norm_tangent(zg, zdg, gg, kind, EPS)
    alloc.verify()
    assert alloc.handed.get("workspace") == 1 and alloc.handed.get("empty_cl") == 1 and alloc.handed.get("torch.empty") == 1
    assert torch.isfinite(out).all()
    grads = torch.autograd.grad(out, [zg, zdg] + ([gg] if gg is not None else []), dg)
    alloc.verify()
    assert alloc.handed.get("workspace") == 2 and alloc.handed.get("empty_cl") == 3
    for name, g in zip(NAMES[1:], grads):
        assert torch.isfinite(g).all(), name
    want = _reference(kind, z, zd, dout, gamma)
    for name, g, ref in zip(NAMES, [out] + list(grads), want):
        assert rel_err(g, ref) <= 1e-5, name
