"""Where the HIP ops write and what they read: every op of hipdwc.ops / spectral / penalty run with guarded buffers.

The parity tests check what the kernels compute.  Here the same ops run under tests/guarded_alloc.py:
  * ``ops.workspace`` hands out a FRESH scratch block of exactly the size the call site asked for (in production the arena is at
    least 1 MiB and only grows, so at test shapes a kernel that writes past what it declared lands inside the arena), poisoned
    with NaN, between two guard zones;
  * every ``empty_cl`` / ``torch.empty`` / ``torch.empty_like`` output of the three modules is such a block too (torch recycles
    blocks: an element a kernel never writes would otherwise still hold the right answer of the previous run);
  * test inputs sit between NaN-valued guards (a read past either end times a zero weight is NaN, not 0).
Each case: forward, guards verified, values against the reference and tolerance of the op's own parity test, backward, guards
verified, every gradient -- and a NaN anywhere fails by name.  The shapes are the smallest that reach each launch form (the tables
of the parity tests).  The last test asserts that every ``workspace(`` call site of the three modules was exercised.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as ga
from test_bf16_parity import CONV_SHAPES as BF16_CONV_SHAPES
from test_hip_parity import CONV_SHAPES as FP32_CONV_SHAPES, close
from test_spectral_norm import SN_CASES, _block as _sn_block

pytestmark = pytest.mark.gpu

from hipdwc import _lib, ops, penalty, spectral          # noqa: E402
from oracle import dwcgan_oracle as orc                    # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16

# ---- the call sites the recorder must see -------------------------------------------------------------------------------------------
_PKG = os.path.dirname(os.path.abspath(ops.__file__))


def _scan_sites():
    sites = {}
    for name in ("ops.py", "spectral.py", "penalty.py"):
        with open(os.path.join(_PKG, name)) as f:
            for no, line in enumerate(f, 1):
                if re.search(r"\bworkspace\(", line) and not line.lstrip().startswith("def "):
                    sites[(name, no)] = line.strip()
    return sites


SITES = _scan_sites()
# (file, text that identifies ONE call site): reason.  At most two lines.
EXEMPT = {
}
SEEN = set()
EXPECTED, RAN = set(), set()


def cases(argname, values, ids):
    """pytest.mark.parametrize that also registers the case names: the coverage test at the end only judges a run of all of them."""
    values = list(values)
    names = [ids(v) if callable(ids) else ids[i] for i, v in enumerate(values)]
    assert len(set(names)) == len(names), names

    def deco(fn):
        EXPECTED.update("%s[%s]" % (fn.__name__, n) for n in names)
        return pytest.mark.parametrize(argname, values, ids=names)(fn)
    return deco


def single(fn):
    EXPECTED.add(fn.__name__)
    return fn


@pytest.fixture
def guards(monkeypatch, request):
    """The guarded allocator applied to hipdwc: scratch, channels-last outputs and every torch.empty / empty_like of the three modules."""
    alloc = ga.DEFAULT
    alloc.forget()
    proxy = ga.TorchProxy(alloc)
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    for mod in (ops, spectral, penalty):
        monkeypatch.setattr(mod, "torch", proxy)
    ops.set_precision("fp32")
    yield alloc
    ops.set_precision("fp32")
    SEEN.update(alloc.sites)
    alloc.forget()
    RAN.add(request.node.name)


def gi(t, channels_last=None):
    return ga.guarded_input(t, device=DEV, channels_last=channels_last)


def rb(t):
    return t.to(BF).float()


def check(name, got, want, rel, atol=1e-6):
    got = got.detach().float().cpu()
    nan = int(torch.isnan(got).sum())
    assert nan == 0, "%s holds NaN in %d of %d elements (never written, or computed from memory nobody wrote)" % (name, nan, got.numel())
    close(got, want, rel=rel, atol=atol, msg=name)


def ids_x(s):
    return "x".join(str(v) for v in s)


# ---- convolutions -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_ref(shape, half):
    """(x, w, b, gy, y, dx, dw, db) of act(conv(reflect_pad(x))) on the CPU oracle, as tests/test_hip_parity.py (fp32) and
    tests/test_bf16_parity.py (operands rounded to bf16) build them.  Computed once per shape, never modified."""
    B, ci, co, H, W, k, s, p, act = shape
    g = torch.Generator().manual_seed(sum(v for v in shape if isinstance(v, int)) + (11 if half else 0))
    rnd = rb if half else (lambda t: t)
    x = rnd(torch.randn(B, ci, H, W, generator=g))
    w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (ci * k * k) ** 0.5)
    b = torch.randn(co, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    wv = rb(wr.detach()) + (wr - wr.detach()) if half else wr                 # value of rb(w), gradient w.r.t. w
    if act == "heads":
        pre = orc.conv_block(xr, wv, br, s, p)
        yr = torch.cat([torch.tanh(pre[:, :3]), torch.sigmoid(pre[:, 3:4])], 1)
    else:
        yr = orc.conv_block(xr, wv, br, s, p, act=act)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    return x, w, b, gy, yr.detach(), xr.grad, wr.grad, br.grad


def _conv_tols(half, act):
    if not half:
        return 2e-5, 5e-5, 5e-5                     # tests/test_hip_parity.py test_conv_forward_backward
    plain = act == "none"                           # tests/test_bf16_parity.py test_bf16_conv_forward_backward
    return 6e-3, (6e-3 if plain else 1.5e-2), (3e-4 if plain else 1e-2)


def _run_conv(guards, shape, half, backward=True):
    B, ci, co, H, W, k, s, p, act = shape
    x, w, b, gy, yr, dxr, dwr, dbr = _conv_ref(shape, half)
    ops.set_precision("bf16" if half else "fp32")
    if half and ci == 3:                            # an image: packed to NHWC8 by the op under test
        x0 = gi(x, channels_last=False).requires_grad_(True)
        xd = ops.pack_image(x0)
        assert xd.dtype == BF and xd.shape[1] == 8
    else:
        x0 = xd = gi(x.to(BF) if half else x).requires_grad_(True)
    wd, bd = gi(w, channels_last=False).requires_grad_(True), gi(b).requires_grad_(True)
    yd = ops.conv2d(xd, wd, bd, s, p, act)
    guards.verify()
    ty, tdx, tdw = _conv_tols(half, act)
    assert yd.shape == yr.shape and yd.dtype == (BF if half else torch.float32)
    check("y", yd, yr, ty)
    if not backward:
        return
    yd.backward(gi(gy.to(yd.dtype)))
    guards.verify()
    check("dx", x0.grad, dxr, tdx)
    check("dw", wd.grad, dwr, tdw)
    check("db", bd.grad, dbr, tdw)


H2_MASKED_ROWS = (2, 32, 96, 32, 16, 3, 1, 1, "none")


def _norm_shape(s):
    B, ci, co, H, k, st, p, act = s
    return (B, ci, co, H, H, k, st, p, act)


CONV_CASES = [("fp32", _norm_shape(s)) for s in FP32_CONV_SHAPES] + [("bf16", _norm_shape(s)) for s in BF16_CONV_SHAPES] + [
    # tests/test_h2_parity.py: Cout 96 masks rows of the last tile.  (Forward only, as there: ops.conv2d has no backward for 96 output
    # channels -- the data gradient gathers dY (power-of-two channel counts only) and the bias-gradient pass takes channel counts C
    # with C / 4 dividing 256 or a multiple of it; both refuse 96 with DWC_EINVAL.)
    ("fp32", H2_MASKED_ROWS),
    ("fp32", (4, 128, 256, 32, 32, 3, 1, 1, "none")),        # test_h2_contraction_split_of_small_launches: 64 tiles, split whole
    ("fp32", (2, 64, 128, 32, 32, 3, 1, 1, "relu")),         # fp32 data gradient with the border ring inside the halo launch
]


@cases("case", CONV_CASES, ids=lambda c: c[0] + "-" + ids_x(c[1]))
def test_conv_memory_contract(guards, case):
    _run_conv(guards, case[1], case[0] == "bf16", backward=case[1] != H2_MASKED_ROWS)


# (name, precision, shape, {ops switch: value}); S2DGRAD_MIN_WGS = 0 lets a 2-image batch take the stride-2 halo data gradient
S1 = (2, 64, 128, 32, 32, 3, 1, 1, "relu")
S2 = (2, 64, 128, 32, 32, 4, 2, 1, "relu")
SWITCH_CASES = [
    ("DGRAD_FOLD=0", "fp32", (1, 16, 32, 6, 6, 4, 2, 1, "tanh"), {"DGRAD_FOLD": 0}),
    ("DGRAD_FOLD=0", "bf16", (1, 16, 32, 6, 6, 4, 2, 1, "tanh"), {"DGRAD_FOLD": 0}),
    ("X3_S2=0", "fp32", S2, {"X3_S2": 0}),
    ("S2HALO=0", "bf16", S2, {"S2HALO": 0}),
    ("s2-halo-dgrad", "fp32", S2, {"S2DGRAD_MIN_WGS": 0}),
    ("s2-halo-dgrad", "bf16", S2, {"S2DGRAD_MIN_WGS": 0}),
    ("S2DGRAD=0", "fp32", S2, {"S2DGRAD_MIN_WGS": 0, "S2DGRAD": 0}),
    ("S2DGRAD=0", "bf16", S2, {"S2DGRAD_MIN_WGS": 0, "S2DGRAD": 0}),
    ("RING_FUSED=0-s1", "fp32", S1, {"RING_FUSED": 0}),
    ("RING_FUSED=0-s1", "bf16", S1, {"RING_FUSED": 0}),
    ("RING_FUSED=0-s2", "fp32", S2, {"S2DGRAD_MIN_WGS": 0, "RING_FUSED": 0}),
    ("RING_FUSED=0-s2", "bf16", S2, {"S2DGRAD_MIN_WGS": 0, "RING_FUSED": 0}),
    ("X3_PLANES=3-k3", "fp32", (2, 256, 256, 16, 16, 3, 1, 1, "none"), {"X3_PLANES": 3}),
    ("X3_PLANES=3-k5", "fp32", (1, 256, 128, 16, 16, 5, 1, 2, "none"), {"X3_PLANES": 3}),
    ("X3_PLANES=3-ring", "fp32", S1, {"X3_PLANES": 3}),
]


@cases("case", SWITCH_CASES, ids=lambda c: c[0] + "-" + c[1])
def test_conv_alternative_paths_memory_contract(guards, monkeypatch, case):
    _, prec, shape, switches = case
    for k, v in switches.items():
        assert hasattr(ops, k)
        monkeypatch.setattr(ops, k, v)
    _run_conv(guards, shape, prec == "bf16")


@cases("fuse", [1, 0], ids=lambda v: "RES_FUSE=%d" % v)
def test_residual_gradient_memory_contract(guards, monkeypatch, fuse):
    """x + IN(conv(x)): the identity-branch gradient in the data gradient's epilogue (ResGradToken) and, with DWC_RES_FUSE=0, summed by
    autograd.  Tolerances of a convolution + norm block (tests/test_hip_parity.py test_golden_conv_blocks)."""
    monkeypatch.setattr(ops, "RES_FUSE", fuse)
    B, C, H = 2, 64, 16
    g = torch.Generator().manual_seed(31)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (1.0 / (C * 9) ** 0.5)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = orc.instance_norm(orc.conv_block(xr, wr, None, 1, 1)) + xr
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, wd = gi(x).requires_grad_(True), gi(w, channels_last=False).requires_grad_(True)
    tok = ops.res_token(xd)
    assert (tok is not None) == bool(fuse)
    yd = ops.instance_norm(ops.conv2d(xd, wd, None, 1, 1, "none", token=tok), residual=xd, token=tok)
    guards.verify()
    check("y", yd, yr.detach(), 5e-5, 2e-6)
    yd.backward(gi(gy))
    guards.verify()
    check("dx", xd.grad, xr.grad, 3e-4, 2e-6)
    check("dw", wd.grad, wr.grad, 3e-4, 2e-6)


@cases("case", [(prec, s) for prec in ("fp32", "bf16") for s in [(2, 64, 32, 32), (1, 16, 9, 24)]], ids=lambda c: c[0] + "-" + ids_x(c[1]))
def test_heads_memory_contract(guards, case):
    """ops.conv2d_heads: test_fused_image_heads / test_bf16_fused_image_heads."""
    prec, (B, C, H, W) = case
    half = prec == "bf16"
    x, w, b, gy, yr, dxr, dwr, dbr = _conv_ref((B, C, 4, H, W, 7, 1, 3, "heads"), half)
    ops.set_precision(prec)
    xd = gi(x.to(BF) if half else x).requires_grad_(True)
    wd, bd = gi(w, channels_last=False).requires_grad_(True), gi(b).requires_grad_(True)
    if half:
        w8, b8 = torch.cat([wd, wd.new_zeros(4, C, 7, 7)], 0), torch.cat([bd, bd.new_zeros(4)], 0)
        yd = ops.conv2d_heads(xd, w8, b8)
        guards.verify()
        assert yd.shape == (B, 8, H, W) and yd.dtype == BF
        assert float(yd.detach()[:, 4:].abs().max()) == 0.0
        check("y", yd[:, :4], yr, 6e-3)
        yd.backward(gi(torch.cat([gy, torch.zeros(B, 4, H, W)], 1).to(BF)))
        tdx, tdw = 1.5e-2, 1e-2
    else:
        yd = ops.conv2d_heads(xd, wd, bd)
        guards.verify()
        check("y", yd, yr, 2e-5)
        yd.backward(gi(gy))
        tdx, tdw = 5e-5, 5e-5
    guards.verify()
    check("dx", xd.grad, dxr, tdx)
    check("dw", wd.grad, dwr, tdw)
    check("db", bd.grad, dbr, tdw)


# (precision, B, Cin, Cout, H): (1, 8, 16, 6) is the table's shape; 32 -> 32 channels makes both GEMMs long enough for split-K partials
@cases("case", [("fp32", 1, 8, 16, 6), ("bf16", 1, 8, 16, 6), ("fp32", 1, 32, 32, 6)], ids=ids_x)
def test_zeropad_conv_and_max_pool_memory_contract(guards, case):
    """ops.conv2d_zeropad + ops.max_pool2: test_max_pool2_and_zeropad_conv (bf16: the tolerances of a bf16 convolution behind an
    activation)."""
    prec, B, C, co, H = case
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B + C + H + co)
    x = rnd(torch.randn(B, C, H, H, generator=g))
    x[:, :, :2, :2] = 0.0                                  # a tied (all-zero) window: gradient goes to its first element
    w, b = rnd(torch.randn(co, C, 3, 3, generator=g) * 0.2), torch.randn(co, generator=g) * 0.1
    xr = x.clone().requires_grad_(True)
    yr = F.max_pool2d(torch.relu(F.conv2d(xr, w, b, padding=1)), 2, 2)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    xd = gi(x.to(BF) if half else x).requires_grad_(True)
    yd = ops.max_pool2(ops.conv2d_zeropad(xd, gi(w, channels_last=False), gi(b), 1, "relu"))
    guards.verify()
    check("y", yd, yr.detach(), 6e-3 if half else 2e-5)
    yd.backward(gi(gy.to(yd.dtype)))
    guards.verify()
    check("dx", xd.grad, xr.grad, 1.5e-2 if half else 5e-5)


# ---- norms --------------------------------------------------------------------------------------------------------------------------
@cases("case", [(prec, mode, s) for prec in ("fp32", "bf16") for mode in ("in", "in_relu", "adain_relu", "adain_res")
                for s in [(2, 512, 2), (2, 8, 6), (3, 64, 32)]], ids=lambda c: "%s-%s-%s" % (c[0], c[1], ids_x(c[2])))
def test_instance_norm_memory_contract(guards, case):
    """test_instance_norm / test_bf16_instance_norm."""
    prec, mode, (B, C, H) = case
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 2 + 0.7)
    res = rnd(torch.randn(B, C, H, H, generator=g)) if mode.endswith("res") else None
    ga_ = (torch.randn(B * C, generator=g) * 0.5 + 1) if mode.startswith("adain") else None
    be = torch.randn(B * C, generator=g) if mode.startswith("adain") else None
    relu = mode.endswith("relu")
    # A pre-activation value of exactly 0 (four bf16 values of a 2 x 2 plane whose mean IS one of them) leaves ReLU's derivative to
    # the implementation's rounding of the mean: such planes are drawn again.  1e-4 is far above the fp32 rounding of a normalised
    # value (a few 1e-7 here) and far below anything a wrong kernel would be excused by: 0.01 % of a unit-variance plane.
    for _ in range(16):
        pre = orc.adain(x, ga_, be) if ga_ is not None else orc.instance_norm(x)
        tied = (pre.abs() < 1e-4).flatten(2).any(2) if relu else torch.zeros(B, C, dtype=torch.bool)
        if not tied.any():
            break
        x[tied] = rnd(torch.randn(int(tied.sum()), H, H, generator=g) * 2 + 0.7)
    assert not tied.any()
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if res is not None else None
    gr, br = (ga_.clone().requires_grad_(True), be.clone().requires_grad_(True)) if ga_ is not None else (None, None)
    yr = orc.adain(xr, gr, br) if ga_ is not None else orc.instance_norm(xr)
    if relu:
        yr = torch.clamp_min(yr, 0)
    if rr is not None:
        yr = yr + rr
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    xd = gi(cast(x)).requires_grad_(True)
    rd = gi(cast(res)).requires_grad_(True) if res is not None else None
    gd, bd = (gi(ga_).requires_grad_(True), gi(be).requires_grad_(True)) if ga_ is not None else (None, None)
    yd = ops.instance_norm(xd, gd, bd, residual=rd, relu=relu)
    guards.verify()
    ty, tdx, tp, tres = (6e-3, 8e-3, 2e-3, 1e-6) if half else (3e-5, 2e-4, 1e-4, 2e-5)
    check("y", yd, yr.detach(), ty)
    yd.backward(gi(cast(gy)))
    guards.verify()
    check("dx", xd.grad, xr.grad, tdx)
    if rd is not None:
        check("dres", rd.grad, rr.grad, tres)
    if gd is not None:
        check("dgamma", gd.grad, gr.grad, tp)
        check("dbeta", bd.grad, br.grad, tp)


@cases("case", [(prec, relu, s) for prec in ("fp32", "bf16") for relu in (False, True) for s in [(2, 8, 10), (3, 128, 16)]],
       ids=lambda c: "%s-%s-%s" % (c[0], "relu" if c[1] else "none", ids_x(c[2])))
def test_layer_norm_memory_contract(guards, case):
    """test_layer_norm / test_bf16_layer_norm."""
    prec, relu, (B, C, H) = case
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B + C + H)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 1.5 - 0.3)
    ga_, be = torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.1
    xr, gr, br = [t.clone().requires_grad_(True) for t in (x, ga_, be)]
    yr = orc.layer_norm_munit(xr, gr, br)
    if relu:
        yr = torch.clamp_min(yr, 0)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    xd, gd, bd = gi(cast(x)).requires_grad_(True), gi(ga_).requires_grad_(True), gi(be).requires_grad_(True)
    yd = ops.layer_norm_munit(xd, gd, bd, relu=relu)
    guards.verify()
    ty, tdx, tp = (6e-3, 8e-3, 2e-3) if half else (3e-5, 2e-4, 1e-4)
    check("y", yd, yr.detach(), ty)
    yd.backward(gi(cast(gy)))
    guards.verify()
    check("dx", xd.grad, xr.grad, tdx)
    check("dgamma", gd.grad, gr.grad, tp)
    check("dbeta", bd.grad, br.grad, tp)


# ---- pointwise ----------------------------------------------------------------------------------------------------------------------
# (precision, up?, shape); the bf16 forms take channel counts that are multiples of 8
@cases("case", [("fp32", True, (2, 8, 1, 3)), ("fp32", True, (1, 8, 19, 7)), ("fp32", False, (2, 4, 8, 12)),
                ("bf16", True, (2, 8, 1, 3)), ("bf16", True, (1, 8, 19, 7)), ("bf16", False, (2, 8, 8, 12))],
       ids=lambda c: "%s-%s-%s" % (c[0], "up" if c[1] else "down", ids_x(c[2])))
def test_resample_memory_contract(guards, case):
    """test_resample_and_golden (1e-6) / test_bf16_resample_blend_l1_pack (6e-3: a stored bf16 tensor)."""
    prec, up, shape = case
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(sum(shape))
    x = rnd(torch.randn(shape, generator=g))
    xr = x.clone().requires_grad_(True)
    yr = orc.upsample_bilinear2x(xr) if up else orc.downsample_half(xr)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    xd = gi(x.to(BF) if half else x).requires_grad_(True)
    yd = ops.upsample2x(xd) if up else ops.downsample_half(xd)
    guards.verify()
    tol = 6e-3 if half else 1e-6
    check("y", yd, yr.detach(), tol)
    yd.backward(gi(gy.to(yd.dtype)))
    guards.verify()
    check("dx", xd.grad, xr.grad, tol)


@cases("prec", ["fp32", "bf16"], ids=str)
def test_pack_and_blend_memory_contract(guards, prec):
    """pack_image and attention_blend at 8 x 8: test_pack_blend_l1 / test_bf16_resample_blend_l1_pack."""
    half = prec == "bf16"
    planes = 8 if half else 4
    ops.set_precision(prec)
    g = torch.Generator().manual_seed(11)
    x3 = torch.randn(2, 3, 8, 8, generator=g)
    xd = gi(x3, channels_last=False).requires_grad_(True)
    x4 = ops.pack_image(xd)
    guards.verify()
    assert x4.shape == (2, planes, 8, 8) and x4.is_contiguous(memory_format=torch.channels_last)
    check("packed planes 0..2", x4[:, :3], rb(x3) if half else x3, 0.0, 0.0)
    check("packed padding planes", x4[:, 3:], torch.zeros(2, planes - 3, 8, 8), 0.0, 0.0)
    gy = rb(torch.randn(2, planes, 8, 8, generator=g))
    x4.backward(gi(gy.to(x4.dtype)))
    guards.verify()
    check("d image", xd.grad, gy[:, :3], 0.0, 0.0)
    # blend
    heads = torch.cat([torch.tanh(torch.randn(2, 3, 8, 8, generator=g)), torch.sigmoid(torch.randn(2, 1, 8, 8, generator=g))], 1)
    heads = rb(heads) if half else heads
    real3 = rb(x3) if half else x3
    hr = heads.clone().requires_grad_(True)
    outr = hr[:, :3] * hr[:, 3:4] + real3 * (1 - hr[:, 3:4])
    go = rb(torch.randn(outr.shape, generator=g))
    (outr * go).sum().backward()
    pad = torch.zeros(2, planes - 4, 8, 8)
    hd = gi(torch.cat([heads, pad], 1).to(x4.dtype)).requires_grad_(True)
    outd = ops.attention_blend(hd, x4.detach())
    guards.verify()
    check("blend", outd[:, :3], outr.detach(), 6e-3 if half else 1e-6)
    check("blend padding planes", outd[:, 3:], torch.zeros(2, planes - 3, 8, 8), 0.0, 0.0)
    outd.backward(gi(torch.cat([go, torch.zeros(2, planes - 3, 8, 8)], 1).to(outd.dtype)))
    guards.verify()
    check("d heads", hd.grad[:, :4], hr.grad, 6e-3 if half else 1e-5)


@cases("case", [((3, 4, 9, 7), True), ((5, 64), False)], ids=lambda c: ids_x(c[0]))
def test_l1_mean_memory_contract(guards, case):
    """test_pack_blend_l1: 1e-6."""
    shape, image = case
    g = torch.Generator().manual_seed(sum(shape))
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr_ = (ar[:, :3] - br[:, :3]).abs().mean() if image else (ar - br).abs().mean()
    (lr_ * 3.0).backward()
    ad, bd = gi(a).requires_grad_(True), gi(b).requires_grad_(True)
    ld = ops.l1_mean(ad, bd, image=image)
    guards.verify()
    assert not torch.isnan(ld), "l1_mean is NaN"
    assert abs(float(ld.detach()) - float(lr_)) <= 1e-6 * max(1.0, abs(float(lr_)))
    ld.backward(gi(torch.tensor(3.0)))
    guards.verify()
    check("da", ad.grad, ar.grad, 1e-6)
    check("db", bd.grad, br.grad, 1e-6)


@single
def test_bf16_feature_l1_memory_contract(guards):
    """test_bf16_resample_blend_l1_pack, feature L1: value 1e-5 relative, gradient a stored bf16 tensor."""
    ops.set_precision("bf16")
    g = torch.Generator().manual_seed(5)
    a, b = rb(torch.randn(2, 8, 3, 5, generator=g)), rb(torch.randn(2, 8, 3, 5, generator=g))
    ar = a.clone().requires_grad_(True)
    lr_ = (ar - b).abs().mean()
    lr_.backward()
    ad = gi(a.to(BF)).requires_grad_(True)
    ld = ops.l1_mean(ad, gi(b.to(BF)))
    guards.verify()
    assert not torch.isnan(ld), "l1_mean is NaN"
    assert abs(float(ld.detach()) - float(lr_)) <= 1e-5 * float(lr_)
    ld.backward()
    guards.verify()
    check("da", ad.grad, ar.grad, 6e-3)


@cases("case", [(3, 1, 1), (4, 4, 3)], ids=ids_x)
def test_adv_tail_memory_contract(guards, case):
    """test_adv_tail_and_weighted_sum_vs_oracle."""
    B, hw, segs = case
    g = torch.Generator().manual_seed(B * 10 + hw + segs)
    src = torch.randn(segs * B, 1, hw, hw, generator=g)
    cls = torch.randn(segs * B, 8, generator=g) * 2
    labels = (torch.rand(B, 8, generator=g) > 0.5).float()
    targets, w_src, w_cls = (0.0, 0.0, 1.0)[:segs], (1.0, 0.7, 2.0)[:segs], (0.0, 0.3, 2.0)[:segs]
    sr, cr = src.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    want = 0
    for s in range(segs):
        want = want + w_src[s] * ((sr[s * B:(s + 1) * B] - targets[s]) ** 2).mean() \
            + w_cls[s] * orc.bce_with_logits_mean(cr[s * B:(s + 1) * B], labels)
    (want * 1.7).backward()
    sd, cd = gi(src, channels_last=False).requires_grad_(True), gi(cls).requires_grad_(True)
    got = ops.adv_tail(sd, cd, gi(labels), B, targets, w_src, w_cls)
    guards.verify()
    assert not torch.isnan(got), "adv_tail is NaN"
    assert abs(float(got.detach()) - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
    got.backward(gi(torch.tensor(1.7)))
    guards.verify()
    check("dsrc", sd.grad, sr.grad, 1e-5)
    check("dcls", cd.grad, cr.grad, 1e-5)


@single
def test_gmm_kl_memory_contract(guards):
    """test_gmm_kl_one_launch_matches_reference_expression at (5, 3, 16, +1): float64, 2e-6."""
    B, K, D, extra = 5, 3, 16, 1
    g = torch.Generator().manual_seed(B * 7 + K)
    mu = torch.randn(B, K, D, generator=g)
    lv = torch.randn(B, K, D, generator=g) * 0.7
    lab = (torch.rand(B, K + extra, generator=g) > 0.5).float() * 2 - 1
    sigma = 0.25
    mu64, lv64 = mu.double().requires_grad_(True), lv.double().requires_grad_(True)
    var = lv64.exp()
    want = (0.5 * (torch.log(sigma / var) + (var + (mu64 - lab.double()[:, :K].unsqueeze(-1)) ** 2) / sigma - 1.0)).sum(2).mean(0).sum()
    (want * 1.5).backward()
    mud, lvd = gi(mu).requires_grad_(True), gi(lv).requires_grad_(True)
    got = ops.gmm_kl_sp(mud, lvd, gi(lab), sigma)
    guards.verify()
    assert not torch.isnan(got), "gmm_kl_sp is NaN"
    assert abs(got.item() - want.item()) <= 2e-6 * abs(want.item()), (got.item(), want.item())
    got.backward(gi(torch.tensor(1.5)))
    guards.verify()
    check("dmu", mud.grad, mu64.grad.float(), 2e-6, 0.0)
    check("dlv", lvd.grad, lv64.grad.float(), 2e-6, 0.0)


# ---- dense and LSTM -----------------------------------------------------------------------------------------------------------------
def _linear_ref(M, K, N, relu, seed):
    g = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 0.1
    gy = torch.randn(M, N, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = F.linear(xr, wr, br)
    yr = torch.relu(yr) if relu else yr
    (yr * gy.double()).sum().backward()
    return x, w, b, gy, yr.detach().float(), xr.grad.float(), wr.grad.float(), br.grad.float()


@single
def test_linear_small_memory_contract(guards):
    """ops.linear on csrc/linear_small.hip at (16, 64, 256): test_linear_small_matches_float64, 2e-6 of the largest magnitude."""
    M, K, N = 16, 64, 256
    assert _lib.load().dwc_linear_small_ok(M, N, K) == 1
    x, w, b, gy, yr, dxr, dwr, dbr = _linear_ref(M, K, N, True, M + K + N)
    xd, wd, bd = gi(x).requires_grad_(True), gi(w).requires_grad_(True), gi(b).requires_grad_(True)
    yd = ops.linear(xd, wd, bd, "relu")
    guards.verify()
    check("y", yd, yr, 2e-6, 0.0)
    yd.backward(gi(gy))
    guards.verify()
    check("dx", xd.grad, dxr, 2e-6, 0.0)
    check("dw", wd.grad, dwr, 2e-6, 0.0)
    check("db", bd.grad, dbr, 2e-6, 0.0)


@cases("case", [(5, 12, 8), (37, 600, 1200)], ids=ids_x)
def test_linear_any_memory_contract(guards, case):
    """test_linear_any_matches_float64: 2e-5 of the largest magnitude."""
    M, K, N = case
    x, w, b, gy, yr, dxr, dwr, dbr = _linear_ref(M, K, N, False, M + K + N)
    xd, wd, bd = gi(x).requires_grad_(True), gi(w).requires_grad_(True), gi(b).requires_grad_(True)
    yd = ops.linear_any(xd, wd, bd)
    guards.verify()
    check("y", yd, yr, 2e-5, 0.0)
    yd.backward(gi(gy))
    guards.verify()
    check("dx", xd.grad, dxr, 2e-5, 0.0)
    check("dw", wd.grad, dwr, 2e-5, 0.0)
    check("db", bd.grad, dbr, 2e-5, 0.0)


@functools.lru_cache(maxsize=None)
def _lstm_ref(T_, B, I, H, lens):
    g = torch.Generator().manual_seed(T_ * 1000 + B + H)
    if lens is None:
        lens = sorted((int(v) for v in torch.randint(1, T_ + 1, (B,), generator=g)), reverse=True)
        lens[0] = T_
    x = torch.randn(T_, B, I, generator=g)
    ref = torch.nn.LSTM(I, H, 1, bidirectional=True)
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * (1.0 / H ** 0.5))
    xr = x.clone().requires_grad_(True)
    outs, (hn, cn) = ref(torch.nn.utils.rnn.pack_padded_sequence(xr, list(lens)))
    mem, _ = torch.nn.utils.rnn.pad_packed_sequence(outs, total_length=T_)
    g1, g2, g3 = torch.randn(mem.shape, generator=g), torch.randn(hn.shape, generator=g), torch.randn(cn.shape, generator=g)
    ((mem * g1).sum() + (hn * g2).sum() + (cn * g3).sum()).backward()
    return x, ref, tuple(lens), mem.detach(), hn.detach(), cn.detach(), (g1, g2, g3), xr.grad


@cases("case", [(7, 3, 12, 16, (7, 4, 1), 1), (7, 3, 12, 16, (7, 4, 1), 0), (6, 70, 12, 20, None, 1), (6, 70, 12, 20, None, 0)],
       ids=lambda c: "%dx%dx%dx%d-%s" % (c[0], c[1], c[2], c[3], "persistent" if c[5] else "per-step"))
def test_lstm_memory_contract(guards, monkeypatch, case):
    """test_lstm_bidir_matches_packed_nn_lstm, dense products on the HIP GEMM kernels.  (The persistent launches clear their scratch
    themselves -- hipMemsetAsync in dwc_lstm_seq_fwd / _bwd --, so poisoned scratch is what they must cope with.)"""
    T_, B, I, H, lens, seq = case
    monkeypatch.setattr(ops, "LSTM_SEQ", seq)
    assert ops.gemm_ok(I, 4 * H) and ops.gemm_ok(H, 4 * H)
    x, ref, lens, mem, hn, cn, (g1, g2, g3), dxr = _lstm_ref(T_, B, I, H, lens)
    xd = gi(x).requires_grad_(True)
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    par = {n: [gi(getattr(ref, n + "_l0" + suf)).requires_grad_(True) for suf in ("", "_reverse")] for n in names}
    lens_t = torch.tensor(lens)
    out, cell = ops.lstm_bidir(xd, gi(lens_t.to(torch.int32)), *[torch.stack(par[n]) for n in names], owners=tuple(par["weight_ih"]))
    guards.verify()
    if seq:
        ops.lstm_status_poll(torch.device(DEV))
        ops.lstm_status_poll(torch.device(DEV), wait=True)
        assert int(ops._lstm_status(torch.device(DEV))[0].item()) == 0
    last, cols = (lens_t - 1).to(DEV), torch.arange(B, device=DEV)
    mem_d = torch.cat([out[0], out[1]], -1)
    hn_d = torch.stack([out[0][last, cols], out[1][0]])
    cn_d = torch.stack([cell[0][last, cols], cell[1][0]])
    check("outputs", mem_d, mem, 2e-5)
    check("cell states", cell, cell.detach().float().cpu(), 0.0, 0.0)          # (NaN check of every slot, the inactive ones included)
    check("h_n", hn_d, hn, 2e-5)
    check("c_n", cn_d, cn, 2e-5)
    ((mem_d * g1.to(DEV)).sum() + (hn_d * g2.to(DEV)).sum() + (cn_d * g3.to(DEV)).sum()).backward()
    guards.verify()
    check("dx", xd.grad, dxr, 1e-4)
    for n in names:
        for k, suf in enumerate(("", "_reverse")):
            check(n + suf, par[n][k].grad, getattr(ref, n + "_l0" + suf).grad, 1e-4)


# ---- spectral norm, penalty ---------------------------------------------------------------------------------------------------------
@single
def test_sn_epilogue_memory_contract(guards, golden_dir):
    """test_sn_block_fp32_vs_reference, first case: the segmented epilogue (S = 3), forward and backward."""
    case = SN_CASES[0]
    gold = np.load(os.path.join(golden_dir, "sn_ops.npz"))
    name, B = case[0], case[1]
    blk, gg = _sn_block(case, gold)
    x = gi(torch.cat([gg("x")] * 3)).requires_grad_(True)
    y = blk(x, segments=3)
    guards.verify()
    check(name + " y1", y[:B], gg("y1"), 5e-5, 2e-6)
    check(name + " y3", y[2 * B:], gg("y3"), 5e-5, 2e-6)
    m = blk.conv.module
    check(name + " u", m.weight_u, gg("u3"), 0, 1e-5)
    check(name + " v", m.weight_v, gg("v3"), 0, 1e-5)
    y.backward(gi(torch.cat([gg("gy")] * 3)))
    guards.verify()
    check(name + " dx", x.grad.view((3, B) + tuple(x.shape[1:])).sum(0), gg("dx"), 3e-4, 2e-6)
    check(name + " dw", m.weight_bar.grad, gg("dw"), 3e-4, 2e-6)
    check(name + " db", m.bias.grad, gg("db"), 3e-4, 2e-6)


@cases("mode", ["gp", "r1"], ids=str)
def test_penalty_reduction_memory_contract(guards, mode):
    """hipdwc.penalty._penalty / _scale at (3, 5, 7): test_penalty_reduction_kernels_vs_float64, 1e-5 of the largest magnitude."""
    B, H, W = 3, 5, 7
    gen = torch.Generator().manual_seed(100 * B + H)
    g = torch.randn(B, H * W, 4, generator=gen)
    if mode == "gp":
        g[B - 1] = 0.0
    g[:, :, 3] = 1e30                                  # the padding plane: a kernel that reads it into a sum overflows
    g64 = g[:, :, :3].double()
    q64 = (g64 ** 2).sum((1, 2))
    if mode == "gp":
        r = q64.sqrt()
        P64 = ((r - 1) ** 2).mean()
        k64 = torch.where(q64 > 0, 2 * (r - 1) / (B * r.clamp_min(1e-300)), torch.zeros_like(q64))
    else:
        P64 = (q64 ** 2).mean()
        k64 = 4 * q64 / B
    ghat64 = torch.zeros(B, H * W, 4, dtype=torch.float64)
    ghat64[:, :, :3] = k64.view(B, 1, 1) * g64
    gd = gi(g.view(B, H, W, 4).permute(0, 3, 1, 2))                 # NHWC4 image buffer [B, 4, H, W]
    out, k = penalty._penalty(gd, mode)
    ghat = penalty._scale(gd, k)
    guards.verify()
    for name, got, want in (("P", out, P64), ("k", k, k64), ("ghat", ghat.permute(0, 2, 3, 1).reshape(B, H * W, 4), ghat64)):
        got = got.detach().double().cpu()
        assert not torch.isnan(got).any(), name + " holds NaN"
        err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)
        assert err <= 1e-5, (name, err)


@single
def test_penalty_act_bwd_memory_contract(guards):
    """hipdwc.penalty._act_bwd (dwc_act_bwd_bias with exactly the scratch it asks for): g = dy * lrelu'(y) is one multiply, the column
    sums at the bias-gradient tolerance of test_conv_forward_backward."""
    B, C, H, W = 3, 8, 5, 7
    gen = torch.Generator().manual_seed(17)
    y, dy = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    pre = y.clone().requires_grad_(True)                     # (lrelu keeps the sign: its derivative at y is its derivative at the pre-activation)
    orc.activation(pre, "lrelu").backward(dy)
    want = pre.grad
    g, db = penalty._act_bwd(gi(dy), gi(y), "lrelu", want_g=True, want_db=True)
    guards.verify()
    check("g", g, want, 1e-6)
    check("db", db, want.double().sum((0, 2, 3)).float(), 5e-5)


# ---- optimiser ----------------------------------------------------------------------------------------------------------------------
@single
def test_optimiser_memory_contract(guards):
    """FusedAdam, FusedEMA and the weight refresh behind the step on sizes across the 8192-element chunking, every tensor the
    launches touch in a guarded block: test_fused_adam_and_ema_match_torch, test_weight_refresh_multi_matches_single_layout_kernels."""
    from hipdwc.optim import FusedAdam, FusedEMA
    g = torch.Generator().manual_seed(0)
    shapes = [(7,), (8192,), (8193,), (20000,), (61, 20, 3, 3)]          # the last: a filter with two prepared layouts (10 980 elements)
    layouts = [("fwd", 64, 20, 1, False), ("dgrad", 64, 20, 1, False)]
    ref = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    hip = [torch.nn.Parameter(gi(p.detach(), channels_last=False)) for p in ref]
    kw = dict(lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-4)
    o_ref, o_hip = torch.optim.Adam(ref, foreach=False, **kw), FusedAdam(hip, **kw)
    for p in hip:                                                          # the moments too (FusedAdam would use torch.zeros_like)
        o_hip.state[p]["step"] = torch.tensor(0.0, dtype=torch.float32)
        o_hip.state[p]["exp_avg"] = gi(torch.zeros(p.shape), channels_last=False)
        o_hip.state[p]["exp_avg_sq"] = gi(torch.zeros(p.shape), channels_last=False)
    for kind, cop, cip, st, half in layouts:
        ops._prepped(hip[4], kind, cop, cip, st, None, half)
    launches = ops.REFRESH_STATS["launches"]
    for step in range(3):
        for a, b in zip(ref, hip):
            gr = torch.randn(a.shape, generator=g)
            a.grad, b.grad = gr.clone(), gi(gr, channels_last=False)
        o_ref.step()
        o_hip.step()
    guards.verify()
    assert ops.REFRESH_STATS["launches"] == launches + 3
    for i, (a, b) in enumerate(zip(ref, hip)):
        check("param %d" % i, b, a, 2e-6, 1e-7)
        check("m %d" % i, o_hip.state[b]["exp_avg"], o_ref.state[a]["exp_avg"], 2e-6)
        check("v %d" % i, o_hip.state[b]["exp_avg_sq"], o_ref.state[a]["exp_avg_sq"], 2e-6)
    for kind, cop, cip, st, half in layouts:
        got = ops._prepped(hip[4], kind, cop, cip, st, None, half)          # cache hit: the tensor the step's refresh rebuilt
        fresh = hip[4].detach().clone().requires_grad_(True)
        want = ops._prepped(fresh, kind, cop, cip, st, None, half)          # the single-layout kernel on the same weights
        assert got.data_ptr() != want.data_ptr()
        assert not torch.isnan(got).any(), "refreshed %s layout holds NaN" % kind
        assert torch.equal(got, want), kind
    dst = [torch.nn.Parameter(gi(torch.randn(p.shape, generator=g), channels_last=False)) for p in hip]
    want = [torch.lerp(a.detach().cpu(), b.detach().cpu(), 0.999) for a, b in zip(hip, dst)]
    FusedEMA(torch.nn.ParameterList(hip), torch.nn.ParameterList(dst)).step(0.999)
    guards.verify()
    for i, (w, b) in enumerate(zip(want, dst)):
        check("ema %d" % i, b, w, 1e-6, 1e-7)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_workspace_call_site_was_exercised():
    """Every ``workspace(`` call site of hipdwc/ops.py, spectral.py and penalty.py was reached by a case above, with scratch of exactly
    the size it asked for -- apart from at most two documented exemptions.  Judges only a run of all the module's cases."""
    missing_cases = EXPECTED - RAN
    if missing_cases:
        pytest.skip("%d of the module's %d cases did not run (a selection with -k?)" % (len(missing_cases), len(EXPECTED)))
    # the harness was in force: scratch, channels-last outputs, plain outputs and inputs all came from guarded blocks
    for kind in ("workspace", "empty_cl", "torch.empty", "torch.empty_like", "input"):
        assert ga.DEFAULT.handed.get(kind, 0) > 0, "no %s block was handed out" % kind
    assert len(EXEMPT) <= 2
    exempt = set()
    for (name, text), reason in EXEMPT.items():
        hits = [site for site, line in SITES.items() if site[0] == name and text in line]
        assert len(hits) == 1 and reason, (name, text, hits)
        exempt.add(hits[0])
    assert SEEN <= set(SITES), sorted(SEEN - set(SITES))
    assert not (SEEN & exempt), "an exempted call site is reached after all: %s" % sorted(SEEN & exempt)
    missed = sorted(set(SITES) - SEEN - exempt)
    assert not missed, "workspace() call sites no case reached: " + "; ".join("%s:%d  %s" % (s[0], s[1], SITES[s]) for s in missed)
