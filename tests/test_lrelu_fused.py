"""LeakyReLU(0.1) fused into the IN / AdaIN / LN kernels (csrc/norm.hip) and into nn.Linear on few rows (csrc/linear_small.hip):
``gen.activ: lrelu`` and ``dis.norm: in / ln`` with the default ``dis.activ: lrelu``.

Tolerances are the ones the ReLU forms are held to, measured with the same ``close`` (max|hip - ref| <= rel * max|ref| + atol):
  * fp32 norms (tests/test_hip_parity.py::test_instance_norm / test_layer_norm): y 3e-5, dx 2e-4, dgamma / dbeta 1e-4, dres 2e-5;
  * bf16 norms (tests/test_bf16_parity.py, tests/test_memory_contracts.py): y 6e-3, dx 8e-3, dgamma / dbeta 2e-3, dres 1e-6;
  * nn.Linear against float64 (tests/test_small_ops.py::test_linear_small_matches_float64): 2e-6 of the largest magnitude;
  * blocks (tests/test_hip_parity.py::test_conv_block_beyond_shipped_configs_vs_reference): y 5e-5 (+2e-6), gradients 3e-4 (+2e-6);
  * grouped decode (test_grouped_decode_equals_concatenated_decode): output 2e-6, gradients 2e-5.
LeakyReLU's kink (a jump of 0.9 in the derivative) is smaller than ReLU's: none of them is loosened.

The tests without the ``gpu`` mark (end of the file) need the built library only."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as ga

from hipdwc import _lib, ops, penalty, spectral, synth          # noqa: E402
from oracle import dwcgan_oracle as orc                          # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLOPE = 0.1


def close(a, b, rel=2e-5, atol=1e-6, msg=""):
    """tests/test_hip_parity.py::close."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = rel * b.abs().max().item() + atol
    print("%-28s max err %.3e (limit %.3e)" % (msg, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


def dev(t, grad=False):
    return t.detach().clone().to(DEV).requires_grad_(grad)


def rb(t):
    return t.to(BF).float()


@pytest.fixture(autouse=True)
def fp32_mode():
    ops.set_precision("fp32")
    yield
    ops.set_precision("fp32")


def ids_x(s):
    return "x".join(str(v) for v in s)


# ---- 1. instance norm / AdaIN + lrelu (+ residual) against the oracle expression ------------------------------------------------------
# (B, C, H): resident HW 256 / resident HW 1024 with an odd number of workgroup pairs / multi-pass, one column group / 4-pixel planes
# (D's tail) / multi-pass
# (2, 512, 5): HW 25 is no resident plane; the statistics and backward-partial walks run their unrolled loop and a tail in one workgroup,
# the apply walks split it into chunks of 8 (bf16: 16) rows -- unrolled loop only -- and a last chunk that is tail only
IN_SHAPES = [(2, 64, 16), (3, 64, 32), (2, 8, 6), (2, 512, 2), (1, 128, 8), (2, 512, 5)]
IN_SHAPES_BF16 = IN_SHAPES + [(2, 128, 16), (1, 128, 32)]            # the bf16 resident branch at C = 128 as well (C = 64 above)
IN_MODES = ["in_lrelu", "adain_lrelu", "adain_lrelu_res"]


def _instance_norm_case(prec, mode, B, C, H):
    """Inputs and the CPU reference of one case: orc.instance_norm / orc.adain, F.leaky_relu(., 0.1), + residual."""
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B * 1000 + C + H + 17)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 2 + 0.7)
    res = rnd(torch.randn(B, C, H, H, generator=g)) if mode.endswith("res") else None
    ga_ = be = None
    if mode.startswith("adain"):
        ga_ = torch.randn(B * C, generator=g) * 0.5 + 1
        ga_[0], ga_[B * C // 2] = -0.8, -1.3                         # the slope must follow the pre-activation, not x-hat
        be = torch.randn(B * C, generator=g)
    # A pre-activation within rounding of 0 leaves the slope of that element to the implementation's rounding of the mean (tests/
    # test_memory_contracts.py::test_instance_norm_memory_contract has the argument and the 1e-4): such planes are drawn again.
    for _ in range(16):
        pre = orc.adain(x, ga_, be) if ga_ is not None else orc.instance_norm(x)
        tied = (pre.abs() < 1e-4).flatten(2).any(2)
        if not tied.any():
            break
        x[tied] = rnd(torch.randn(int(tied.sum()), H, H, generator=g) * 2 + 0.7)
    assert not tied.any()
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if res is not None else None
    gr, br = (ga_.clone().requires_grad_(True), be.clone().requires_grad_(True)) if ga_ is not None else (None, None)
    yr = F.leaky_relu(orc.adain(xr, gr, br) if ga_ is not None else orc.instance_norm(xr), SLOPE)
    if rr is not None:
        yr = yr + rr
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    return x, res, ga_, be, gy, yr.detach(), xr.grad, (rr.grad if rr is not None else None), (gr.grad if gr is not None else None), \
        (br.grad if br is not None else None)


@gpu
@pytest.mark.parametrize("mode", IN_MODES)
@pytest.mark.parametrize("prec,shape", [("fp32", s) for s in IN_SHAPES] + [("bf16", s) for s in IN_SHAPES_BF16],
                         ids=lambda v: v if isinstance(v, str) else ids_x(v))
def test_instance_norm_lrelu(prec, shape, mode):
    B, C, H = shape
    half = prec == "bf16"
    x, res, ga_, be, gy, yr, dxr, drr, dgr, dbr = _instance_norm_case(prec, mode, B, C, H)
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    xd = dev(cast(x), True)
    rd = dev(cast(res), True) if res is not None else None
    gd, bd = (dev(ga_, True), dev(be, True)) if ga_ is not None else (None, None)
    yd = ops.instance_norm(xd, gd, bd, residual=rd, act="lrelu")
    ty, tdx, tp, tres = (6e-3, 8e-3, 2e-3, 1e-6) if half else (3e-5, 2e-4, 1e-4, 2e-5)
    close(yd, yr, rel=ty, msg="y")
    (yd * cast(gy).to(DEV)).sum().backward()
    close(xd.grad, dxr, rel=tdx, msg="dx")
    if rd is not None:
        close(rd.grad, drr, rel=tres, msg="dres")
    if gd is not None:
        close(gd.grad, dgr, rel=tp, msg="dgamma")
        close(bd.grad, dbr, rel=tp, msg="dbeta")


@gpu
def test_instance_norm_relu_argument_still_means_relu():
    """``relu=`` positionally and by keyword, ``act`` winning over it, and act='relu' being the same launch as relu=True."""
    g = torch.Generator().manual_seed(5)
    x = dev(torch.randn(2, 8, 6, 6, generator=g))
    a = ops.instance_norm(x, None, None, None, True)
    assert torch.equal(a, ops.instance_norm(x, relu=True)) and torch.equal(a, ops.instance_norm(x, act="relu"))
    assert torch.equal(a, ops.instance_norm(x, relu=False, act="relu"))
    assert torch.equal(ops.instance_norm(x), ops.instance_norm(x, relu=True, act="none"))
    ga_, be = dev(torch.rand(8, generator=g)), dev(torch.randn(8, generator=g))
    b = ops.layer_norm_munit(x, ga_, be, True)
    assert torch.equal(b, ops.layer_norm_munit(x, ga_, be, act="relu")) and torch.equal(b, ops.layer_norm_munit(x, ga_, be, relu=True))


# ---- 2. MUNIT layer norm + lrelu -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 128, 16), (1, 64, 32), (2, 8, 10), (2, 512, 5)], ids=ids_x)      # (2, 512, 5): see IN_SHAPES
def test_layer_norm_lrelu(prec, shape):
    B, C, H = shape
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B + C + H + 17)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 1.5 - 0.3)
    ga_, be = torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.1
    if C == 128:
        ga_[1] = -0.6                                                 # one negative gamma entry
    xr, gr, br = [t.clone().requires_grad_(True) for t in (x, ga_, be)]
    yr = F.leaky_relu(orc.layer_norm_munit(xr, gr, br), SLOPE)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    xd, gd, bd = dev(cast(x), True), dev(ga_, True), dev(be, True)
    yd = ops.layer_norm_munit(xd, gd, bd, act="lrelu")
    ty, tdx, tp = (6e-3, 8e-3, 2e-3) if half else (3e-5, 2e-4, 1e-4)
    close(yd, yr, rel=ty, msg="y")
    (yd * cast(gy).to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=tdx, msg="dx")
    close(gd.grad, gr.grad, rel=tp, msg="dgamma")
    close(bd.grad, br.grad, rel=tp, msg="dbeta")


# ---- 3. ops.linear(..., "lrelu") on csrc/linear_small.hip against float64 -------------------------------------------------------------
# (slope 0.1: the default, Conv2dBlock's; 0.2: the reference's LinearBlock, networks.py:614, what MLP(activ='lrelu') runs)
@gpu
@pytest.mark.parametrize("slope", [0.1, 0.2])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,K,N", [(16, 64, 256), (3, 16, 16)])
def test_linear_lrelu_matches_float64(monkeypatch, M, K, N, bias, slope):
    lib = _lib.load()
    assert lib.dwc_linear_small_ok(M, N, K) == 1
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    gy = torch.randn(M, N, generator=g)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    yr = F.leaky_relu(F.linear(xr, wr, br), slope)
    (yr * gy.double()).sum().backward()

    def no_conv(*a, **k):
        raise AssertionError("ops.linear(..., 'lrelu') left csrc/linear_small.hip for the 1x1-convolution form")
    monkeypatch.setattr(ops, "conv2d", no_conv)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    yd = ops.linear(xd, wd, bd, "lrelu") if slope == 0.1 else ops.linear(xd, wd, bd, "lrelu", slope=slope)
    (yd * gy.to(DEV)).sum().backward()
    for name, got, want in (("y", yd, yr), ("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad)) + ((("db", bd.grad, br.grad),) if bias else ()):
        err = (got.detach().cpu().double() - want.detach()).abs().max().item() / max(want.detach().abs().max().item(), 1e-30)
        print("%-3s max err %.2e of the largest magnitude" % (name, err))
        assert err <= 2e-6, (name, err)


@gpu
def test_linear_small_bwd_act_codes():
    """dwc_linear_small_bwd_act: code 1 is dwc_linear_small_bwd with y, code 0 ignores y; code 3, a missing y and a LeakyReLU slope
    outside (0, 1) are refused."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    M, K, N = 5, 32, 48
    x, w, dy = (torch.randn(s, generator=g).to(DEV) for s in ((M, K), (N, K), (M, N)))
    y = torch.randn(M, N, generator=g).to(DEV)
    st = ops._stream()

    def run(fn, *tail):
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(N, device=DEV)
        rc = fn(dy.data_ptr(), tail[0], x.data_ptr(), w.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), M, N, K, *tail[1:], st)
        torch.cuda.synchronize()
        return rc, dx, dw, db
    old = run(lib.dwc_linear_small_bwd, y.data_ptr())
    new = run(lib.dwc_linear_small_bwd_act, y.data_ptr(), 1, 0.1)
    assert old[0] == 0 and new[0] == 0 and all(torch.equal(a, b) for a, b in zip(old[1:], new[1:]))
    plain = run(lib.dwc_linear_small_bwd, None)
    none = run(lib.dwc_linear_small_bwd_act, y.data_ptr(), 0, 0.1)
    assert none[0] == 0 and all(torch.equal(a, b) for a, b in zip(plain[1:], none[1:]))
    assert run(lib.dwc_linear_small_bwd_act, y.data_ptr(), 3, 0.1)[0] == _lib.EINVAL
    assert run(lib.dwc_linear_small_bwd_act, None, 2, 0.1)[0] == _lib.EINVAL
    for slope in (0.0, 1.0, -0.1, float("nan")):
        assert run(lib.dwc_linear_small_bwd_act, y.data_ptr(), 2, slope)[0] == _lib.EINVAL


# ---- 4. blocks -----------------------------------------------------------------------------------------------------------------------
# (name, B, Cin, Cout, H, k, stride, pad, norm)
BLOCK_CASES = [
    ("res3_in", 2, 16, 16, 12, 3, 1, 1, "in"),
    ("dis4_in", 2, 16, 32, 16, 4, 2, 1, "in"),         # D's layer
    ("up5_ln", 2, 16, 8, 12, 5, 1, 2, "ln"),
    ("stem7_in", 2, 3, 8, 16, 7, 1, 3, "in"),
    ("stem7_none", 2, 3, 8, 16, 7, 1, 3, "none"),      # the style encoder's stem: lrelu in the convolution's epilogue
]
DIS_CASE = BLOCK_CASES[1]


def _block_reference(case):
    """F.pad(reflect) / F.conv2d / F.instance_norm or the MUNIT LN expression / F.leaky_relu on the CPU; returns the inputs too."""
    name, B, ci, co, H, k, s, p, norm = case
    g = torch.Generator().manual_seed(sum(case[1:8]) + len(name))
    x = torch.randn(B, ci, H, H, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    b = torch.randn(co, generator=g) * 0.1
    gamma, beta = torch.rand(co, generator=g), torch.randn(co, generator=g) * 0.1
    xr, wr, br, gr, ber = [t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta)]
    h = F.conv2d(F.pad(xr, (p,) * 4, mode="reflect"), wr, br, stride=s)
    if norm == "in":
        h = F.instance_norm(h, eps=1e-5)
    elif norm == "ln":
        h = orc.layer_norm_munit(h, gr, ber)
    yr = F.leaky_relu(h, SLOPE)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    ref = {"y": yr.detach(), "dx": xr.grad, "dw": wr.grad, "db": br.grad, "dgamma": gr.grad, "dbeta": ber.grad}
    return x, w, b, gamma, beta, gy, ref


def _run_block(case, inputs):
    import networks.networks as nets
    name, B, ci, co, H, k, s, p, norm = case
    x, w, b, gamma, beta, gy, _ = inputs
    blk = nets.Conv2dBlock(ci, co, k, s, p, norm=norm, activation="lrelu", pad_type="reflect").to(DEV)
    with torch.no_grad():
        blk.conv.weight.copy_(w)
        blk.conv.bias.copy_(b)
        if norm == "ln":
            blk.norm.gamma.copy_(gamma)
            blk.norm.beta.copy_(beta)
    xd = dev(x, True)
    y = blk(xd)
    (y * gy.to(DEV)).sum().backward()
    return blk, xd, y


def _check_block(case, blk, xd, y, ref, ty, tg):
    name, norm = case[0], case[8]
    close(y, ref["y"], rel=ty, atol=2e-6, msg=name + " y")
    close(xd.grad, ref["dx"], rel=tg, atol=2e-6, msg=name + " dx")
    close(blk.conv.weight.grad, ref["dw"], rel=tg, atol=2e-6, msg=name + " dw")
    if norm == "none":
        close(blk.conv.bias.grad, ref["db"], rel=tg, atol=2e-6, msg=name + " db")
    if norm == "ln":
        close(blk.norm.gamma.grad, ref["dgamma"], rel=tg, msg=name + " dgamma")
        close(blk.norm.beta.grad, ref["dbeta"], rel=tg, msg=name + " dbeta")


@gpu
@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: c[0])
def test_conv_block_lrelu_is_fused(monkeypatch, case):
    """Conv2dBlock(reflect, lrelu) with norm in / ln / none: values and gradients, and torch's leaky_relu is never reached."""
    inputs = _block_reference(case)                    # (the reference itself uses F.leaky_relu: computed before the patch)

    def no_leaky(*a, **k):
        raise AssertionError("Conv2dBlock reached torch.nn.functional.leaky_relu: the activation is not fused")
    monkeypatch.setattr(torch.nn.functional, "leaky_relu", no_leaky)
    assert ops.NORM_ACT_FUSED == 1
    blk, xd, y = _run_block(case, inputs)
    _check_block(case, blk, xd, y, inputs[-1], 5e-5, 3e-4)
    if case[8] == "in":                                # the documented IN deviation: the true bias gradient is zero, flagged, not computed
        assert blk.conv.bias.grad is None and getattr(blk.conv.bias, "_dwc_zero_grad", False)


@gpu
def test_res_block_lrelu_grouped_equals_concatenated(monkeypatch):
    """ResBlock(adain, lrelu, reflect): groups=3 keeps the one-convolution-for-three-groups form and equals the block on cat([x] * 3)."""
    import networks.networks as nets
    torch.manual_seed(11)
    B, C, H = 2, 16, 12
    blk = nets.ResBlock(dim=C, norm="adain", activation="lrelu", pad_type="reflect").to(DEV)
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn(B, C, H, H, generator=g)
    params = [(torch.randn(3 * B * C, generator=g) * 0.5 + 1, torch.randn(3 * B * C, generator=g)) for _ in range(2)]
    gy = torch.randn(3 * B, C, H, H, generator=g).to(DEV)
    batches = []
    real_conv = ops.conv2d

    def spy(x, *a, **k):
        batches.append(x.shape[0])
        return real_conv(x, *a, **k)
    monkeypatch.setattr(ops, "conv2d", spy)
    outs = []
    for grouped in (True, False):
        del batches[:]
        blk.zero_grad(set_to_none=True)
        x = dev(x0, True)
        leaves = []
        for m, (wt, bs) in zip((blk.model[0].norm, blk.model[1].norm), params):
            m.weight, m.bias = dev(wt, True), dev(bs, True)
            leaves += [m.weight, m.bias]
        y = blk(x, groups=3) if grouped else blk(torch.cat([x] * 3))
        (y * gy).sum().backward()
        assert batches == ([B, 3 * B] if grouped else [3 * B, 3 * B]), batches
        outs.append([y.detach(), x.grad.detach(), blk.model[0].conv.weight.grad.detach().clone(),
                     blk.model[1].conv.weight.grad.detach().clone()] + [t.grad.detach() for t in leaves])
    names = ("y", "dx", "dw (first conv)", "dw (second conv)", "dgamma0", "dbeta0", "dgamma1", "dbeta1")
    for a, b, name in zip(outs[0], outs[1], names):
        close(a, b, rel=2e-6 if name == "y" else 2e-5, msg="grouped vs concatenated: " + name)


# ---- 5. absmax contract --------------------------------------------------------------------------------------------------------------
def _slot_bits(slot):
    pool = ops._AMAX[torch.cuda.current_device()][0]
    return int(pool[(slot - pool.data_ptr()) // 8])


@gpu
@pytest.mark.parametrize("kind,shape", [("in", (2, 64, 16)), ("in", (2, 8, 6)), ("ln", (2, 8, 10))], ids=lambda v: v if isinstance(v, str) else ids_x(v))
def test_absmax_slot_holds_the_activated_maximum(monkeypatch, kind, shape):
    """fp32, two-plane kernels: the slot tagged on y holds exactly max|y| of the ACTIVATED values, the one on dx exactly max|dx|.
    gamma = 0.1, beta = -5: every pre-activation is about -5, so max|y| is 0.1 * |pre| -- a slot raised from the un-activated value
    would be 10 x too large."""
    monkeypatch.setattr(ops, "X3_PLANES", 2)
    B, C, H = shape
    g = torch.Generator().manual_seed(C + H)
    x = dev(torch.randn(B, C, H, H, generator=g), True)
    n = B * C if kind == "in" else C
    ga_, be = dev(torch.full((n,), 0.1), True), dev(torch.full((n,), -5.0), True)
    tags = []
    real = ops.set_amax

    def rec(t, slot, ep):
        tags.append((t, slot, ep))
        return real(t, slot, ep)
    monkeypatch.setattr(ops, "set_amax", rec)
    y = ops.instance_norm(x, ga_, be, act="lrelu") if kind == "in" else ops.layer_norm_munit(x, ga_, be, act="lrelu")
    (y * dev(torch.randn(y.shape, generator=g))).sum().backward()
    torch.cuda.synchronize()
    assert float(y.detach().max()) < 0 and 0.4 < float(y.detach().abs().max()) < 0.7      # the largest |y| is a negative pre-activation times 0.1
    assert len(tags) == 2, "one tag for y, one for dx"
    (ty, sy, ey), (tdx, sdx, edx) = tags
    assert ty.data_ptr() == y.data_ptr() and tdx.shape == x.shape
    for name, t, slot, ep in (("y", ty, sy, ey), ("dx", tdx, sdx, edx)):
        word = _slot_bits(slot)
        want = int(t.detach().abs().max().view(torch.int32))
        print("%s: slot %#x, max|t| bits %#x" % (name, word & 0xffffffff, want))
        assert word >> 32 == ep, (name, "epoch")
        assert word & 0xffffffff == want, (name, word & 0xffffffff, want)
    assert ops.amax_of(y) == (sy, ey)
    ops._amax_verify(y, (sy, ey))
    ops._amax_verify(tdx, (sdx, edx))


# ---- 6. scratch and output bounds ----------------------------------------------------------------------------------------------------
@pytest.fixture
def guards(monkeypatch):
    """tests/test_memory_contracts.py::guards: fresh scratch of exactly the requested size and every output between guard zones."""
    alloc = ga.GuardedAllocator()
    proxy = ga.TorchProxy(alloc)
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    for mod in (ops, spectral, penalty):
        monkeypatch.setattr(mod, "torch", proxy)
    yield alloc
    alloc.forget()


def _scratch_sizes(alloc):
    return sorted(n for _, n, _, label in alloc.blocks if label.startswith("workspace("))


def _nan_free(name, t):
    nan = int(torch.isnan(t.detach().float()).sum())
    assert nan == 0, "%s holds NaN in %d elements (never written, or computed from memory nobody wrote)" % (name, nan)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_instance_norm_lrelu_memory_contract(guards, prec):
    B, C, H = 2, 8, 6
    half = prec == "bf16"
    x, res, ga_, be, gy, yr, dxr, drr, dgr, dbr = _instance_norm_case(prec, "adain_lrelu_res", B, C, H)
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    gi = lambda t: ga.guarded_input(t, device=DEV)
    xd, rd = gi(cast(x)).requires_grad_(True), gi(cast(res)).requires_grad_(True)
    gd, bd = gi(ga_).requires_grad_(True), gi(be).requires_grad_(True)
    want = _lib.load().dwc_instnorm_ws_bytes(B, H * H, C)
    yd = ops.instance_norm(xd, gd, bd, residual=rd, act="lrelu")
    assert _scratch_sizes(guards) == [want]
    guards.verify()
    ty, tdx, tp, tres = (6e-3, 8e-3, 2e-3, 1e-6) if half else (3e-5, 2e-4, 1e-4, 2e-5)
    _nan_free("y", yd)
    close(yd, yr, rel=ty, msg="y")
    yd.backward(gi(cast(gy)))
    assert _scratch_sizes(guards) == [want]
    guards.verify()
    for name, got, ref, tol in (("dx", xd.grad, dxr, tdx), ("dres", rd.grad, drr, tres), ("dgamma", gd.grad, dgr, tp), ("dbeta", bd.grad, dbr, tp)):
        _nan_free(name, got)
        close(got, ref, rel=tol, msg=name)


@gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_layer_norm_lrelu_memory_contract(guards, prec):
    B, C, H = 2, 8, 10
    half = prec == "bf16"
    rnd = rb if half else (lambda t: t)
    g = torch.Generator().manual_seed(B + C + H + 17)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 1.5 - 0.3)
    ga_, be = torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.1
    xr, gr, br = [t.clone().requires_grad_(True) for t in (x, ga_, be)]
    yr = F.leaky_relu(orc.layer_norm_munit(xr, gr, br), SLOPE)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy).sum().backward()
    ops.set_precision(prec)
    cast = (lambda t: t.to(BF)) if half else (lambda t: t)
    gi = lambda t: ga.guarded_input(t, device=DEV)
    xd, gd, bd = gi(cast(x)).requires_grad_(True), gi(ga_).requires_grad_(True), gi(be).requires_grad_(True)
    want = _lib.load().dwc_layernorm_ws_bytes(B, H * H, C)
    yd = ops.layer_norm_munit(xd, gd, bd, act="lrelu")
    assert _scratch_sizes(guards) == [want]
    guards.verify()
    ty, tdx, tp = (6e-3, 8e-3, 2e-3) if half else (3e-5, 2e-4, 1e-4)
    _nan_free("y", yd)
    close(yd, yr.detach(), rel=ty, msg="y")
    yd.backward(gi(cast(gy)))
    assert _scratch_sizes(guards) == [want]
    guards.verify()
    for name, got, ref, tol in (("dx", xd.grad, xr.grad, tdx), ("dgamma", gd.grad, gr.grad, tp), ("dbeta", bd.grad, br.grad, tp)):
        _nan_free(name, got)
        close(got, ref, rel=tol, msg=name)


# ---- 8. the A/B switch ---------------------------------------------------------------------------------------------------------------
@gpu
def test_norm_act_fused_switch_reproduces_the_unfused_route(monkeypatch):
    """ops.NORM_ACT_FUSED = 0: D's in / lrelu layer takes the norm unfused, then torch's leaky_relu -- same y and gradients as the fused
    form within the bounds of test 1 (3e-5 / 2e-4)."""
    inputs = _block_reference(DIS_CASE)
    fused = _run_block(DIS_CASE, inputs)
    calls = []
    real = torch.nn.functional.leaky_relu

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(torch.nn.functional, "leaky_relu", spy)
    monkeypatch.setattr(ops, "NORM_ACT_FUSED", 0)
    unfused = _run_block(DIS_CASE, inputs)
    assert calls, "the unfused route did not call torch's leaky_relu"
    close(fused[2], unfused[2], rel=3e-5, msg="y")
    close(fused[1].grad, unfused[1].grad, rel=2e-4, msg="dx")
    close(fused[0].conv.weight.grad, unfused[0].conv.weight.grad, rel=2e-4, msg="dw")
    _check_block(DIS_CASE, unfused[0], unfused[1], unfused[2], inputs[-1], 5e-5, 3e-4)


# ---- 7. without a GPU ----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {"dwc_norm_act_ok", "dwc_linear_small_fwd_act", "dwc_linear_small_bwd_act"}


def test_new_symbols_in_header_binding_and_library():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    declared = set(re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_lib.SIGNATURES)
    assert not any("batchnorm" in n for n in NEW_SYMBOLS)
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert getattr(lib, n) is not None
    assert [lib.dwc_norm_act_ok(a) for a in (0, 1, 2, 3, -1)] == [1, 1, 1, 0, 0]


def test_abi_version_agrees_in_header_binding_and_library():
    """The fused-activation entry points were additive (ABI 10 as it was); the version has moved on since (11: the plan queries of the
    im2col entry layer).  Header, binding and library must name the same one."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    version = int(re.search(r"#define\s+DWC_ABI_VERSION\s+(\d+)\b", header).group(1))
    assert version == 11
    assert _lib.ABI_VERSION == version and _lib.load().dwc_version() == version


def test_norm_entry_points_refuse_unknown_activation_codes():
    """Codes other than 0 / 1 / 2 return DWC_EINVAL before any launch (no device needed: null pointers are never touched)."""
    lib = _lib.load()
    ws = 1 << 20
    for act in (3, 4, -1, 7):
        assert lib.dwc_instnorm_fwd(None, None, None, None, None, None, None, 2, 36, 8, 1e-5, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_instnorm_bwd(None, None, None, None, None, None, None, None, None, 2, 36, 8, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_bf16_instnorm_fwd(None, None, None, None, None, None, None, 2, 36, 8, 1e-5, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_layernorm_fwd(None, None, None, None, None, None, 2, 36, 8, 1e-5, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_layernorm_bwd(None, None, None, None, None, None, None, None, None, 2, 36, 8, 1e-5, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_bf16_layernorm_bwd(None, None, None, None, None, None, None, None, None, 2, 36, 8, 1e-5, act, 1, ws, None) == _lib.EINVAL
        assert lib.dwc_linear_small_fwd(1, 1, None, 1, 4, 16, 16, act, None) == _lib.EINVAL
        assert lib.dwc_linear_small_fwd_act(1, 1, None, 1, 4, 16, 16, act, 0.1, None) == _lib.EINVAL
    for slope in (0.0, 1.0, -0.1, float("nan")):
        assert lib.dwc_linear_small_fwd_act(1, 1, None, 1, 4, 16, 16, 2, slope, None) == _lib.EINVAL


def test_linear_block_accepts_lrelu_only():
    import networks.networks as nets
    blk = nets.LinearBlock(8, 8, activation="lrelu")
    assert blk.act_kind == "lrelu" and blk.LRELU_SLOPE == 0.2          # reference networks.py:614
    with pytest.raises(NotImplementedError):
        nets.LinearBlock(8, 8, activation="tanh")
    with pytest.raises(NotImplementedError):
        nets.LinearBlock(8, 8, norm="ln")


def test_unknown_norm_activation_is_a_value_error():
    x = torch.randn(1, 8, 4, 4)
    with pytest.raises(ValueError):
        ops.instance_norm(x, act="selu")
    with pytest.raises(ValueError):
        ops.layer_norm_munit(x, torch.ones(8), torch.zeros(8), act="tanh")


def test_generator_with_lrelu_constructs_like_relu():
    from networks.networks_v2 import AdaINGen_v2
    from vocab import Vocab
    shapes = {}
    for activ in ("relu", "lrelu"):
        cfg = synth.make_config(image_size=32, tiny=True)
        cfg["gen"]["activ"] = activ
        torch.manual_seed(1)
        gen = AdaINGen_v2(cfg["input_dim"], Vocab(dataset=cfg["dataset"]), cfg["gen"])
        shapes[activ] = [(k, tuple(v.shape)) for k, v in gen.state_dict().items()]
    assert shapes["lrelu"] == shapes["relu"] and shapes["relu"]
