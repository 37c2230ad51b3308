"""Batch normalisation, Conv2dBlock(norm='bn') / dis.norm 'bn' (reference networks.py:542 nn.BatchNorm2d), on the segmented kernels of
csrc/norm.hip (hipdwc.batchnorm).

CPU: the C ABI's new symbols agree between header, ctypes table and library (they came with ABI 10); the tiny 'bn' Solver is built bit-equal to the
reference and loads its state_dict strictly; the stock-op form of the segmented semantics (DWC_BN_HIP=0) against single calls of
nn.BatchNorm2d in float64.  GPU: the kernels against float64 on every launch-plan branch (fp32 and bf16), running statistics in a
given order, eval mode, one segmented call = S single calls bit for bit, run-to-run bit equality, the reference's block
(tests/golden/make_golden_bn.py), guarded buffers, absmax slots, and the tiny 'bn' Solver over two iterations against the imported
reference, buffers included."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as ga
import tiny_solver as ts
from hipdwc import _lib, batchnorm, ops, synth

T = torch.from_numpy
DEV = "cuda:0"
BF = torch.bfloat16
ACTS = ("none", "relu", "lrelu")

# (name, B, Cin, Cout, H, k, stride, pad, activation) -- tests/golden/make_golden_bn.py BN_CASES
BN_CASES = [
    ("k4s2_lrelu", 2, 16, 32, 16, 4, 2, 1, "lrelu"),
    ("k3s1_relu", 2, 8, 16, 12, 3, 1, 1, "relu"),
    ("k4s2_none", 2, 8, 16, 8, 4, 2, 1, "none"),
    ("k3s1_tanh", 2, 16, 8, 10, 3, 1, 1, "tanh"),
]

# (S, Bs, C, H): segments, samples per segment, channels, plane edge
SHAPES = [
    (1, 2, 8, 6),
    (3, 3, 16, 2),        # HW 4 < row groups
    (4, 2, 64, 16),       # 4 chunks
    (2, 1, 512, 4),
    (3, 2, 128, 9),       # HW 81, ragged chunk
    (2, 1, 1024, 3),      # one row group
    (2, 5, 256, 32),
    (1, 2, 512, 5),       # HW 25: the unrolled walk and its tail in one workgroup; apply chunks of 8 / 16 rows, the last one tail only
    (1, 2, 24, 6),        # idle row groups: bf16 3 column groups x 85 row groups, thread 255 idles; fp32 6 x 42, four idle threads
]


def ids_x(s):
    return "x".join(str(v) for v in s)


def close(a, b, rel, atol=1e-6, msg=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    assert not torch.isnan(a).any(), msg + ": NaN"
    err = (a - b).abs().max().item()
    lim = rel * b.abs().max().item() + atol
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


def _bn_config():
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = "bn"
    return cfg


def _act(y, act):
    return {"none": lambda t: t, "relu": torch.relu, "lrelu": lambda t: F.leaky_relu(t, 0.1), "tanh": torch.tanh}[act](y)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
BN_SYMBOLS = {"dwc_batchnorm_ws_bytes", "dwc_batchnorm_fwd", "dwc_batchnorm_bwd", "dwc_batchnorm_fwd_amax", "dwc_batchnorm_bwd_amax",
              "dwc_bf16_batchnorm_fwd", "dwc_bf16_batchnorm_bwd"}


def test_bn_symbols_header_table_library():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    declared = {n for n in re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header) if "batchnorm" in n}
    assert declared == BN_SYMBOLS
    assert {n for n in _lib.SIGNATURES if "batchnorm" in n} == BN_SYMBOLS
    version = int(re.search(r"#define\s+DWC_ABI_VERSION\s+(\d+)\b", header).group(1))      # (10 brought these symbols; 11 since the plan queries)
    assert version >= 10 and _lib.ABI_VERSION == version
    assert int(re.search(r"#define\s+DWC_BN_MAX_SEGMENTS\s+(\d+)", header).group(1)) == _lib.BN_MAX_SEGMENTS == 8
    assert ctypes.sizeof(_lib.BnOrder) == 4 * 9
    lib = _lib.load()
    assert lib.dwc_version() == version
    for n in BN_SYMBOLS:
        assert hasattr(lib, n), n
    # scratch: two planes of per-(sample, chunk, channel) partials and two of per-(segment, channel) sums, whatever S
    assert lib.dwc_batchnorm_ws_bytes(3, 3, 64, 16) >= (2 * 9 * 16 + 2 * 3 * 16) * 4
    assert lib.dwc_batchnorm_ws_bytes(2, 2, 4096, 8) >= lib.dwc_batchnorm_ws_bytes(1, 2, 4096, 8) * 2 - 64


def test_tiny_bn_init_equals_reference(golden_dir):
    import networks.networks as nets
    ref = np.load(os.path.join(golden_dir, "tiny_bn_init.npz"))
    s = ts.build(_bn_config())
    for prefix, mod in (("init/gen/", s.gen), ("init/dis/", s.dis)):
        sd = mod.state_dict()
        want = {k[len(prefix):]: ref[k] for k in ref.files if k.startswith(prefix)}
        assert list(sd.keys()) == list(want.keys())
        for k, v in want.items():
            assert sd[k].shape == v.shape and sd[k].dtype == T(v).dtype, k
            assert torch.equal(sd[k], T(v)), k          # same seed, same draw order: bit-exact
    assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
    bns = s.dis.bn_layers()
    assert len(bns) == 2 * 2 and all(isinstance(m, torch.nn.BatchNorm2d) and isinstance(m, nets.SegmentedBatchNorm2d) for m in bns)
    assert not type(bns[0]).__name__.startswith(("Conv", "Linear"))
    sd = s.dis.state_dict()
    assert "cnns_feat.0.1.norm.running_var" in sd and "cnns_feat.0.1.norm.num_batches_tracked" in sd
    assert "cnns_feat.0.0.norm.weight" not in sd                      # the first layer has no norm, as in the reference
    in_opt = {id(p) for p in s.dis_opt.param_groups[0]["params"]}
    assert all(id(m.weight) in in_opt and id(m.bias) in in_opt for m in bns)
    # a reference checkpoint loads strictly
    fresh = ts.build(_bn_config())
    fresh.dis.load_state_dict({k[len("init/dis/"):]: T(ref[k]) for k in ref.files if k.startswith("init/dis/")}, strict=True)


def test_bn_stock_op_path_on_cpu_vs_single_calls(monkeypatch):
    """DWC_BN_HIP=0: one segmented call on [x0 | x1 | x2] with order (0, 2, 1, 2) against four calls of nn.BatchNorm2d on x0, x2, x1,
    x2, float64: outputs, gradients, running buffers, num_batches_tracked; then eval mode."""
    import networks.networks as nets
    monkeypatch.setattr(batchnorm, "BN_HIP", 0)
    g = torch.Generator().manual_seed(11)
    C, Bs = 6, 2
    xs = [(torch.randn(Bs, C, 5, 4, generator=g, dtype=torch.float64) * (1 + j) + j).requires_grad_(True) for j in range(3)]
    gys = [torch.randn(Bs, C, 5, 4, generator=g, dtype=torch.float64) for _ in range(3)]
    ref = torch.nn.BatchNorm2d(C).double()
    mod = nets.SegmentedBatchNorm2d(C).double()
    with torch.no_grad():
        for m in (ref, mod):
            m.weight.copy_(torch.linspace(-1.0, 1.5, C))
            m.bias.copy_(torch.linspace(0.3, -0.2, C))
    want = {}
    for j in (0, 2, 1, 2):
        want[j] = F.leaky_relu(ref(xs[j]), 0.1)
    sum((want[j] * gys[j]).sum() for j in range(3)).backward()
    want_dx = [x.grad.clone() for x in xs]
    for x in xs:
        x.grad = None
    y = mod(torch.cat(xs), act="lrelu", segments=3, stat_order=(0, 2, 1, 2))
    (y * torch.cat(gys)).sum().backward()
    for j in range(3):
        close(y[j * Bs:(j + 1) * Bs], want[j], rel=1e-12, atol=1e-12, msg="y%d" % j)
    for j in range(3):          # (segment 2 is called twice with the same value; the loss holds it once on both sides)
        close(xs[j].grad, want_dx[j], rel=1e-10, atol=1e-12, msg="dx%d" % j)
    close(mod.running_mean, ref.running_mean, rel=1e-12, atol=1e-14, msg="running_mean")
    close(mod.running_var, ref.running_var, rel=1e-12, atol=1e-14, msg="running_var")
    assert int(mod.num_batches_tracked) == int(ref.num_batches_tracked) == 4
    ref.eval()
    mod.eval()
    rm = mod.running_mean.clone()
    close(mod(xs[1].detach(), act="relu"), torch.relu(ref(xs[1].detach())), rel=1e-12, atol=1e-12, msg="eval y")
    assert torch.equal(mod.running_mean, rm) and int(mod.num_batches_tracked) == 4
    # a segment outside the order leaves the buffers alone; default order = every segment once
    mod.train()
    before = mod.running_var.clone()
    mod(torch.cat([t.detach() for t in xs]), segments=3, stat_order=())
    assert torch.equal(mod.running_var, before) and int(mod.num_batches_tracked) == 4
    mod(torch.cat([t.detach() for t in xs]), segments=3)
    assert int(mod.num_batches_tracked) == 7


def test_bn_argument_errors(monkeypatch):
    monkeypatch.setattr(batchnorm, "BN_HIP", 0)
    x, w, b = torch.randn(2, 4, 1, 1), torch.ones(4), torch.zeros(4)
    rm, rv = torch.zeros(4), torch.ones(4)
    with pytest.raises(NotImplementedError):
        batchnorm.batch_norm(x, w, b, rm, rv, momentum=None)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        batchnorm.batch_norm(x, w, b, rm, rv, segments=2)            # one value per (segment, channel), as torch refuses it
    with pytest.raises(ValueError):
        batchnorm.batch_norm(x, w, b, rm, rv, segments=2, order=(0, 2))
    with pytest.raises(ValueError):
        batchnorm.batch_norm(torch.randn(3, 4, 2, 2), w, b, rm, rv, segments=2)
    with pytest.raises(ValueError):
        batchnorm.batch_norm(x, w, b, rm, rv, act="tanh")
    monkeypatch.setattr(batchnorm, "BN_HIP", 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        batchnorm.batch_norm(torch.randn(2, 4, 2, 2), w, b, rm, rv)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: kernels against float64
# ---------------------------------------------------------------------------------------------------------------------------------
def rb(t):
    return t.to(BF).float()


def _stats64(x, S):
    """Per segment: (mean, biased variance, unbiased variance), float64 [S, C]."""
    xs = x.double().reshape(S, -1, *x.shape[1:])
    mean = xs.mean((1, 3, 4))
    n = xs.shape[1] * xs.shape[3] * xs.shape[4]
    var = ((xs - mean[:, None, :, None, None]) ** 2).mean((1, 3, 4))
    return mean, var, var * (n / (n - 1.0))


def _forward64(x, ga, be, S, act, eps=1e-5):
    xs = x.double().reshape(S, -1, *x.shape[1:])
    mu = xs.mean((1, 3, 4), keepdim=True)
    v = ((xs - mu) ** 2).mean((1, 3, 4), keepdim=True)
    pre = ((xs - mu) / torch.sqrt(v + eps)).reshape(x.shape) * ga.double()[None, :, None, None] + be.double()[None, :, None, None]
    return pre, _act(pre, act)


def _running64(x, S, order, rm0, rv0, momentum=0.1):
    mean, _, uvar = _stats64(x, S)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    for j in order:
        rm = (1 - momentum) * rm + momentum * mean[j]
        rv = (1 - momentum) * rv + momentum * uvar[j]
    return rm, rv


@functools.lru_cache(maxsize=32)
def _case(shape, act, offsets, half):
    """(x, gamma, beta, gy, y, dx, dgamma, dbeta) with the float64 results, computed once per case and never modified.  gamma has
    negative entries.  With an activation, elements whose pre-activation lies within 1e-4 of the kink are moved off it: there the
    derivative is left to the rounding of the mean (1e-4 is far above the fp32 rounding of a normalised value, a few 1e-7, and far
    below anything a wrong kernel would be excused by); bf16 inputs are rounded first, so the reference sees what the kernel reads."""
    S, Bs, C, H = shape
    B = S * Bs
    g = torch.Generator().manual_seed(S * 1000 + Bs * 100 + C + H + (7 if offsets else 0))
    rnd = rb if half else (lambda t: t)
    x = torch.randn(B, C, H, H, generator=g) * 2 + 0.7
    if offsets:
        x = x + 10.0 * torch.arange(B, dtype=torch.float32)[:, None, None, None]      # per-sample pivots far apart
    x = rnd(x)
    ga = torch.randn(C, generator=g) * 0.5 + 1
    ga[1::3] = -ga[1::3]
    be = torch.randn(C, generator=g) * 0.3
    if act != "none":
        for _ in range(32):
            pre, _ = _forward64(x, ga, be, S, "none")
            tied = pre.abs() < 1e-4
            if not tied.any():
                break
            x = rnd(torch.where(tied, x + 0.25 + x.abs() / 64, x))      # (several bf16 steps at any magnitude)
        assert not tied.any()
    xr, gr, br = x.double().requires_grad_(True), ga.double().requires_grad_(True), be.double().requires_grad_(True)
    _, yr = _forward64(xr, gr, br, S, act)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy.double()).sum().backward()
    return x, ga, be, gy, yr.detach(), xr.grad, gr.grad, br.grad


def _dev(t, half=False, grad=False):
    t = t.to(DEV)
    if t.dim() == 4:
        t = (t.to(BF) if half else t).contiguous(memory_format=torch.channels_last)
    return t.requires_grad_(True) if grad else t


def _run(shape, act, x, ga, be, gy, half, order=None, rm=None, rv=None):
    S, Bs, C, H = shape
    xd, gd, bd = _dev(x, half, True), _dev(ga, grad=True), _dev(be, grad=True)
    rm = torch.zeros(C, device=DEV) if rm is None else rm
    rv = torch.ones(C, device=DEV) if rv is None else rv
    y = batchnorm.batch_norm(xd, gd, bd, rm, rv, segments=S, order=order, act=act)
    assert y.dtype == (BF if half else torch.float32) and y.is_contiguous(memory_format=torch.channels_last)
    (y.float() * gy.to(DEV)).sum().backward()
    return y, xd.grad, gd.grad, bd.grad, rm, rv


TOL = {False: (3e-5, 2e-4, 1e-4), True: (6e-3, 8e-3, 2e-3)}      # y, dx, dgamma / dbeta: test_instance_norm / test_bf16_instance_norm


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets", [False, True], ids=["plain", "offsets"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids_x)
def test_bn_kernels_vs_float64(shape, act, offsets, half):
    S, Bs, C, H = shape
    x, ga, be, gy, yr, dxr, dgr, dbr = _case(shape, act, offsets, half)
    y, dx, dg, db, rm, rv = _run(shape, act, x, ga, be, gy, half)
    ty, tdx, tp = TOL[half]
    close(y, yr, ty, msg="y")
    close(dx, dxr, tdx, msg="dx")
    close(dg, dgr, tp, msg="dgamma")
    close(db, dbr, tp, msg="dbeta")
    wm, wv = _running64(x, S, range(S), torch.zeros(C), torch.ones(C))
    close(rm, wm, 1e-5, atol=0, msg="running_mean")
    close(rv, wv, 1e-5, atol=0, msg="running_var")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 2, 8, 6), (3, 2, 128, 9), (2, 5, 256, 32)], ids=ids_x)
def test_bn_large_common_offset(shape):
    """x = 40 + 0.05 randn: E[x^2] - E[x]^2 in fp32 is about 4 % off here (1600 against a variance of 0.0025); the pivoted,
    parallel-variance statistics keep test_bn_kernels_vs_float64's tolerance."""
    S, Bs, C, H = shape
    g = torch.Generator().manual_seed(C + H)
    x = 40.0 + 0.05 * torch.randn(S * Bs, C, H, H, generator=g)
    ga, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    _, yr = _forward64(x, ga, be, S, "none")
    naive = (x ** 2).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2                 # what the kernels must not do
    assert ((naive.double() - x.double().var((0, 2, 3), unbiased=False)).abs() / 0.0025).max() > 0.01
    y, _, _, _, rm, rv = _run(shape, "none", x, ga, be, torch.zeros_like(x), False)
    close(y, yr, 3e-5, msg="y")
    wm, wv = _running64(x, S, range(S), torch.zeros(C), torch.ones(C))
    close(rm, wm, 1e-5, atol=0, msg="running_mean")
    close(rv, wv, 1e-5, atol=0, msg="running_var")


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 3, 16, 2), (3, 2, 128, 9)], ids=ids_x)
def test_bn_running_statistics_in_order(shape, half):
    """Order (0, 2, 1, 2) -- the D step's -- against the sequential float64 update from non-trivial buffers; a repeated and a
    permuted entry both matter at this tolerance."""
    S, Bs, C, H = shape
    x, ga, be, gy = _case(shape, "lrelu", True, half)[:4]
    g = torch.Generator().manual_seed(3)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    order = (0, 2, 1, 2)
    _, _, _, _, rm, rv = _run(shape, "lrelu", x, ga, be, gy, half, order=order, rm=rm0.to(DEV), rv=rv0.to(DEV))
    wm, wv = _running64(x, S, order, rm0, rv0)
    close(rm, wm, 1e-5, atol=0, msg="running_mean")
    close(rv, wv, 1e-5, atol=0, msg="running_var")
    for wrong in ((0, 1, 2, 2), (0, 1, 2)):
        om, _ = _running64(x, S, wrong, rm0, rv0)
        assert (om - wm).abs().max() > 100 * 1e-5 * wm.abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,C,H", [(3, 16, 5), (2, 64, 12)])
def test_bn_eval_mode(B, C, H, act, half):
    """training=False: the running buffers normalise, nothing is written to them, the backward has no coupling terms."""
    g = torch.Generator().manual_seed(B + C + H)
    rnd = rb if half else (lambda t: t)
    x = rnd(torch.randn(B, C, H, H, generator=g) * 2 + 0.7)
    ga, be = torch.randn(C, generator=g) * 0.5 + 1, torch.randn(C, generator=g) * 0.3
    ga[1::3] = -ga[1::3]
    rm0, rv0 = torch.randn(C, generator=g) * 0.5 + 0.7, torch.rand(C, generator=g) * 4 + 1
    xr, gr, br = x.double().requires_grad_(True), ga.double().requires_grad_(True), be.double().requires_grad_(True)
    pre = F.batch_norm(xr, rm0.double(), rv0.double(), gr, br, False, 0.1, 1e-5)
    assert act == "none" or not (pre.abs() < 1e-5).any()
    yr = _act(pre, act)
    gy = rnd(torch.randn(yr.shape, generator=g))
    (yr * gy.double()).sum().backward()
    xd, gd, bd = _dev(x, half, True), _dev(ga, grad=True), _dev(be, grad=True)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    y = batchnorm.batch_norm(xd, gd, bd, rm, rv, segments=3 if B % 3 == 0 else 1, act=act, training=False)
    (y.float() * gy.to(DEV)).sum().backward()
    ty, tdx, tp = TOL[half]
    close(y, yr, ty, msg="y")
    close(xd.grad, xr.grad, tdx, msg="dx")
    close(gd.grad, gr.grad, tp, msg="dgamma")
    close(bd.grad, br.grad, tp, msg="dbeta")
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: segments, determinism
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1], ids=ids_x)
def test_bn_segmented_call_equals_single_calls(shape, half):
    """One call over S segments = S calls on the slices: y and dx bit for bit (a segment's statistics do not depend on S), dgamma /
    dbeta (summed over the segments in another order) to 1e-6, the buffers after the sequence bit for bit."""
    S, Bs, C, H = shape
    x, ga, be, gy = _case(shape, "lrelu", True, half)[:4]
    y, dx, dg, db, rm, rv = _run(shape, "lrelu", x, ga, be, gy, half)
    rm1, rv1 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    dg1 = db1 = 0
    for s in range(S):
        sl = slice(s * Bs, (s + 1) * Bs)
        ys, dxs, dgs, dbs, _, _ = _run((1, Bs, C, H), "lrelu", x[sl], ga, be, gy[sl], half, rm=rm1, rv=rv1)
        assert torch.equal(ys, y[sl]), "y of segment %d" % s
        assert torch.equal(dxs, dx[sl]), "dx of segment %d" % s
        dg1, db1 = dg1 + dgs, db1 + dbs
    close(dg, dg1, 1e-6, atol=1e-7, msg="dgamma")
    close(db, db1, 1e-6, atol=1e-7, msg="dbeta")
    assert torch.equal(rm, rm1) and torch.equal(rv, rv1)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2, 128, 9), (2, 5, 256, 32)], ids=ids_x)
def test_bn_second_run_is_bit_equal(shape, half):
    x, ga, be, gy = _case(shape, "relu", False, half)[:4]
    a = _run(shape, "relu", x, ga, be, gy, half, order=(0, 1, 0))
    b = _run(shape, "relu", x, ga, be, gy, half, order=(0, 1, 0))
    for u, v, name in zip(a, b, ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")):
        assert torch.equal(u, v), name


@pytest.mark.gpu
def test_bn_unsupported_channels_take_the_stock_path_and_entry_points_refuse():
    """C = 6 is not a multiple of 4: batch_norm runs the stock-op form (same semantics); the entry point itself answers DWC_EINVAL for
    that, for S = 9, an order entry >= S, nine updates and N < 2, and DWC_EWORKSPACE for short scratch -- nothing is launched."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 6, 3, 3, generator=g)
    ga, be = torch.rand(6, generator=g) + 0.5, torch.randn(6, generator=g)
    _, yr = _forward64(x, ga, be, 2, "relu")
    rm, rv = torch.zeros(6, device=DEV), torch.ones(6, device=DEV)
    assert not batchnorm.supported(x.to(DEV), 2)
    y = batchnorm.batch_norm(x.to(DEV), ga.to(DEV), be.to(DEV), rm, rv, segments=2, order=(1, 0, 1), act="relu")
    close(y, yr, 3e-5, msg="y")
    wm, wv = _running64(x, 2, (1, 0, 1), torch.zeros(6), torch.ones(6))
    close(rm, wm, 1e-5, atol=0, msg="running_mean")
    close(rv, wv, 1e-5, atol=0, msg="running_var")
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=DEV)
    p = t.data_ptr()

    def fwd(S=2, Bs=2, HW=9, C=8, order=(0, 1), training=1, ws_bytes=1 << 16):
        o = _lib.BnOrder(len(order), (ctypes.c_int * 8)(*(list(order) + [0] * 8)[:8]))
        return lib.dwc_batchnorm_fwd(p, p, p, p, p, p, p, p, S, Bs, HW, C, 1e-5, 0.1, 0, training, o, p, ws_bytes, ops._stream())
    assert fwd(C=6) == fwd(S=9) == fwd(S=0) == fwd(order=(0, 2)) == fwd(order=(0,) * 9) == fwd(Bs=1, HW=1) == fwd(C=4 * 257) == -1
    assert fwd(training=0) == -1                                       # eval mode is one segment
    assert lib.dwc_bf16_batchnorm_fwd(p, p, p, p, p, p, p, p, 1, 2, 9, 12, 1e-5, 0.1, 0, 1, _lib.BnOrder(), p, 1 << 16, ops._stream()) == -1
    assert fwd(ws_bytes=64) == -2
    assert lib.dwc_batchnorm_bwd(p, p, p, p, p, p, p, p, p, 2, 2, 9, 8, 0, 1, p, 64, ops._stream()) == -2
    assert lib.dwc_batchnorm_bwd(p, p, p, p, p, p, p, p, p, 2, 2, 9, 8, 3, 1, p, 1 << 16, ops._stream()) == -1      # tanh is not fused
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the block against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: c[0])
def test_bn_block_vs_reference(golden_dir, case):
    """Three consecutive calls of the reference's block on x_a, x_b, x_a vs ONE call on [x_a | x_b], S = 2, order (0, 1, 0): the two
    x_a calls have the same value, so their gy add on segment 0 (tolerances of test_conv_block_beyond_shipped_configs_vs_reference)."""
    import networks.networks as nets
    gold = np.load(os.path.join(golden_dir, "bn_ops.npz"))
    name, B, ci, co, H, k, s_, p, act = case
    gg = lambda key: T(gold["%s/%s" % (name, key)])
    blk = nets.Conv2dBlock(ci, co, k, s_, p, norm="bn", activation=act, pad_type="reflect").to(DEV)
    with torch.no_grad():
        blk.conv.weight.copy_(gg("w"))
        blk.conv.bias.copy_(gg("b"))
        blk.norm.weight.copy_(gg("bn_w"))
        blk.norm.bias.copy_(gg("bn_b"))
    assert torch.equal(gg("y1"), gg("y3"))
    xa, xb = gg("xa").to(DEV).requires_grad_(True), gg("xb").to(DEV).requires_grad_(True)
    y = blk(torch.cat([xa, xb]), segments=2, stat_order=(0, 1, 0))
    close(y[:B], gg("y1"), rel=5e-5, atol=2e-6, msg=name + " y1")
    close(y[B:], gg("y2"), rel=5e-5, atol=2e-6, msg=name + " y2")
    close(blk.norm.running_mean, gg("running_mean3"), rel=1e-5, atol=0, msg=name + " running_mean")
    close(blk.norm.running_var, gg("running_var3"), rel=1e-5, atol=0, msg=name + " running_var")
    assert int(blk.norm.num_batches_tracked) == 3
    (y * torch.cat([gg("gy1") + gg("gy3"), gg("gy2")]).to(DEV)).sum().backward()
    close(xa.grad, gg("dxa"), rel=3e-4, atol=2e-6, msg=name + " dxa")
    close(xb.grad, gg("dxb"), rel=3e-4, atol=2e-6, msg=name + " dxb")
    close(blk.conv.weight.grad, gg("dw"), rel=3e-4, atol=2e-6, msg=name + " dw")
    close(blk.norm.weight.grad, gg("dbn_w"), rel=3e-4, atol=2e-6, msg=name + " dbn_w")
    close(blk.norm.bias.grad, gg("dbn_b"), rel=3e-4, atol=2e-6, msg=name + " dbn_b")
    bg = blk.conv.bias.grad                                           # identically zero in training mode: none, or exact zeros
    assert bg is None or not bg.any()
    # the buffers after one and two calls: single-segment calls in sequence
    blk1 = nets.Conv2dBlock(ci, co, k, s_, p, norm="bn", activation=act, pad_type="reflect").to(DEV)
    blk1.load_state_dict({k_: v for k_, v in blk.state_dict().items() if "running" not in k_ and "tracked" not in k_}, strict=False)
    with torch.no_grad():
        close(blk1(xa.detach()), gg("y1"), rel=5e-5, atol=2e-6, msg=name + " single call")
        close(blk1.norm.running_var, gg("running_var1"), rel=1e-5, atol=0, msg=name + " running_var after one call")
        blk1(xb.detach())
        close(blk1.norm.running_mean, gg("running_mean2"), rel=1e-5, atol=0, msg=name + " running_mean after two calls")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: guarded buffers, absmax slots
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def guards(monkeypatch):
    """tests/guarded_alloc.py applied to hipdwc.batchnorm: fresh, poisoned, guarded scratch of exactly the size asked for, and
    every output of the module (channels-last results, statistics, parameter gradients) between guards."""
    alloc = ga.GuardedAllocator()
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    monkeypatch.setattr(batchnorm, "torch", ga.TorchProxy(alloc))
    yield alloc
    alloc.forget()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(1, 2, 8, 6), (3, 2, 128, 9)], ids=ids_x)
def test_bn_memory_contract(guards, shape, training, half):
    """No write outside scratch or outputs, and no NaN left in an output (poisoned buffers: an element nobody writes, or a value
    computed from scratch nobody wrote, is NaN), at the smallest and the ragged shape."""
    S, Bs, C, H = shape
    if not training:
        S, Bs = 1, S * Bs
    x, ga_, be, gy, yr, dxr, dgr, dbr = _case(shape, "lrelu", False, half)
    xd = guards.guarded_input((x.to(BF) if half else x), device=DEV).requires_grad_(True)
    gd, bd = guards.guarded_input(ga_, device=DEV).requires_grad_(True), guards.guarded_input(be, device=DEV).requires_grad_(True)
    rm, rv = guards.guarded_input(torch.zeros(C), device=DEV), guards.guarded_input(torch.ones(C), device=DEV)
    y = batchnorm.batch_norm(xd, gd, bd, rm, rv, segments=S, order=tuple(range(S)) + (0,), act="lrelu", training=training)
    guards.verify()
    assert guards.handed.get("workspace", 0) == 1 and guards.handed.get("empty_cl", 0) == 1
    ty, tdx, tp = TOL[half]
    if training:
        close(y, yr, ty, msg="y")
    else:
        assert not torch.isnan(y.float()).any() and torch.equal(rm.cpu(), torch.zeros(C))
    y.backward(guards.guarded_input(gy.to(BF) if half else gy, device=DEV))
    guards.verify()
    for name, t in (("dx", xd.grad), ("dgamma", gd.grad), ("dbeta", bd.grad), ("running_mean", rm), ("running_var", rv)):
        assert not torch.isnan(t.float()).any(), name
    if training:
        close(xd.grad, dxr, tdx, msg="dx")
        close(gd.grad, dgr, tp, msg="dgamma")
        close(bd.grad, dbr, tp, msg="dbeta")


@pytest.fixture
def slots(monkeypatch):
    recs = []
    real = ops.set_amax

    def set_amax(t, slot, ep):
        recs.append((t, slot, ep))
        return real(t, slot, ep)
    monkeypatch.setattr(ops, "set_amax", set_amax)
    return recs


def _slot_word(slot):
    torch.cuda.synchronize()
    pool = ops._AMAX[torch.cuda.current_device()][0]
    return int(pool[(slot - pool.data_ptr()) // 8])


def _assert_tag(t, slot, ep, what):
    word = _slot_word(slot)
    bits = int(t.detach().abs().max().view(torch.int32))
    assert (word >> 32) == ep, "%s: slot epoch %d, tag says %d" % (what, word >> 32, ep)
    assert (word & 0xffffffff) == bits, "%s: slot holds %#x, max|t| is %#x" % (what, word & 0xffffffff, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", [(1, 2, 8, 6), (3, 2, 128, 9), (4, 2, 64, 16), (1, 2, 12, 6)], ids=ids_x)      # (C = 12: 3 x 85 threads walk rows, thread 255 idles up to the publish barrier)
def test_bn_absmax_slots(slots, shape, where):
    """The tag of y and of dx equals max|t| bit for bit, with a peak planted in the first / the last pixel of the last sample (the
    ends of a row walk: the first row of the first row group, the last row of a ragged last chunk)."""
    assert ops.X3_PLANES == 2
    S, Bs, C, H = shape
    B = S * Bs
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, H, generator=g)
    gy = torch.randn(B, C, H, H, generator=g)
    n, c = B - 1, C - 1
    h = w = 0 if where == "first" else H - 1
    x[n, c, h, w] = 60.0
    gy[n, c, h, w] = 500.0
    ga, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    ga[c] = 1.5                                                        # (the planted element is the largest |y| whatever the draw)
    xd = _dev(x, grad=True)
    y = batchnorm.batch_norm(xd, ga.to(DEV), be.to(DEV), None, None, segments=S, act="lrelu")
    (y * gy.to(DEV)).sum().backward()
    assert len(slots) == 2 and slots[0][0].data_ptr() == y.data_ptr() and slots[1][0].shape == x.shape
    _assert_tag(y, slots[0][1], slots[0][2], "y")
    _assert_tag(slots[1][0], slots[1][1], slots[1][2], "dx")
    assert torch.equal(slots[1][0], xd.grad)
    am = y.detach().abs().reshape(-1).argmax()
    assert tuple(int(v) for v in np.unravel_index(int(am), tuple(y.shape))) == (n, c, h, w)
    assert ops.amax_live(y) == (slots[0][1], slots[0][2])


@pytest.mark.gpu
def test_bn_absmax_all_zero_output_carries_the_epoch(slots):
    """gamma = 0, beta = -1, relu: y is all zeros; its slot must still hold the tag's epoch (magnitude bits 0), or the consumer
    would poison its result."""
    x = torch.randn(4, 16, 5, 5, generator=torch.Generator().manual_seed(1))
    y = batchnorm.batch_norm(_dev(x), torch.zeros(16, device=DEV), -torch.ones(16, device=DEV), None, None, segments=2, act="relu")
    assert not y.any() and len(slots) == 1
    word = _slot_word(slots[0][1])
    assert (word >> 32) == slots[0][2] and (word & 0xffffffff) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the tiny 'bn' Solver against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _buffers(s):
    return {k: v for k, v in s.dis.state_dict().items()
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


@pytest.mark.gpu
def test_tiny_bn_two_iterations_vs_reference(golden_dir):
    """dis.norm 'bn': two iterations of the tiny Solver (HostNoise, the reference's random stream) against the imported reference
    (its BN-fed convolution biases frozen: tests/golden/make_golden_bn.py): every loss scalar, every D gradient the fixture holds of
    both D steps (a frozen bias: none, or exact zeros), every BN buffer after each dis_update (four updates per layer, order fake,
    real, fake1, real) and each gen_update (two more).  Iteration-1 buffers: 16 x the deviation the reference itself shows under
    one ulp of input noise (``sens``)."""
    fx = ts.load(golden_dir, "tiny_bn_step")
    ref = fx.npz

    def check_buffers(it, s, when):
        for k, v in _buffers(s).items():
            key = "it%d/after_%s/%s" % (it, when, k)
            w = T(ref[key])
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(w) == 6 * it + (4 if when == "dis" else 6), (key, int(v), int(w))
                continue
            err = (v.detach().cpu().double() - w.double()).abs().max().item()
            lim = 1e-5 * w.abs().max().item() if it == 0 else 16 * float(ref["sens/" + key])
            print("%s: max err %.3e, limit %.3e, ratio to sens %.1f" % (key, err, lim, err / max(float(ref["sens/" + key]), 1e-30)))
            assert err <= lim, "%s: max err %.3e > %.3e" % (key, err, lim)

    ts.two_iterations(fx, _bn_config(), ts.FIXED_BOUNDS, init=False,          # (tiny_bn_init.npz holds the initial tensors themselves)
                      after_dis=lambda it, s: check_buffers(it, s, "dis"), after_gen=lambda it, s: check_buffers(it, s, "gen"))


@pytest.mark.gpu
def test_bn_penalties_stay_unbuilt():
    s = ts.build(_bn_config(), DEV)
    assert not s.dis.penalty_hip_ok()
    with pytest.raises(NotImplementedError):
        s.dis.forward_src_scale0_torch(torch.randn(2, 3, 32, 32, device=DEV))
