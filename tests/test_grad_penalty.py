"""Gradient / R1 penalties of the discriminator on the HIP kernels (hipdwc.penalty, csrc/penalty.hip).

Bounds and where they come from:
  * reduction kernels against float64: 1e-5 of each tensor's largest magnitude -- a tree sum of N <= 12 288 fp32 squares is bounded
    by about log2(N) * 2^-24 ~ 1e-6, one decade of room; two launches on the same input are bit-equal (fixed-order sums);
  * seed kernel: exact (one multiply);
  * whole operator against a float64 CPU double backward and the Solver against the reference's recorded run: the bounds of
    test_hip_parity.test_tiny_dis_penalties_vs_reference -- scalars 2e-4 relative, every gradient 2e-3 of its largest magnitude.
    The same float64 reference in float32 on the CPU stays inside them at these seeds (checked when the seeds were chosen: a
    LeakyReLU near-tie that flips a mask would be a property of the input, not of a kernel).
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import tiny_solver as ts                                    # noqa: E402
from hipdwc import _lib, host, ops, penalty, synth          # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"
MODES = ("gp", "r1")


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


# ---- 1. reduction kernels ---------------------------------------------------------------------------------------------------------
def _penalty_launch(g, mode, dout):
    lib = _lib.load()
    B, pixels, planes = g.shape
    q, k = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    out = torch.empty((), device=DEV)
    ghat = torch.empty_like(g)
    st = ops._stream()
    _lib.check(lib.dwc_grad_penalty_fwd(g.data_ptr(), q.data_ptr(), k.data_ptr(), out.data_ptr(), B, pixels, planes, 3,
                                        penalty.MODES[mode], st), "grad_penalty_fwd")
    _lib.check(lib.dwc_grad_penalty_scale(g.data_ptr(), k.data_ptr(), dout.data_ptr(), ghat.data_ptr(), B, pixels, planes, 3, st),
               "grad_penalty_scale")
    torch.cuda.synchronize()
    return out, q, k, ghat


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W", [(3, 5, 7), (2, 64, 64)])
def test_penalty_reduction_kernels_vs_float64(B, H, W, mode):
    gen = torch.Generator().manual_seed(100 * B + H)
    g = torch.randn(B, H * W, 4, generator=gen)
    if mode == "gp":
        g[B - 1] = 0.0                                 # |g| = 0: finite P, k = 0
    g[:, :, 3] = 1e30                                  # the padding plane: a kernel that reads it into a sum overflows
    dout = torch.tensor([0.75])
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
    ghat64[:, :, :3] = 0.75 * k64.view(B, 1, 1) * g64
    gd, dd = g.to(DEV), dout.to(DEV)
    first = _penalty_launch(gd, mode, dd)
    for name, got, want in zip(("P", "q", "k", "ghat"), first, (P64, q64, k64, ghat64)):
        assert torch.isfinite(got).all(), name
        err = rel_err(got, want)
        print("%s B%d %dx%d %s: rel err %.3e" % (mode, B, H, W, name, err))
        assert err <= 1e-5, (name, err)
    assert torch.equal(first[3][:, :, 3], torch.zeros_like(first[3][:, :, 3]))
    if mode == "gp":
        assert float(first[2][B - 1]) == 0.0 and float(first[1][B - 1]) == 0.0
    second = _penalty_launch(gd, mode, dd)
    for name, a, b in zip(("P", "q", "k", "ghat"), first, second):
        assert torch.equal(a, b), "%s differs between two launches" % name


# ---- 2. seed kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["lrelu", "relu", "none"])
@pytest.mark.parametrize("rows,C", [(5, 8), (64, 512)])
def test_src_head_seed_exact(rows, C, act):
    gen = torch.Generator().manual_seed(rows + C)
    a = torch.randn(rows, C, generator=gen)
    a[0, :4] = 0.0                                     # act'(0): the slope side, as dwc_act_bwd_bias reads it
    w = torch.randn(C, generator=gen)
    slope = {"lrelu": 0.1, "relu": 0.0, "none": 1.0}[act]
    want = w.view(1, C) * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    ad, wd = a.to(DEV), w.to(DEV)
    d = torch.empty_like(ad)
    _lib.check(_lib.load().dwc_src_head_seed(ad.data_ptr(), wd.data_ptr(), d.data_ptr(), rows, C, ops.ACT[act], ops._stream()),
               "src_head_seed")
    assert torch.equal(d.cpu(), want)


# ---- 3. the whole operator against a float64 CPU double backward --------------------------------------------------------------------
def _make_dis(n_layer, dim, size, seed):
    from networks.networks import MsImageDis
    params = dict(synth.make_config(image_size=size, tiny=True)["dis"], n_layer=n_layer, dim=dim, num_scales=1, norm="none",
                  activ="lrelu", pad_type="reflect")
    torch.manual_seed(seed)
    dis = MsImageDis(3, params)
    dis.apply(host.weights_init("gaussian"))
    with torch.no_grad():
        for blk in dis.cnns_feat[0]:
            blk.conv.bias.normal_(0.0, 0.05)
    return dis


def reference_penalties(dis, x, dtype):
    """Both penalties and their gradients w.r.t. every parameter of scale 0 on stock torch CPU ops, as the reference takes them."""
    blocks = list(dis.cnns_feat[0])
    params = []
    for i, blk in enumerate(blocks):
        params += [("w%d" % i, blk.conv.weight), ("b%d" % i, blk.conv.bias)]
    params += [("w_src", dis.cnns_src[0].weight), ("b_src", dis.cnns_src[0].bias)]
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params}
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    h = xr
    for i in range(len(blocks)):
        h = F.leaky_relu(F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), p["w%d" % i], p["b%d" % i], stride=2), 0.1)
    y = F.conv2d(h, p["w_src"], p["b_src"])
    g = torch.autograd.grad(y, xr, torch.ones_like(y), create_graph=True)[0].reshape(x.size(0), -1)
    q = (g ** 2).sum(1)
    out = {}
    for mode, P in (("gp", ((q.sqrt() - 1) ** 2).mean()), ("r1", (q ** 2).mean())):
        grads = torch.autograd.grad(P, list(p.values()), retain_graph=True, allow_unused=True)
        out[mode] = (P.detach(), dict(zip(p.keys(), grads)))
    return out


OPERATOR_SHAPES = [(2, 8, 16, 3), (4, 64, 32, 2), (4, 64, 128, 4)]       # (n_layer, dim, image size, batch)


@functools.lru_cache(maxsize=None)
def _operator_case(n_layer, dim, size, B):
    dis = _make_dis(n_layer, dim, size, seed=7 + n_layer + size)
    x = torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(size + B))
    return dis, x, reference_penalties(dis, x, torch.float64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", OPERATOR_SHAPES, ids=lambda s: "L%d-d%d-s%d-B%d" % s)
def test_src_grad_penalty_vs_float64_double_backward(shape, mode):
    dis, x, ref = _operator_case(*shape)
    want_P, want_g = ref[mode]
    dis = dis.to(DEV)
    try:
        for prm in dis.parameters():
            prm.grad = None
        P = dis.src_grad_penalty(x.to(DEV), mode)
        P.backward()
        torch.cuda.synchronize()
        got, want = float(P), float(want_P)
        print("%s %s: P %.8e want %.8e" % (shape, mode, got, want))
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)
        blocks = list(dis.cnns_feat[0])
        for i, blk in enumerate(blocks):
            err = rel_err(blk.conv.weight.grad, want_g["w%d" % i])
            print("  dW%d rel err %.3e" % (i, err))
            assert err <= 2e-3, (i, err)
            assert blk.conv.bias.grad is None or not blk.conv.bias.grad.any()
        err = rel_err(dis.cnns_src[0].weight.grad, want_g["w_src"])
        print("  dw_src rel err %.3e" % err)
        assert err <= 2e-3, err
        assert dis.cnns_src[0].bias.grad is None or not dis.cnns_src[0].bias.grad.any()
        for k in want_g:                                 # the reference agrees: no gradient reaches a bias
            if k.startswith("b"):
                assert want_g[k] is None or not want_g[k].any()
    finally:
        dis.cpu()


# ---- 4-6. Solver level -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_step.npz"))


@pytest.fixture(scope="module")
def fixture_penalties(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_penalties.npz"))


def _config(norm=None, **top):
    cfg = synth.make_config(image_size=32, tiny=True)
    if norm is not None:
        cfg["dis"]["norm"] = norm
    return dict(cfg, **top)


def _dis_step(s, tiny, cfg, iters=15):
    s.dis_update(*ts.step_args(ts.batch_of(tiny, DEV), cfg, iters))
    torch.cuda.synchronize()


def _conv2d_forbidden(*a, **k):
    raise AssertionError("torch.nn.functional.conv2d called inside dis_update with ops.PENALTY_HIP on")


@pytest.mark.parametrize("hip", [True, False], ids=["hip", "torch"])
def test_tiny_dis_penalties_vs_reference_by_branch(tiny, fixture_penalties, hip, monkeypatch):
    """gp_w = 10, use_r1 = True, iteration 15 against the reference's recorded run: on the HIP branch (no F.conv2d may run) and on
    the torch branch."""
    ref = fixture_penalties
    monkeypatch.setattr(ops, "PENALTY_HIP", 1 if hip else 0)
    with ts.host_noise():
        s = ts.build(_config(), DEV)
        assert torch.equal(torch.get_rng_state(), T(tiny["rng_state_after_init"]))
        grabbed = ts.grab_dis(s)
        if hip:
            assert s.dis.penalty_hip_ok()
            monkeypatch.setattr(F, "conv2d", _conv2d_forbidden)
        _dis_step(s, tiny, _config(gp_w=10.0, use_r1=True))
        monkeypatch.undo()
        for k in ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1"):
            got, want = float(getattr(s, k)), float(ref[k])
            print("%s: %.8e want %.8e" % (k, got, want))
            assert abs(got - want) <= 2e-4 * max(abs(want), 1e-12) + (2e-4 if k != "loss_r1" else 0.0), (k, got, want)
        assert set(grabbed) == {n for n, _ in s.dis.named_parameters()}
        for k, g in grabbed.items():
            assert g is not None, k
            err = rel_err(g, T(ref["grad/" + k]))
            print("grad %s: rel err %.3e" % (k, err))
            assert err <= 2e-3, (k, err)


def test_r1_penalty_is_fp32_under_bf16(tiny, fixture_penalties, monkeypatch):
    """loss_r1 depends only on x_real and D's fp32 parameters: the branch runs the fp32 entry points under bf16 activations too."""
    monkeypatch.setattr(ops, "PENALTY_HIP", 1)
    with ts.host_noise(), ts.precision("bf16"):
        s = ts.build(_config(), DEV)
        monkeypatch.setattr(F, "conv2d", _conv2d_forbidden)
        _dis_step(s, tiny, _config(gp_w=0.0, use_r1=True))
        monkeypatch.undo()
        got, want = float(s.loss_r1), float(fixture_penalties["loss_r1"])
        print("loss_r1 (bf16 mode): %.8e want %.8e" % (got, want))
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)


def test_spectral_norm_keeps_the_torch_branch(tiny, monkeypatch):
    """dis.norm 'sn' is outside the closed form: with the switch on, both penalties still run, on forward_src_scale0_torch."""
    monkeypatch.setattr(ops, "PENALTY_HIP", 1)
    calls = []
    real = F.conv2d

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    s = ts.build(_config("sn"), DEV)
    assert not s.dis.penalty_hip_ok()
    monkeypatch.setattr(F, "conv2d", counting)
    _dis_step(s, tiny, _config("sn", gp_w=10.0, use_r1=True))
    monkeypatch.undo()
    assert calls, "the torch branch did not run"
    for k in ("loss_gp", "loss_r1", "loss_dis_all"):
        assert np.isfinite(float(getattr(s, k))), k
