"""Gradient / R1 penalties through ``dis.norm: in / ln`` on the HIP kernels (hipdwc.normjvp, csrc/norm_tangent.hip).

Bounds are those of tests/test_grad_penalty.py: P to 2e-4 relative, every gradient to 2e-3 of its largest magnitude, against
  * a float64 CPU double backward of the chain restated below (the whole operator), and
  * the reference's recorded run (tests/golden/tiny_penalties_ln.npz / _in.npz, recipe tests/golden/make_golden_gp_norm.py; the
    Solver, on both branches).  Keys whose true value is zero -- the convolution biases in front of an instance norm -- are held to
    2e-3 of their layer's weight gradient where the branch computes rounding noise for them, and are None or exactly zero on the HIP
    branch.
At the seeds used here the same float64 reference in float32 on the CPU, through the real module (forward_src_scale0_torch), stays
inside these bounds (test_torch_branch_float32_inside_the_bounds asserts it on the shapes a CPU affords: a LeakyReLU near-tie that
flips a mask would be a property of the input, not of a kernel).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tiny_solver as ts
from hipdwc import host, ops, synth          # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"
MODES = ("gp", "r1")
NORMS = ("ln", "in")


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


# ---- the whole operator against a float64 CPU double backward ------------------------------------------------------------------------
def _make_dis(norm, n_layer, dim, size, seed):
    from networks.networks import MsImageDis
    params = dict(synth.make_config(image_size=size, tiny=True)["dis"], n_layer=n_layer, dim=dim, num_scales=1, norm=norm,
                  activ="lrelu", pad_type="reflect")
    torch.manual_seed(seed)
    dis = MsImageDis(3, params)
    dis.apply(host.weights_init("gaussian"))
    with torch.no_grad():
        for blk in dis.cnns_feat[0]:
            blk.conv.bias.normal_(0.0, 0.05)
            if blk.norm_kind == "ln":
                blk.norm.gamma.uniform_(0.5, 1.5)
                blk.norm.beta.normal_(0.0, 0.1)
    return dis


def _named(dis):
    out = []
    for i, blk in enumerate(dis.cnns_feat[0]):
        out += [("w%d" % i, blk.conv.weight), ("b%d" % i, blk.conv.bias)]
        if blk.norm_kind == "ln":
            out += [("gamma%d" % i, blk.norm.gamma), ("beta%d" % i, blk.norm.beta)]
    return out + [("w_src", dis.cnns_src[0].weight), ("b_src", dis.cnns_src[0].bias)]


def _true_zero(dis):
    """Parameters on which neither penalty depends: a bias in front of an instance norm, the src head's bias."""
    return {"b%d" % i for i, blk in enumerate(dis.cnns_feat[0]) if blk.norm_kind == "in"} | {"b_src"}


def reference_penalties(dis, x, dtype):
    """Both penalties and their gradients w.r.t. every parameter of scale 0 on stock torch CPU ops, as the reference takes them."""
    p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in _named(dis)}
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    h = xr
    for i, blk in enumerate(dis.cnns_feat[0]):
        h = F.conv2d(F.pad(h, (1, 1, 1, 1), mode="reflect"), p["w%d" % i], p["b%d" % i], stride=2)
        if blk.norm_kind == "in":
            c = h - h.mean((2, 3), keepdim=True)
            h = c / ((c * c).mean((2, 3), keepdim=True) + blk.norm.eps).sqrt()
        elif blk.norm_kind == "ln":
            c = h - h.mean((1, 2, 3), keepdim=True)
            s = ((c * c).sum((1, 2, 3), keepdim=True) / (c[0].numel() - 1)).sqrt()
            h = c / (s + blk.norm.eps) * p["gamma%d" % i].reshape(1, -1, 1, 1) + p["beta%d" % i].reshape(1, -1, 1, 1)
        h = F.leaky_relu(h, 0.1)
    y = F.conv2d(h, p["w_src"], p["b_src"])
    g = torch.autograd.grad(y, xr, torch.ones_like(y), create_graph=True)[0].reshape(x.size(0), -1)
    q = (g ** 2).sum(1)
    out = {}
    for mode, P in (("gp", ((q.sqrt() - 1) ** 2).mean()), ("r1", (q ** 2).mean())):
        grads = torch.autograd.grad(P, list(p.values()), retain_graph=True, allow_unused=True)
        out[mode] = (P.detach(), dict(zip(p.keys(), grads)))
    return out


OPERATOR_SHAPES = [(2, 8, 16, 3), (3, 8, 32, 3), (4, 64, 64, 2)]       # (n_layer, dim, image size, batch)


@functools.lru_cache(maxsize=None)
def _operator_case(norm, n_layer, dim, size, B):
    dis = _make_dis(norm, n_layer, dim, size, seed=11 + n_layer + size)
    x = torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(size + B))
    return dis, x, reference_penalties(dis, x, torch.float64)


def _check_grads(got, want_g, zero_keys, label):
    """``got``: name -> gradient or None.  Inside 2e-3 of the reference's largest magnitude; None or exactly zero where the true
    value is zero (and where the reference's own gradient is identically zero: the last layer's beta, act'' = 0)."""
    for k, want in want_g.items():
        g = got[k]
        if k in zero_keys or want is None or not want.any():
            assert g is None or not g.any(), (label, k)
            continue
        assert g is not None, (label, k)
        err = rel_err(g, want)
        print("  %s d%s rel err %.3e" % (label, k, err))
        assert err <= 2e-3, (label, k, err)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", OPERATOR_SHAPES, ids=lambda s: "L%d-d%d-s%d-B%d" % s)
@pytest.mark.parametrize("norm", NORMS)
def test_src_grad_penalty_norm_vs_float64_double_backward(norm, shape, mode):
    dis, x, ref = _operator_case(norm, *shape)
    want_P, want_g = ref[mode]
    dis = dis.to(DEV)
    try:
        assert dis.penalty_hip_ok()
        for prm in dis.parameters():
            prm.grad = None
        P = dis.src_grad_penalty(x.to(DEV), mode)
        P.backward()
        torch.cuda.synchronize()
        got, want = float(P), float(want_P)
        print("%s %s %s: P %.8e want %.8e" % (norm, shape, mode, got, want))
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)
        _check_grads({k: v.grad for k, v in _named(dis)}, want_g, _true_zero(dis), "%s %s" % (norm, mode))
    finally:
        dis.cpu()


@pytest.mark.parametrize("shape", OPERATOR_SHAPES[:2], ids=lambda s: "L%d-d%d-s%d-B%d" % s)
@pytest.mark.parametrize("norm", NORMS)
def test_torch_branch_float32_inside_the_bounds(norm, shape):
    """The A/B partner on the CPU: the double backward of forward_src_scale0_torch in float32 against the float64 restatement."""
    dis, x, ref = _operator_case(norm, *shape)
    for mode in MODES:
        want_P, want_g = ref[mode]
        xr = x.clone().requires_grad_(True)
        y = dis.forward_src_scale0_torch(xr)
        g = torch.autograd.grad(y, xr, torch.ones_like(y), create_graph=True)[0].reshape(x.size(0), -1)
        q = (g ** 2).sum(1)
        P = ((q.sqrt() - 1) ** 2).mean() if mode == "gp" else (q ** 2).mean()
        named = _named(dis)
        grads = torch.autograd.grad(P, [v for _, v in named], allow_unused=True)
        got_P = float(P.detach())
        assert abs(got_P - float(want_P)) <= 2e-4 * abs(float(want_P)) / 4, (norm, mode, got_P, float(want_P))
        for (k, _), gr in zip(named, grads):
            want = want_g[k]
            if k in _true_zero(dis) or want is None or not want.any():
                # (rounding noise in front of an instance norm: held to the layer's weight gradient; anything else is exactly zero)
                lim = 2e-3 * want_g["w" + k[1:]].abs().max().item() if k in _true_zero(dis) and k != "b_src" else 0.0
                assert gr is None or gr.abs().max().item() <= lim / 4, (norm, mode, k)
                continue
            err = rel_err(gr, want)
            assert err <= 2e-3 / 4, (norm, mode, k, err)


# ---- Solver level: the reference's recorded run ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(golden_dir, norm):
    ref = np.load(os.path.join(golden_dir, "tiny_penalties_%s.npz" % norm))
    meta = json.loads(bytes(ref["meta"]).decode())
    sens = json.loads(bytes(ref["sens_json"]).decode())
    assert meta["norm"] == norm and meta["gp_w"] == 10.0 and meta["use_r1"] and meta["iters"] == 15
    return ref, meta, sens


def _limit(ref, k, norm):
    """The absolute bound on fixture key k: 2e-4 relative for a scalar, 2e-3 of the largest magnitude for a gradient -- of the layer's
    weight gradient for a bias in front of an instance norm (true value zero)."""
    if not k.startswith("grad/"):
        return 2e-4 * abs(float(ref[k]))
    if norm == "in" and k.endswith(".conv.bias") and k.split(".")[-3] != "0":
        return 2e-3 * float(np.abs(ref[k[:-4] + "weight"]).max())
    return 2e-3 * float(np.abs(ref[k]).max())


def test_fixture_sensitivities_below_a_quarter_of_the_bounds(golden_dir):
    for norm in NORMS:
        ref, meta, sens = _fixture(golden_dir, norm)
        assert set(sens) == {k for k in ref.files if k.startswith("grad/") or k.startswith("loss_")}
        for k, v in sens.items():
            assert v <= 0.25 * _limit(ref, k, norm), (norm, k, v)


@pytest.mark.parametrize("norm", NORMS)
def test_forward_src_scale0_torch_matches_the_recorded_penalties(golden_dir, norm):
    """Without a GPU: both penalties of the reference's recorded run from forward_src_scale0_torch on the CPU -- loss_r1 at x_real,
    loss_gp at the recorded ``x_hat`` (the recording's random stream and generator produced it)."""
    from networks.networks import MsImageDis
    ref, meta, _ = _fixture(golden_dir, norm)
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = norm
    torch.manual_seed(meta["seed"])
    from solver import Solver
    s = Solver(cfg, torch.device("cpu"), None)
    assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
    assert isinstance(s.dis, MsImageDis)
    x = synth.make_batch(meta["B"], meta["S"], seed=meta["batch_seed"])["x_real"][:, :3].float().requires_grad_(True)
    y = s.dis.forward_src_scale0_torch(x)
    got = float(s.r1_penalty(y, x)) * 10. / 2
    want = float(ref["loss_r1"])
    assert abs(got - want) <= 2e-4 * abs(want), (got, want)
    x_hat = T(ref["x_hat"]).clone().requires_grad_(True)
    got_gp = float(s.gradient_penalty(s.dis.forward_src_scale0_torch(x_hat), x_hat)) * meta["gp_w"]
    want_gp = float(ref["loss_gp"])
    assert abs(got_gp - want_gp) <= 2e-4 * abs(want_gp), (got_gp, want_gp)


def _config(norm, gan_type=None, **top):
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = norm
    if gan_type is not None:
        cfg["dis"]["gan_type"] = gan_type
    return dict(cfg, **top)


def _batch(meta):
    return {k: v.to(DEV) for k, v in synth.make_batch(meta["B"], meta["S"], seed=meta["batch_seed"]).items()}


_REAL_CONV2D = F.conv2d


def _conv2d_forbidden(*a, **k):
    raise AssertionError("torch.nn.functional.conv2d called inside dis_update with ops.PENALTY_HIP on")


@pytest.mark.gpu
@pytest.mark.parametrize("hip", [True, False], ids=["hip", "torch"])
@pytest.mark.parametrize("norm", NORMS)
def test_tiny_dis_penalties_norm_vs_reference_by_branch(golden_dir, norm, hip, monkeypatch):
    """gp_w = 10, use_r1 = True, iteration 15 against the reference's recorded run: on the HIP branch (no F.conv2d may run) and on
    the torch branch."""
    ref, meta, _ = _fixture(golden_dir, norm)
    monkeypatch.setattr(ops, "PENALTY_HIP", 1 if hip else 0)
    with ts.host_noise():
        s = ts.build(_config(norm), DEV, seed=meta["seed"])
        batch = _batch(meta)
        assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
        grabbed = ts.grab_dis(s)
        if hip:
            assert s.dis.penalty_hip_ok()
            monkeypatch.setattr(F, "conv2d", _conv2d_forbidden)
        s.dis_update(*ts.step_args(batch, _config(norm, gp_w=10.0, use_r1=True), meta["iters"]))
        torch.cuda.synchronize()
        monkeypatch.undo()
        for k in ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1"):
            got, want = float(getattr(s, k)), float(ref[k])
            print("%s %s: %.8e want %.8e" % (norm, k, got, want))
            assert abs(got - want) <= _limit(ref, k, norm), (k, got, want)
        assert set(grabbed) == {n for n, _ in s.dis.named_parameters()} == {k[5:] for k in ref.files if k.startswith("grad/")}
        for k, g in grabbed.items():
            want = T(ref["grad/" + k])
            zero = norm == "in" and k.endswith(".conv.bias") and k.split(".")[-3] != "0"
            if g is None:
                assert zero, k                               # (flagged: no gradient tensor for an identically-zero gradient)
                continue
            err = (g.detach().cpu().double() - want.double()).abs().max().item()
            lim = _limit(ref, "grad/" + k, norm)
            print("grad %s: max err %.3e, limit %.3e" % (k, err, lim))
            assert err <= lim, (k, err, lim)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_r1_penalty_norm_is_fp32_under_bf16(golden_dir, norm, monkeypatch):
    """loss_r1 depends only on x_real and D's fp32 parameters: the branch runs the fp32 entry points under bf16 activations too."""
    ref, meta, _ = _fixture(golden_dir, norm)
    monkeypatch.setattr(ops, "PENALTY_HIP", 1)
    with ts.host_noise(), ts.precision("bf16"):
        s = ts.build(_config(norm), DEV, seed=meta["seed"])
        monkeypatch.setattr(F, "conv2d", _conv2d_forbidden)
        s.dis_update(*ts.step_args(_batch(meta), _config(norm, gp_w=0.0, use_r1=True), meta["iters"]))
        torch.cuda.synchronize()
        monkeypatch.undo()
        got, want = float(s.loss_r1), float(ref["loss_r1"])
        print("%s loss_r1 (bf16 mode): %.8e want %.8e" % (norm, got, want))
        assert abs(got - want) <= 2e-4 * abs(want), (got, want)


def _wgan_ln_two_iterations(hip, monkeypatch):
    monkeypatch.setattr(ops, "PENALTY_HIP", 1 if hip else 0)
    with ts.host_noise():
        s = ts.build(_config("ln", gan_type="wgan"), DEV)
        batch = _batch({"B": 3, "S": 32, "batch_seed": 4321})
        cfg = _config("ln", gan_type="wgan", gp_w=10.0)
        # (the wgan objective does not depend on a constant added to src: the true gradient of the src heads' biases is zero, what is
        # computed for them is rounding noise, and Adam turns the SIGN of that noise into a step of lr -- frozen, as in
        # tests/golden/make_golden_gan.py and tests/test_gan_solver.py)
        for conv in s.dis.cnns_src:
            conv.bias.requires_grad_(False)
        assert s.dis.penalty_hip_ok()
        grabbed = ts.grab_dis(s)
        out = []
        for it in range(2):
            if hip:
                monkeypatch.setattr(F, "conv2d", _conv2d_forbidden)
            s.dis_update(*ts.step_args(batch, cfg, it))
            if hip:
                monkeypatch.setattr(F, "conv2d", _REAL_CONV2D)
            s.gen_update(*ts.step_args(batch, cfg, it))
            s.smooth_moving()
            s.update_learning_rate()
            s.update_attention_status(it)
            torch.cuda.synchronize()
            losses = ts.read_losses(s, ("loss_dis", "loss_dis_all", "loss_gp", "loss_gen_adv", "loss_gen_total"))
            out.append((losses, {k: (None if g is None else g.cpu()) for k, g in grabbed.items()}))
        return out


@pytest.mark.gpu
def test_wgan_gp_with_layer_norm_two_iterations_hip_against_torch_branch(monkeypatch):
    """``gan_type: wgan``, ``norm: ln``, ``gp_w: 10`` -- WGAN-GP as people configure it: two iterations, every loss finite, and the HIP
    branch (no F.conv2d inside dis_update) agrees with the torch branch within the bounds above."""
    hip = _wgan_ln_two_iterations(True, monkeypatch)
    tor = _wgan_ln_two_iterations(False, monkeypatch)
    for it in range(2):
        for k, want in tor[it][0].items():
            got = hip[it][0][k]
            print("it%d %s: hip %.8e torch %.8e" % (it, k, got, want))
            assert np.isfinite(got) and np.isfinite(want), (it, k)
            assert abs(got - want) <= 2e-4 * abs(want), (it, k, got, want)
        assert set(hip[it][1]) == set(tor[it][1])
        for k, want in tor[it][1].items():
            got = hip[it][1][k]
            assert (got is None) == (want is None), (it, k)
            if want is None:
                continue
            err = rel_err(got, want)
            print("it%d grad %s: rel err %.3e" % (it, k, err))
            assert err <= 2e-3, (it, k, err)
