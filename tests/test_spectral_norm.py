"""Spectral normalisation, Conv2dBlock(norm='sn') / dis.norm 'sn' (reference networks.py:754-816) on csrc/spectral_norm.hip.

CPU: construction equals the reference's (keys, shapes, values, random stream), u / v stay out of the optimiser, a reference SN
state_dict loads strictly.  GPU: the multi-tensor power iteration against a float64 restatement, bit-identical run to run; the SN
block against the imported reference (fixtures: tests/golden/make_golden_sn.py), fp32 and bf16, one segmented call = S calls; the
tiny SN Solver over two iterations and a penalised D step against the reference."""
import copy
import os

import numpy as np
import pytest
import torch

import tiny_solver as ts
from hipdwc import ops, synth

T = torch.from_numpy
DEV = "cuda:0"
BF = torch.bfloat16

# (name, B, Cin, Cout, H, k, stride, pad, activation) -- tests/golden/make_golden_sn.py SN_CASES
SN_CASES = [
    ("k4s2_lrelu", 2, 16, 32, 16, 4, 2, 1, "lrelu"),
    ("k3s1_tanh", 2, 8, 16, 12, 3, 1, 1, "tanh"),
    ("k4s2_c14_sigmoid", 3, 8, 14, 8, 4, 2, 1, "sigmoid"),
    ("k3s1_c6_none", 2, 16, 6, 10, 3, 1, 1, "none"),
]


def _sn_config():
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = "sn"
    return cfg


def close(a, b, rel, atol=1e-6, msg=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = rel * b.abs().max().item() + atol
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tiny_sn_init_equals_reference(golden_dir):
    ref = np.load(os.path.join(golden_dir, "tiny_sn_init.npz"))
    s = ts.build(_sn_config())
    for prefix, mod in (("init/gen/", s.gen), ("init/dis/", s.dis)):
        sd = mod.state_dict()
        want = {k[len(prefix):]: ref[k] for k in ref.files if k.startswith(prefix)}
        assert list(sd.keys()) == list(want.keys())
        for k, v in want.items():
            assert sd[k].shape == v.shape, k
            assert torch.equal(sd[k], T(v)), k          # same seed, same draw order: bit-exact
    assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
    sd = s.dis.state_dict()
    assert "cnns_feat.0.1.conv.module.weight_bar" in sd and "cnns_feat.0.1.conv.module.weight_u" in sd
    assert "cnns_feat.0.0.conv.weight" in sd                           # the first layer has no norm, as in the reference
    # u / v: Parameters without gradient, in the state_dict, NOT in the optimiser (reference solver.py:64-67)
    uv = [p for n, p in s.dis.named_parameters() if n.endswith("weight_u") or n.endswith("weight_v")]
    assert len(uv) == 2 * 2 * 2 and not any(p.requires_grad for p in uv)
    in_opt = {id(p) for p in s.dis_opt.param_groups[0]["params"]}
    assert not any(id(p) in in_opt for p in uv)
    assert all(id(p) in in_opt for n, p in s.dis.named_parameters() if n.endswith("weight_bar"))
    # a reference SN checkpoint loads strictly
    fresh = ts.build(_sn_config())
    fresh.dis.load_state_dict({k[len("init/dis/"):]: T(ref[k]) for k in ref.files if k.startswith("init/dis/")}, strict=True)


def test_sn_linear_block_stays_unbuilt():
    import networks.networks as nets
    with pytest.raises(NotImplementedError):
        nets.LinearBlock(8, 8, norm="sn")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: power iteration
# ---------------------------------------------------------------------------------------------------------------------------------
class _SNParams(torch.nn.Module):
    def __init__(self, cout, k, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.weight_bar = torch.nn.Parameter(torch.randn(cout, k, generator=g) * 0.05)
        u, v = torch.randn(cout, generator=g), torch.randn(k, generator=g)
        self.weight_u = torch.nn.Parameter(u / u.norm(), requires_grad=False)
        self.weight_v = torch.nn.Parameter(v / v.norm(), requires_grad=False)


def _power64(w, u, S):
    w, u = w.double(), u.double()
    out = []
    for _ in range(S):
        t = w.t().mv(u)
        v = t / (t.norm() + 1e-12)
        x = w.mv(v)
        u = x / (x.norm() + 1e-12)
        out.append((u, v, float(u.dot(x))))
    return out


@pytest.mark.gpu
def test_sn_power_iteration_vs_float64_and_deterministic():
    from hipdwc import spectral
    shapes = [(128, 1024), (512, 8192), (37, 100), (12, 27), (256, 2048), (5, 4096)]
    for S in (1, 2, 3, 4):
        mods = [_SNParams(c, k, 10 * S + i).to(DEV) for i, (c, k) in enumerate(shapes)]
        u0 = [m.weight_u.detach().cpu().clone() for m in mods]
        runs = []
        for rep in range(2):
            for m, u in zip(mods, u0):
                m.weight_u.data.copy_(u)
            run = spectral.sn_power_iteration(mods, S)
            runs.append([tuple(t.cpu().clone() for t in run.layer(m)) + (m.weight_u.detach().cpu().clone(),
                                                                        m.weight_v.detach().cpu().clone()) for m in mods])
        for (c, k), m, u, got, again in zip(shapes, mods, u0, runs[0], runs[1]):
            for a, b in zip(got, again):
                assert torch.equal(a, b), ("not bit-identical run to run", c, k, S)
            U, V, R, u_last, v_last = got
            want = _power64(m.weight_bar.detach().cpu(), u, S)
            for s, (uw, vw, sigma) in enumerate(want):
                assert (U[s].double() - uw).abs().max() <= 1e-5, (c, k, S, s, "u")
                assert (V[s].double() - vw).abs().max() <= 1e-5, (c, k, S, s, "v")
                assert abs(1.0 / float(R[s]) - sigma) <= 1e-5 * abs(sigma), (c, k, S, s, "sigma")
            assert torch.equal(u_last, U[S - 1]) and torch.equal(v_last, V[S - 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the block against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _block(case, gold):
    import networks.networks as nets
    name, B, ci, co, H, k, s_, p, act = case
    gg = lambda key: T(gold["%s/%s" % (name, key)])
    blk = nets.Conv2dBlock(ci, co, k, s_, p, norm="sn", activation=act, pad_type="reflect").to(DEV)
    m = blk.conv.module
    with torch.no_grad():
        m.weight_bar.copy_(gg("w"))
        m.bias.copy_(gg("b"))
        m.weight_u.copy_(gg("u0"))
        m.weight_v.copy_(gg("v0"))
    return blk, gg


@pytest.mark.gpu
@pytest.mark.parametrize("case", SN_CASES, ids=lambda c: c[0])
def test_sn_block_fp32_vs_reference(golden_dir, case):
    """Three consecutive calls of the reference's block vs ONE segmented call (S = 3) on cat([x] * 3): y of the first and the
    third call, u / v after the three, dx / dW_bar / db of the sum (tolerances of test_conv_block_beyond_shipped_configs_vs_reference)."""
    gold = np.load(os.path.join(golden_dir, "sn_ops.npz"))
    name, B = case[0], case[1]
    blk, gg = _block(case, gold)
    x = gg("x").to(DEV).requires_grad_(True)
    y = blk(torch.cat([x] * 3), segments=3)
    m = blk.conv.module
    close(y[:B], gg("y1"), rel=5e-5, atol=2e-6, msg=name + " y1")
    close(y[2 * B:], gg("y3"), rel=5e-5, atol=2e-6, msg=name + " y3")
    close(m.weight_u, gg("u3"), rel=0, atol=1e-5, msg=name + " u")
    close(m.weight_v, gg("v3"), rel=0, atol=1e-5, msg=name + " v")
    (y * torch.cat([gg("gy")] * 3).to(DEV)).sum().backward()
    close(x.grad, gg("dx"), rel=3e-4, atol=2e-6, msg=name + " dx")
    close(m.weight_bar.grad, gg("dw"), rel=3e-4, atol=2e-6, msg=name + " dw")
    close(m.bias.grad, gg("db"), rel=3e-4, atol=2e-6, msg=name + " db")
    # one call = one iteration (the reference module's call)
    blk1, _ = _block(case, gold)
    y1 = blk1(x.detach())
    close(y1, gg("y1"), rel=5e-5, atol=2e-6, msg=name + " single call")
    close(blk1.conv.module.weight_u, gg("u1"), rel=0, atol=1e-5, msg=name + " u after one call")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SN_CASES, ids=lambda c: c[0])
def test_sn_block_segmented_equals_single_calls(golden_dir, case):
    """One segmented call (S = 3) equals three single-segment calls on a copy of the block, gradients included."""
    gold = np.load(os.path.join(golden_dir, "sn_ops.npz"))
    name, B = case[0], case[1]
    blk, gg = _block(case, gold)
    twin = copy.deepcopy(blk)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(gg("x").shape, generator=g).to(DEV).requires_grad_(True) for _ in range(3)]
    gys = [torch.randn(gg("gy").shape, generator=g).to(DEV) for _ in range(3)]
    y = blk(torch.cat(xs), segments=3)
    (y * torch.cat(gys)).sum().backward()
    xt = [t.detach().clone().requires_grad_(True) for t in xs]
    yt = [twin(t) for t in xt]
    sum((a * b).sum() for a, b in zip(yt, gys)).backward()
    for j in range(3):
        close(y[j * B:(j + 1) * B], yt[j], rel=2e-6, atol=1e-7, msg="%s y%d" % (name, j))
        close(xs[j].grad, xt[j].grad, rel=2e-5, atol=1e-7, msg="%s dx%d" % (name, j))
    mb, mt = blk.conv.module, twin.conv.module
    assert torch.equal(mb.weight_u, mt.weight_u) and torch.equal(mb.weight_v, mt.weight_v)
    close(mb.weight_bar.grad, mt.weight_bar.grad, rel=2e-5, atol=1e-7, msg=name + " dw")
    close(mb.bias.grad, mt.bias.grad, rel=2e-5, atol=1e-7, msg=name + " db")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SN_CASES, ids=lambda c: c[0])
def test_sn_block_bf16(golden_dir, case):
    """bf16 activations: the segmented block against a torch restatement fed the operands the kernels multiply (bf16 x and W_bar,
    the fp32 sigma of the fixture's iterations), at the tolerances of test_bf16_conv_forward_backward for a convolution behind an
    activation: dZ = g * r_s is a product rounded to bf16 before the data / weight gradients, like g behind a fused activation."""
    gold = np.load(os.path.join(golden_dir, "sn_ops.npz"))
    name, B, ci, co, H, k, s_, p, act = case
    ops.set_precision("bf16")
    try:
        blk, gg = _block(case, gold)
        x = gg("x").to(BF).float()
        wr = gg("w").clone().requires_grad_(True)
        br = gg("b").clone().requires_grad_(True)
        xr = x.clone().requires_grad_(True)
        u3, v3 = gg("u3"), gg("v3")
        ys = []
        for j in range(3):
            uj, vj = gg("u%d" % (j + 1)), gg("v%d" % (j + 1))
            sigma = float(uj.double().dot(wr.detach().double().reshape(co, -1).mv(vj.double())))
            # forward value with this call's sigma; gradient through sigma with the last pair (hipdwc.spectral docstring)
            sig = sigma + (torch.dot(u3, wr.reshape(co, -1).mv(v3)) - torch.dot(u3, wr.reshape(co, -1).mv(v3)).detach())
            wq = wr.detach().to(BF).float() + (wr - wr.detach())
            z = torch.nn.functional.conv2d(torch.nn.functional.pad(xr, (p,) * 4, mode="reflect"), wq / sig, br, stride=s_)
            ys.append({"lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.1), "tanh": torch.tanh, "sigmoid": torch.sigmoid,
                       "relu": torch.relu, "none": lambda t: t}[act](z))
        gy = gg("gy").to(BF).float()
        sum((yy * gy).sum() for yy in ys).backward()
        xd = x.to(DEV).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        yd = blk(torch.cat([xd] * 3), segments=3)
        assert yd.dtype == BF
        close(yd[:B], ys[0], 6e-3, msg=name + " y1")
        close(yd[2 * B:], ys[2], 6e-3, msg=name + " y3")
        (yd.float() * torch.cat([gy] * 3).to(DEV)).sum().backward()
        m = blk.conv.module
        close(xd.grad, xr.grad, 1.5e-2, msg=name + " dx")
        close(m.weight_bar.grad, wr.grad, 1e-2, msg=name + " dw")
        close(m.bias.grad, br.grad, 1e-2, msg=name + " db")
    finally:
        ops.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the tiny SN Solver against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def _uv(s):
    return {k: v for k, v in s.dis.state_dict().items() if k.endswith("weight_u") or k.endswith("weight_v")}


@pytest.mark.gpu
def test_tiny_sn_two_iterations_vs_reference(golden_dir):
    """dis.norm 'sn': two iterations of the tiny Solver (HostNoise, the reference's random stream) against the imported reference:
    every loss scalar, every D gradient of both D steps (exactly the recorded parameters have one), every u / v after each
    dis_update (4 iterations per SN layer) and each gen_update (2 more).  A wrong iteration count per step moves u / v by far more
    than the tolerance."""
    fx = ts.load(golden_dir, "tiny_sn_step")

    def check_uv(it, s, when, atol):
        for k, v in _uv(s).items():
            close(v, T(fx.npz["it%d/after_%s/%s" % (it, when, k)]), rel=0, atol=atol, msg="it%d after_%s %s" % (it, when, k))

    ts.two_iterations(fx, _sn_config(), ts.FIXED_BOUNDS._replace(frozen="rest"), init=False,      # (tiny_sn_init.npz holds the tensors)
                      # (after iteration 0 Adam's sign steps may flip near-zero entries of W_bar)
                      after_dis=lambda it, s: check_uv(it, s, "dis", 1e-5 if it == 0 else 1e-4),
                      after_gen=lambda it, s: check_uv(it, s, "gen", 1e-4))


@pytest.mark.gpu
def test_tiny_sn_dis_penalties_vs_reference(golden_dir):
    """dis.norm 'sn' with gp_w = 10 and use_r1 (iteration 15): the penalties' scale-0 calls run one more iteration each, then
    W_bar / sigma in torch for the double backward; scalars, every D gradient and u / v against the reference."""
    fx = ts.load(golden_dir, "tiny_sn_step")
    ref = fx.npz
    with ts.host_noise():
        cfg = dict(_sn_config(), gp_w=10.0, use_r1=True)
        s = ts.build(cfg, DEV)
        grabbed = ts.grab_dis(s)
        s.dis_update(*ts.step_args(fx.batch(DEV), cfg, 15))
        for k in ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1"):
            got, want = float(getattr(s, k)), float(ref["pen/" + k])
            assert abs(got - want) <= 2e-4 * max(abs(want), 1e-12) + (2e-4 if k != "loss_r1" else 0.0), (k, got, want)
        ref_g = {k[len("pen/dgrad/"):]: T(ref[k]) for k in ref.files if k.startswith("pen/dgrad/")}
        assert set(ref_g) == {k for k, g in grabbed.items() if g is not None}
        for k, g in ref_g.items():
            close(grabbed[k], g, rel=2e-3, msg=k)
        for k, v in _uv(s).items():
            close(v, T(ref["pen/after_dis/" + k]), rel=0, atol=1e-5, msg="pen after_dis " + k)
