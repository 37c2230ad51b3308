"""``gen.activ: lrelu`` with ``dis.norm: in`` / ``ln`` (``dis.activ: lrelu``): two iterations of the tiny Solver on the fused HIP path
against the imported reference (tests/golden/make_golden_lrelu.py wrote tiny_lrelu_in.npz / tiny_lrelu_ln.npz).

Iteration 0 sees the reference's own weights and is held to what tests/test_batch_norm.py::test_tiny_bn_two_iterations_vs_reference
applies: loss scalars 2e-4 of max(1, |value|), D gradients 2e-3 of the tensor's largest magnitude (+1e-6); the sampled G gradients to
the 5e-3 of tests/test_hip_parity.py::test_tiny_three_iterations_vs_reference.  Iteration 1 follows an Adam step of +-lr on every
parameter: its D gradients and loss scalars are held to 16 x ``sens`` -- the multiple that test uses --, ``sens`` being the deviation
the reference itself shows under one ulp of input noise (floored at one fp32 spacing).  Measured on the MI355X, largest ratio to
``sens``: 'in' D gradients 3.9 / 1.7 (iteration 0 / 1), loss scalars 2.0 / 2.0; 'ln' D gradients 5.0 / 6.0, loss scalars 2.0 / 4.0."""
import json
import os

import numpy as np
import pytest
import torch

from hipdwc import host, ops, synth          # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"
SENS_MULTIPLE = 16
G_SAMPLE = 32


def _config(dis_norm):
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["activ"] = "lrelu"
    cfg["dis"]["norm"] = dis_norm
    return cfg


def _build(cfg, device="cpu"):
    from solver import Solver
    torch.manual_seed(1234)
    s = Solver(cfg, torch.device(device), None)
    if device != "cpu":
        s = s.to(device)
    s.copy_nets()
    return s


def _checksum(t):
    t = t.detach().double()
    return [float(t.sum()), float((t * t).sum())]


def _sample_idx(n):          # tests/golden/make_golden_lrelu.py sample_idx
    return torch.arange(n) if n <= G_SAMPLE else (torch.arange(G_SAMPLE, dtype=torch.int64) * n) // G_SAMPLE


def _check_init(s, ref):
    """Same state_dict keys and shapes, in order, and the checksums of the reference's initial tensors; same random stream after."""
    for net, mod in (("gen", s.gen), ("dis", s.dis)):
        want = json.loads(bytes(ref["init_keys/%s" % net]).decode())
        sd = mod.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == want, net
        sums = ref["init_sums/%s" % net]
        for (k, v), w in zip(sd.items(), sums):
            got = _checksum(v.cpu())
            assert abs(got[0] - w[0]) <= 1e-9 * max(1.0, abs(w[0])) and abs(got[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])), (net, k, got, w)


@pytest.mark.parametrize("dis_norm", ["in", "ln"])
def test_tiny_lrelu_init_equals_reference(golden_dir, dis_norm):
    """Fails before LinearBlock took 'lrelu': the generator could not be constructed."""
    ref = np.load(os.path.join(golden_dir, "tiny_lrelu_%s.npz" % dis_norm))
    s = _build(_config(dis_norm))
    _check_init(s, ref)
    assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))


def _grab_dis(s):
    grabbed = {}
    real_step = s.dis_opt.step

    def grab(*a, **k):
        grabbed.update({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in s.dis.named_parameters()})
        return real_step(*a, **k)
    s.dis_opt.step = grab
    return grabbed


@pytest.mark.gpu
@pytest.mark.parametrize("dis_norm", ["in", "ln"])
def test_tiny_lrelu_two_iterations_vs_reference(golden_dir, monkeypatch, dis_norm):
    ref = np.load(os.path.join(golden_dir, "tiny_lrelu_%s.npz" % dis_norm))
    want = json.loads(bytes(ref["losses_json"]).decode())
    frozen = set(json.loads(bytes(ref["frozen_json"]).decode()))
    sens = json.loads(bytes(ref["sens_json"]).decode())
    gnames = json.loads(bytes(ref["it0/ggrad_names"]).decode())
    assert (dis_norm == "in") == bool(frozen)

    def no_leaky(*a, **k):
        raise AssertionError("the Solver reached torch.nn.functional.leaky_relu: lrelu is not fused")
    monkeypatch.setattr(torch.nn.functional, "leaky_relu", no_leaky)
    ops.set_precision("fp32")
    host.set_noise(host.HostNoise())
    worst = {}
    try:
        cfg = _config(dis_norm)
        s = _build(cfg, DEV)
        _check_init(s, ref)
        assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
        batch = {k[len("batch/"):]: T(ref[k]).to(DEV) for k in ref.files if k.startswith("batch/")}
        grabbed = _grab_dis(s)
        for it in range(2):
            a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                 batch["label_trg"], cfg, it)
            grabbed.clear()
            s.dis_update(*a)
            ref_g = {k[len("it%d/dgrad/" % it):]: T(ref[k]) for k in ref.files if k.startswith("it%d/dgrad/" % it)}
            assert set(ref_g) | frozen == set(grabbed) and not set(ref_g) & frozen
            for k in frozen:                              # d/d bias in front of an instance norm: none, or exact zeros
                assert grabbed[k] is None or not grabbed[k].any(), k
            for k, g in ref_g.items():
                err = (grabbed[k].detach().cpu().double() - g.double()).abs().max().item()
                sk = sens["it%d/dgrad/%s" % (it, k)]
                lim = 2e-3 * g.abs().max().item() + 1e-6 if it == 0 else SENS_MULTIPLE * sk
                worst["it%d dgrad" % it] = max(worst.get("it%d dgrad" % it, 0.0), err / sk)
                print("it%d dgrad %s: max err %.3e, limit %.3e, ratio to sens %.2f" % (it, k, err, lim, err / sk))
                assert err <= lim, "it%d dgrad %s: max err %.3e > %.3e" % (it, k, err, lim)
            s.gen_update(*a)
            if it == 0:
                gp = dict(s.gen.named_parameters())
                # (convolution biases in front of an instance norm are flagged `_dwc_zero_grad` and get no gradient tensor: the
                # identically-zero gradient that the reference computes as rounding noise)
                have = [k for k, p in gp.items() if p.grad is not None or getattr(p, "_dwc_zero_grad", False)]
                assert sorted(have) == sorted(gnames)
                off = 0
                for k, (amax, _, _) in zip(gnames, ref["it0/gstat"]):
                    p = gp[k]
                    flat = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).cpu()
                    idx = _sample_idx(flat.numel())
                    w = T(ref["it0/ggrad"][off:off + idx.numel()])
                    off += idx.numel()
                    err = (flat[idx] - w).abs().max().item()
                    assert err <= 5e-3 * amax + 1e-6, "it0 ggrad %s: max err %.3e > %.3e" % (k, err, 5e-3 * amax + 1e-6)
                assert off == ref["it0/ggrad"].shape[0]
            s.smooth_moving()
            s.update_learning_rate()
            s.update_attention_status(it)
            for k, v in want[it].items():
                got = float(torch.as_tensor(getattr(s, k)).detach())
                sk = sens["it%d/loss/%s" % (it, k)]
                lim = 2e-4 * max(1.0, abs(v)) if it == 0 else SENS_MULTIPLE * sk
                worst["it%d loss" % it] = max(worst.get("it%d loss" % it, 0.0), abs(got - v) / sk)
                print("it%d %s: %.7g against %.7g, limit %.3e, ratio to sens %.2f" % (it, k, got, v, lim, abs(got - v) / sk))
                assert abs(got - v) <= lim, (it, k, got, v, lim)
    finally:
        host.set_noise(host.DeviceNoise())
        print("dis.norm %s: largest ratio to sens: %s" % (dis_norm, {k: "%.2f" % v for k, v in sorted(worst.items())}))


@pytest.mark.gpu
def test_tiny_lrelu_bf16_iteration_vs_reference(golden_dir):
    """Iteration 0 of the 'in' variant under bf16 activations: the 16 loss scalars are finite and within the bound the whole-iteration
    bf16 comparison against the reference at the c2 shape applies (tests/test_bf16_parity.py::test_bf16_full_iteration_b128): every
    scalar within 3e-2 of max(1, |value|), loss_dis_all and loss_gen_total within 2e-2 relative."""
    ref = np.load(os.path.join(golden_dir, "tiny_lrelu_in.npz"))
    want = json.loads(bytes(ref["losses_json"]).decode())[0]
    assert len(want) == 16
    ops.set_precision("bf16")
    host.set_noise(host.HostNoise())
    try:
        cfg = _config("in")
        s = _build(cfg, DEV)
        batch = {k[len("batch/"):]: T(ref[k]).to(DEV) for k in ref.files if k.startswith("batch/")}
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, 0)
        s.dis_update(*a)
        s.gen_update(*a)
        torch.cuda.synchronize()
        for k, v in want.items():
            got = float(torch.as_tensor(getattr(s, k)).detach())
            print("%s: %.6g against %.6g (%.2e of max(1, |value|))" % (k, got, v, abs(got - v) / max(1.0, abs(v))))
            assert np.isfinite(got), k
            assert abs(got - v) <= 3e-2 * max(1.0, abs(v)), (k, got, v)
        for k in ("loss_dis_all", "loss_gen_total"):
            got = float(torch.as_tensor(getattr(s, k)).detach())
            assert abs(got - want[k]) <= 2e-2 * abs(want[k]), (k, got, want[k])
    finally:
        host.set_noise(host.DeviceNoise())
        ops.set_precision("fp32")
