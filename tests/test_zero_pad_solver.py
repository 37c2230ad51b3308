"""``gen.pad_type: zero`` with ``dis.pad_type: zero``: two iterations of the tiny Solver with the zero rule inside the HIP convolutions
against the imported reference (tests/golden/make_golden_zero.py wrote tiny_zero.npz).

The bounds are those of tests/test_lrelu_solver.py::test_tiny_lrelu_two_iterations_vs_reference.  Iteration 0 sees the reference's
own weights: loss scalars 2e-4 of max(1, |value|), D gradients 2e-3 of the tensor's largest magnitude (+1e-6), the sampled G
gradients 5e-3 of the tensor's largest magnitude (+1e-6).  Iteration 1 follows an Adam step of +-lr on every parameter: its D
gradients and loss scalars are held to 16 x ``sens``, ``sens`` being the deviation the reference itself shows under one ulp of input
noise (floored at one fp32 spacing).  During the two iterations torch.nn.functional.pad raises on a 4-D tensor and
torch.nn.functional.conv2d raises: the padding rule is inside the kernels' gather, no activation is padded on the device and no
convolution runs on torch.

Largest ratio to ``sens`` measured on the MI355X: see the docstring of test_tiny_zero_two_iterations_vs_reference."""
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


def _config():
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["pad_type"] = "zero"
    cfg["dis"]["pad_type"] = "zero"
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
    """Same state_dict keys and shapes, in order, and the checksums of the reference's initial tensors."""
    for net, mod in (("gen", s.gen), ("dis", s.dis)):
        want = json.loads(bytes(ref["init_keys/%s" % net]).decode())
        sd = mod.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == want, net
        sums = ref["init_sums/%s" % net]
        for (k, v), w in zip(sd.items(), sums):
            got = _checksum(v.cpu())
            assert abs(got[0] - w[0]) <= 1e-9 * max(1.0, abs(w[0])) and abs(got[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])), (net, k, got, w)


def test_tiny_zero_init_equals_reference(golden_dir):
    """Fails before the strided convolutions took the zero rule: neither network could be constructed."""
    ref = np.load(os.path.join(golden_dir, "tiny_zero.npz"))
    s = _build(_config())
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


def _forbid_torch_padding_and_convolution(monkeypatch):
    real_pad = torch.nn.functional.pad

    def pad(t, *a, **k):
        if t.dim() == 4:
            raise AssertionError("the Solver reached torch.nn.functional.pad with a 4-D tensor: the zero rule is not inside the kernel")
        return real_pad(t, *a, **k)            # (1-D: a bias padded to the aligned channel count)

    def conv2d(*a, **k):
        raise AssertionError("the Solver reached torch.nn.functional.conv2d")
    monkeypatch.setattr(torch.nn.functional, "pad", pad)
    monkeypatch.setattr(torch.nn.functional, "conv2d", conv2d)


@pytest.mark.gpu
def test_tiny_zero_two_iterations_vs_reference(golden_dir, monkeypatch):
    """Measured on the MI355X, largest ratio to ``sens``: D gradients 5.00 / 3.00 (iteration 0 / 1), loss scalars 4.00 / 1.50."""
    ref = np.load(os.path.join(golden_dir, "tiny_zero.npz"))
    want = json.loads(bytes(ref["losses_json"]).decode())
    frozen = set(json.loads(bytes(ref["frozen_json"]).decode()))
    sens = json.loads(bytes(ref["sens_json"]).decode())
    gnames = json.loads(bytes(ref["it0/ggrad_names"]).decode())
    assert not frozen
    ops.set_precision("fp32")
    host.set_noise(host.HostNoise())
    worst = {}
    try:
        cfg = _config()
        s = _build(cfg, DEV)
        _check_init(s, ref)
        assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
        batch = {k[len("batch/"):]: T(ref[k]).to(DEV) for k in ref.files if k.startswith("batch/")}
        grabbed = _grab_dis(s)
        _forbid_torch_padding_and_convolution(monkeypatch)
        for it in range(2):
            a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                 batch["label_trg"], cfg, it)
            grabbed.clear()
            s.dis_update(*a)
            ref_g = {k[len("it%d/dgrad/" % it):]: T(ref[k]) for k in ref.files if k.startswith("it%d/dgrad/" % it)}
            assert set(ref_g) == set(grabbed)
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
                    print("it0 ggrad %s: max err %.3e, limit %.3e" % (k, err, 5e-3 * amax + 1e-6))
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
        print("pad_type zero: largest ratio to sens: %s" % {k: "%.2f" % v for k, v in sorted(worst.items())})


@pytest.mark.gpu
def test_tiny_zero_bf16_iteration_vs_reference(golden_dir):
    """Iteration 0 under bf16 activations, at the bf16 bounds of tests/test_lrelu_solver.py: the 16 loss scalars are finite and within
    3e-2 of max(1, |value|), loss_dis_all and loss_gen_total within 2e-2 relative."""
    ref = np.load(os.path.join(golden_dir, "tiny_zero.npz"))
    want = json.loads(bytes(ref["losses_json"]).decode())[0]
    assert len(want) == 16
    ops.set_precision("bf16")
    host.set_noise(host.HostNoise())
    try:
        cfg = _config()
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
