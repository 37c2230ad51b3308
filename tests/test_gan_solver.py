"""``dis.gan_type: nsgan`` and ``wgan`` with ``gp_w: 10`` (WGAN-GP): two iterations of the tiny Solver against the imported reference
(tests/golden/make_golden_gan.py wrote tiny_nsgan.npz / tiny_wgan_gp.npz), once on the one-launch loss tails (hipdwc.ops.adv_tail,
dwc_adv_tail_gan_*) and once on the term-by-term route of ``ops.ADV_TAIL_GAN = 0`` -- the route from before the tails took these
objectives -- at the SAME bounds: the fixtures are the yardstick, not the new kernel.

Held exactly like tests/test_lrelu_solver.py.  Iteration 0 sees the reference's own weights: loss scalars 2e-4 of max(1, |value|), D
gradients 2e-3 of the tensor's largest magnitude (+1e-6), the sampled G gradients 5e-3 of it (+1e-6).  Iteration 1 follows an Adam
step of +-lr on every parameter: D gradients and loss scalars within 16 x ``sens``, the deviation the reference itself shows under one
ulp of input noise (floored at one fp32 spacing).  On the tail route MsImageDis._gan_term and torch.nn.functional.binary_cross_entropy
raise: no term of the objective is computed in torch.  The gradient penalty of the wgan runs takes the route ops.PENALTY_HIP selects.
The wgan recording froze the biases of the src heads -- the Wasserstein objective does not depend on them, their gradient is rounding
noise around zero that Adam turns into +-lr steps -- and so does this test; the nsgan recording floors the ``sens`` of those two
gradients at one spacing of their cancelling summands (tests/golden/make_golden_gan.py says why).
Measured on the MI355X, largest ratio to ``sens`` (iteration 0 / 1): tiny_nsgan on the tails D gradients
10.0 / 10.5, loss scalars 7.0 / 3.0, term by term 7.0 / 10.0 and 7.0 / 3.0; tiny_wgan_gp on the tails 10.0 / 10.0 and 6.0 / 4.0, term
by term 12.0 / 10.0 and 6.0 / 4.0; sampled G gradients at most 0.40 of their limit."""
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
FIXTURES = {"tiny_nsgan": ("nsgan", 0), "tiny_wgan_gp": ("wgan", 10)}


def _config(name):
    gan_type, gp_w = FIXTURES[name]
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["gan_type"] = gan_type
    cfg["gp_w"] = gp_w
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


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tiny_gan_init_equals_reference(golden_dir, name):
    ref = np.load(os.path.join(golden_dir, name + ".npz"))
    s = _build(_config(name))
    assert s.dis.gan_type == FIXTURES[name][0]
    _check_init(s, ref)
    assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
    assert os.path.getsize(os.path.join(golden_dir, name + ".npz")) < os.path.getsize(os.path.join(golden_dir, "tiny_bn_step.npz"))
    if name == "tiny_nsgan":          # the recording itself stays where binary_cross_entropy(sigmoid(.)) is the softplus to 2.5e-7
        assert 0.0 < float(ref["max_abs_src"]) < 6.0


def _grab_dis(s):
    grabbed = {}
    real_step = s.dis_opt.step

    def grab(*a, **k):
        grabbed.update({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in s.dis.named_parameters()})
        return real_step(*a, **k)
    s.dis_opt.step = grab
    return grabbed


def _two_iterations(golden_dir, name):
    ref = np.load(os.path.join(golden_dir, name + ".npz"))
    want = json.loads(bytes(ref["losses_json"]).decode())
    sens = json.loads(bytes(ref["sens_json"]).decode())
    gnames = json.loads(bytes(ref["it0/ggrad_names"]).decode())
    frozen = set(json.loads(bytes(ref["frozen_json"]).decode()))
    assert frozen == ({"cnns_src.0.bias", "cnns_src.1.bias"} if FIXTURES[name][0] == "wgan" else set())
    ops.set_precision("fp32")
    host.set_noise(host.HostNoise())
    worst = {}
    try:
        cfg = _config(name)
        s = _build(cfg, DEV)
        _check_init(s, ref)
        assert torch.equal(torch.get_rng_state(), T(ref["rng_state_after_init"]))
        batch = {k[len("batch/"):]: T(ref[k]).to(DEV) for k in ref.files if k.startswith("batch/")}
        grabbed = _grab_dis(s)
        for k, p in s.dis.named_parameters():             # frozen in the recording (module docstring): Adam skips what has no gradient
            if k in frozen:
                p.requires_grad_(False)
        for it in range(2):
            a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                 batch["label_trg"], cfg, it)
            grabbed.clear()
            s.dis_update(*a)
            ref_g = {k[len("it%d/dgrad/" % it):]: T(ref[k]) for k in ref.files if k.startswith("it%d/dgrad/" % it)}
            assert set(ref_g) | frozen == set(grabbed) and not set(ref_g) & frozen
            for k in frozen:
                assert grabbed[k] is None, k
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
                    worst["it0 ggrad / limit"] = max(worst.get("it0 ggrad / limit", 0.0), err / (5e-3 * amax + 1e-6))
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
        print("%s (ADV_TAIL_GAN %d): largest ratio to sens: %s" % (name, ops.ADV_TAIL_GAN, {k: "%.2f" % v for k, v in sorted(worst.items())}))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tiny_gan_two_iterations_on_the_tails(golden_dir, monkeypatch, name):
    """Fails without the tails for nsgan / wgan: adv_loss is not reached, _gan_term is."""
    from networks.networks import MsImageDis

    def no_terms(*a, **k):
        raise AssertionError("the Solver computed a term of the adversarial objective in torch: gan_type is not on the loss tail")
    monkeypatch.setattr(ops, "ADV_TAIL_GAN", 1)
    monkeypatch.setattr(MsImageDis, "_gan_term", no_terms)
    monkeypatch.setattr(torch.nn.functional, "binary_cross_entropy", no_terms)
    _two_iterations(golden_dir, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tiny_gan_two_iterations_term_by_term(golden_dir, monkeypatch, name):
    """ADV_TAIL_GAN = 0, the route these objectives took before the tails: the same fixtures at the same bounds."""
    from networks.networks import MsImageDis
    calls = []
    real = MsImageDis._gan_term
    monkeypatch.setattr(ops, "ADV_TAIL_GAN", 0)
    monkeypatch.setattr(MsImageDis, "_gan_term", lambda self, out, flag: (calls.append(flag), real(self, out, flag))[1])
    _two_iterations(golden_dir, name)
    assert len(calls) == 2 * (2 * 2 * 2 + 2 * 2)          # per iteration: D step 2 pairs x 2 scales x 2 terms, G step 2 fakes x 2 scales
