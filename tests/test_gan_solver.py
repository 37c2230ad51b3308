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
import os

import pytest
import torch

import tiny_solver as ts
from hipdwc import ops, synth          # noqa: E402

T = torch.from_numpy
FIXTURES = {"tiny_nsgan": ("nsgan", 0), "tiny_wgan_gp": ("wgan", 10)}
BOUNDS = ts.SENS_BOUNDS._replace(frozen="none")          # what the recording froze has no gradient here either


def _config(name):
    gan_type, gp_w = FIXTURES[name]
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["gan_type"] = gan_type
    cfg["gp_w"] = gp_w
    return cfg


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_tiny_gan_init_equals_reference(golden_dir, name):
    fx = ts.load(golden_dir, name)
    s = ts.build(_config(name))
    assert s.dis.gan_type == FIXTURES[name][0]
    ts.check_init(s, fx)
    assert torch.equal(torch.get_rng_state(), T(fx.npz["rng_state_after_init"]))
    assert os.path.getsize(fx.path) < os.path.getsize(os.path.join(golden_dir, "tiny_bn_step.npz"))
    if name == "tiny_nsgan":          # the recording itself stays where binary_cross_entropy(sigmoid(.)) is the softplus to 2.5e-7
        assert 0.0 < float(fx.npz["max_abs_src"]) < 6.0


def _two_iterations(golden_dir, name):
    fx = ts.load(golden_dir, name)
    assert fx.frozen == ({"cnns_src.0.bias", "cnns_src.1.bias"} if FIXTURES[name][0] == "wgan" else set())

    def freeze(s):             # frozen in the recording (module docstring): Adam skips what has no gradient
        for k, p in s.dis.named_parameters():
            if k in fx.frozen:
                p.requires_grad_(False)
    worst = {}
    try:
        ts.two_iterations(fx, _config(name), BOUNDS, before_loop=freeze, worst=worst)
    finally:
        print("%s (ADV_TAIL_GAN %d): largest ratio to sens: %s" % (name, ops.ADV_TAIL_GAN, ts.ratios(worst, ggrad=True)))


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
