"""``gen.activ: lrelu`` with ``dis.norm: in`` / ``ln`` (``dis.activ: lrelu``): two iterations of the tiny Solver on the fused HIP path
against the imported reference (tests/golden/make_golden_lrelu.py wrote tiny_lrelu_in.npz / tiny_lrelu_ln.npz).

Iteration 0 sees the reference's own weights and is held to what tests/test_batch_norm.py::test_tiny_bn_two_iterations_vs_reference
applies: loss scalars 2e-4 of max(1, |value|), D gradients 2e-3 of the tensor's largest magnitude (+1e-6); the sampled G gradients to
the 5e-3 of tests/test_hip_parity.py::test_tiny_three_iterations_vs_reference.  Iteration 1 follows an Adam step of +-lr on every
parameter: its D gradients and loss scalars are held to 16 x ``sens`` -- the multiple that test uses --, ``sens`` being the deviation
the reference itself shows under one ulp of input noise (floored at one fp32 spacing).  Measured on the MI355X, largest ratio to
``sens``: 'in' D gradients 3.9 / 1.7 (iteration 0 / 1), loss scalars 2.0 / 2.0; 'ln' D gradients 5.0 / 6.0, loss scalars 2.0 / 4.0."""
import pytest
import torch

import tiny_solver as ts
from hipdwc import synth          # noqa: E402

T = torch.from_numpy


def _config(dis_norm):
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["activ"] = "lrelu"
    cfg["dis"]["norm"] = dis_norm
    return cfg


@pytest.mark.parametrize("dis_norm", ["in", "ln"])
def test_tiny_lrelu_init_equals_reference(golden_dir, dis_norm):
    """Fails before LinearBlock took 'lrelu': the generator could not be constructed."""
    fx = ts.load(golden_dir, "tiny_lrelu_%s" % dis_norm)
    s = ts.build(_config(dis_norm))
    ts.check_init(s, fx)
    assert torch.equal(torch.get_rng_state(), T(fx.npz["rng_state_after_init"]))


@pytest.mark.gpu
@pytest.mark.parametrize("dis_norm", ["in", "ln"])
def test_tiny_lrelu_two_iterations_vs_reference(golden_dir, monkeypatch, dis_norm):
    fx = ts.load(golden_dir, "tiny_lrelu_%s" % dis_norm)
    assert (dis_norm == "in") == bool(fx.frozen)          # d/d bias in front of an instance norm: none, or exact zeros

    def no_leaky(*a, **k):
        raise AssertionError("the Solver reached torch.nn.functional.leaky_relu: lrelu is not fused")
    monkeypatch.setattr(torch.nn.functional, "leaky_relu", no_leaky)
    worst = {}
    try:
        ts.two_iterations(fx, _config(dis_norm), ts.SENS_BOUNDS, worst=worst)
    finally:
        print("dis.norm %s: largest ratio to sens: %s" % (dis_norm, ts.ratios(worst)))


@pytest.mark.gpu
def test_tiny_lrelu_bf16_iteration_vs_reference(golden_dir):
    """Iteration 0 of the 'in' variant under bf16 activations: the 16 loss scalars are finite and within the bound the whole-iteration
    bf16 comparison against the reference at the c2 shape applies (tests/test_bf16_parity.py::test_bf16_full_iteration_b128): every
    scalar within 3e-2 of max(1, |value|), loss_dis_all and loss_gen_total within 2e-2 relative."""
    ts.bf16_iteration0(ts.load(golden_dir, "tiny_lrelu_in"), _config("in"))
