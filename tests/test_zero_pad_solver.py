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
import pytest
import torch

import tiny_solver as ts
from hipdwc import synth          # noqa: E402

T = torch.from_numpy


def _config():
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["pad_type"] = "zero"
    cfg["dis"]["pad_type"] = "zero"
    return cfg


def test_tiny_zero_init_equals_reference(golden_dir):
    """Fails before the strided convolutions took the zero rule: neither network could be constructed."""
    fx = ts.load(golden_dir, "tiny_zero")
    s = ts.build(_config())
    ts.check_init(s, fx)
    assert torch.equal(torch.get_rng_state(), T(fx.npz["rng_state_after_init"]))


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
    fx = ts.load(golden_dir, "tiny_zero")
    assert not fx.frozen                                   # every D parameter has a recorded gradient
    worst = {}
    try:
        ts.two_iterations(fx, _config(), ts.SENS_BOUNDS, worst=worst,
                          before_loop=lambda s: _forbid_torch_padding_and_convolution(monkeypatch))
    finally:
        print("pad_type zero: largest ratio to sens: %s" % ts.ratios(worst))


@pytest.mark.gpu
def test_tiny_zero_bf16_iteration_vs_reference(golden_dir):
    """Iteration 0 under bf16 activations, at the bf16 bounds of tests/test_lrelu_solver.py: the 16 loss scalars are finite and within
    3e-2 of max(1, |value|), loss_dis_all and loss_gen_total within 2e-2 relative."""
    ts.bf16_iteration0(ts.load(golden_dir, "tiny_zero"), _config())
