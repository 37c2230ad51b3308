#!/usr/bin/env python3
"""Record the ``gen.activ: lrelu`` fixtures (LeakyReLU 0.1 behind IN / AdaIN / LN and in the MLP) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); the tests read the .npz files
it writes:

    python tests/golden/make_golden_lrelu.py          # tiny_lrelu_in.npz, tiny_lrelu_ln.npz; seconds

Both are the tiny Solver (32x32, B = 3) with gen.activ = 'lrelu'; dis.norm = 'in' in the first, 'ln' in the second (dis.activ is
'lrelu' by default).  Each holds
* the random stream after construction and, per state_dict key of G and D in order, shape and (sum, sum of squares) of the initial
  tensor -- the initialisation is a pure function of the seed, which tests/test_host_logic.py holds bit for bit against the
  reference, so the checksums stand for the 870 KB of weights themselves (LayerNorm draws its gamma: 'ln' shifts the stream);
* two iterations: every loss scalar and every D gradient of both D steps (grabbed in front of dis_opt.step); of iteration 0, as in
  tiny_step.npz, the G gradients left behind by gen_update: 32 evenly spread entries of each (``ggrad``) and its largest
  magnitude, sum and sum of squares (``gstat``), packed into one array each in the order of ``it0/ggrad_names`` (an archive
  member costs some 300 bytes whatever it holds).  Each file stays below tiny_bn_step.npz.
The convolution biases of D that feed an instance norm are frozen first: their true gradient is zero and the reference's rounding
noise there becomes +-lr Adam steps ('in' only; a bias in front of the MUNIT LayerNorm has a real gradient).
``sens_json``, key -> the largest deviation of that key in a second run of the reference on x_real * (1 + 2^-23 randn) -- what one ulp
of input noise does to the reference itself, floored at one fp32 spacing of the key's largest value; the test's iteration-1
tolerance is a multiple of it.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_record as tr  # noqa: E402  (the recording itself; make_golden's import_reference)


def tiny_lrelu_config(dis_norm):
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["activ"] = "lrelu"
    cfg["dis"]["norm"] = dis_norm
    return cfg


def freeze_in_fed_biases(dis):
    """requires_grad_(False) on every convolution bias of D whose output goes straight into an instance norm."""
    frozen = []
    for n, m in dis.named_modules():
        if isinstance(getattr(m, "norm", None), torch.nn.InstanceNorm2d) and getattr(m.conv, "bias", None) is not None:
            m.conv.bias.requires_grad_(False)
            frozen.append(n + ".conv.bias")
    return frozen


def gen_variant(ref_solver, dis_norm):
    cfg = tiny_lrelu_config(dis_norm)
    batch = tr.tiny_batch()
    first, second = [tr.two_iterations(ref_solver, cfg, b, freeze=freeze_in_fed_biases) for b in (batch, tr.one_ulp(batch))]
    tr.write_with_sens("tiny_lrelu_%s" % dis_norm, "dis.norm %s" % dis_norm, batch, first, second)


if __name__ == "__main__":
    ref_solver = tr.mg.import_reference()[0]
    for norm in ("in", "ln"):
        gen_variant(ref_solver, norm)
