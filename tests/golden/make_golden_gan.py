#!/usr/bin/env python3
"""Record the ``dis.gan_type: nsgan`` and ``wgan`` (+ gradient penalty) fixtures by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); the tests read the .npz files
it writes:

    python tests/golden/make_golden_gan.py          # tiny_nsgan.npz, tiny_wgan_gp.npz; seconds

Both are the tiny Solver (32x32, B = 3, synth.make_config(image_size=32, tiny=True), batch seed 4321).  tiny_nsgan.npz sets
dis.gan_type = 'nsgan'; tiny_wgan_gp.npz sets 'wgan' with gp_w = 10 (WGAN-GP; the reference adds the penalty to loss_dis in place, so
loss_dis and loss_dis_all both carry it).  Each holds what the lrelu fixtures hold (make_golden_lrelu.py):
* the random stream after construction and, per state_dict key of G and D in order, shape and (sum, sum of squares) of the initial
  tensor;
* two iterations: every loss scalar and every D gradient of both D steps (grabbed in front of dis_opt.step); of iteration 0 the G
  gradients left behind by gen_update: 32 evenly spread entries of each (``it0/ggrad``) and its largest magnitude, sum and sum of
  squares (``it0/gstat``) in the order of ``it0/ggrad_names``.  Each file stays below tiny_bn_step.npz;
* ``sens_json``, key -> the largest deviation of that key in a second run of the reference on x_real * (1 + 2^-23 randn), floored at one
  fp32 spacing of the key's largest value (and see the src biases below);
* ``max_abs_src``: the largest |src| any call of the reference's discriminator produced during the two iterations.  For nsgan the script
  asserts it below MAX_SRC = 6: there 1 - sigmoid(src) keeps 14 of its 24 bits, and the reference's own
  binary_cross_entropy(sigmoid(src), .) is within 2.5e-7 relative of the exact softplus, so the recording does not depend on how one
  expf rounds (between 8 and 25 it does: tests/test_gan_tails.py).  It holds at batch seed 4321; no other seed was needed.

The biases of the 1x1 src heads (``cnns_src.<scale>.bias``) are where these two objectives differ from lsgan, and both cases are
handled the way make_golden_lrelu.py handles the biases in front of an instance norm:
* wgan: the D objective mean(src_fake) - mean(src_real) (+ a penalty on d src / d x) does not depend on a constant added to src, so the
  TRUE gradient of these biases is zero.  The reference computes 1/N - 1/N sums that leave 0 or +-1e-7, and Adam turns the sign of that
  noise into a +-lr step, which then moves loss_gen_adv = -mean(src) by lr per scale and term.  They are frozen
  (``frozen_json``; requires_grad_(False), so Adam and its weight decay skip them), in the reference here and in the Solver under test.
* nsgan: the gradient is mean(p_fake) + mean(p_fake1) - 2 mean(1 - p_real), weighted: with the tiny D's |src| ~ 1e-4 every p is 0.5 +- 3e-5,
  the terms sum to 2.0 in magnitude and cancel to ~1e-5.  The sign is safe (noise 1e-7), so nothing is frozen; but a second run of the
  reference repeats the same roundings, and the spacing of the RESULT (9e-13) says nothing about a sum of terms of size 1.  The
  ``sens`` of these keys is therefore floored at one fp32 spacing of sum_i |d loss / d src_i| of that D step and scale (measured with
  hooks on the reference's src maps; 2.0 -> 2.4e-7), the same rule -- one spacing of what was rounded -- applied to the summands.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_record as tr  # noqa: E402  (the recording itself; make_golden's import_reference)

MAX_SRC = 6.0


def tiny_gan_config(gan_type, gp_w):
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["gan_type"] = gan_type
    cfg["gp_w"] = gp_w
    return cfg


class DisProbe:
    """While active, over every forward of the reference's MsImageDis: the largest |src| (``worst``) and, per scale, the sum of
    |d loss / d src_i| that autograd sends back into the src maps (``abs_grad``; the recorder clears it in front of each D step)."""

    def __init__(self, ref_nets):
        self.cls, self.worst, self.abs_grad = ref_nets.MsImageDis, 0.0, {}

    def __enter__(self):
        real = self.real = self.cls.forward

        def forward(dis, *a, **k):
            outs = real(dis, *a, **k)
            for scale, o in enumerate(outs):
                self.worst = max(self.worst, float(o[0].detach().abs().max()))
                if o[0].requires_grad:
                    o[0].register_hook(lambda g, scale=scale: self.abs_grad.__setitem__(
                        scale, self.abs_grad.get(scale, 0.0) + float(g.detach().abs().sum())))
            return outs
        self.cls.forward = forward
        return self

    def __exit__(self, *exc):
        self.cls.forward = self.real


def freeze_src_biases(dis):
    frozen = []
    for s, conv in enumerate(dis.cnns_src):
        conv.bias.requires_grad_(False)
        frozen.append("cnns_src.%d.bias" % s)
    return frozen


def run_probed(ref_solver, cfg, batch, probe):
    """The shared two-iteration recording with the src biases frozen for wgan and the probe read after each D step
    -> (what tr.two_iterations returns, key of a src bias' gradient -> sum |d loss / d src_i| of that D step and scale)."""
    src_terms = {}

    def read_probe(it, trainer, out):
        for scale, v in probe.abs_grad.items():
            src_terms[(tr.ts.DGRAD % it) + "cnns_src.%d.bias" % scale] = v
    run = tr.two_iterations(ref_solver, cfg, batch, freeze=freeze_src_biases if cfg["dis"]["gan_type"] == "wgan" else None,
                            before_dis=lambda it, trainer: probe.abs_grad.clear(), after_dis=read_probe)
    return run, src_terms


def gen_variant(ref_solver, ref_nets, name, gan_type, gp_w):
    cfg = tiny_gan_config(gan_type, gp_w)
    batch = tr.tiny_batch()
    with DisProbe(ref_nets) as probe:
        first, src_terms = run_probed(ref_solver, cfg, batch, probe)
        worst_src = probe.worst
        assert worst_src > 0.0 and len(src_terms) == 4, (worst_src, src_terms)
        if gan_type == "nsgan":
            assert worst_src < MAX_SRC, "nsgan: the reference's D reached |src| = %.3f >= %g: choose another batch seed" % (worst_src, MAX_SRC)
        second, _ = run_probed(ref_solver, cfg, tr.one_ulp(batch), probe)
    print("%s: largest |src| %.3e; sum |d loss / d src| per D step and scale %s"
          % (name, worst_src, {k: "%.4g" % v for k, v in sorted(src_terms.items())}))
    # (a src bias' gradient is a cancelling sum: its sens is floored at one spacing of the summands' total magnitude, module docstring)
    tr.write_with_sens(name, name, batch, first, second, floors=src_terms, extra={"max_abs_src": np.array(worst_src, dtype=np.float64)})


if __name__ == "__main__":
    ref = tr.mg.import_reference()
    gen_variant(ref[0], ref[1], "tiny_nsgan", "nsgan", 0)
    gen_variant(ref[0], ref[1], "tiny_wgan_gp", "wgan", 10)
