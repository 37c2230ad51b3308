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
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_reference, build_ref_solver, read_losses, checksum, t2n; synth)
from make_golden_lrelu import sample_idx  # noqa: E402  (which entries of a G gradient the fixtures keep)

synth = mg.synth
t2n = mg.t2n
BATCH_SEED = 4321
MAX_SRC = 6.0
LIMIT_BYTES = 290030          # tiny_bn_step.npz


def tiny_gan_config(gan_type, gp_w):
    cfg = synth.make_config(image_size=32, tiny=True)
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


def run_tiny(ref_solver, cfg, batch, probe):
    """make_golden_lrelu.py run_tiny, with the src biases frozen for wgan and the probe read after each D step."""
    trainer = mg.build_ref_solver(ref_solver, cfg)
    init = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    for net, mod in (("gen", trainer.gen), ("dis", trainer.dis)):
        sd = mod.state_dict()
        init["init_keys/%s" % net] = np.frombuffer(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode(), dtype=np.uint8)
        init["init_sums/%s" % net] = np.array([mg.checksum(v) for v in sd.values()], dtype=np.float64)
    frozen = freeze_src_biases(trainer.dis) if cfg["dis"]["gan_type"] == "wgan" else []
    out, grabbed, src_terms = {}, {}, {}
    real_step = trainer.dis_opt.step

    def grab_then_step(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            if p.grad is not None:
                grabbed[k] = t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = grab_then_step
    losses, gnames, gsamples, gstats = [], [], [], []
    for it in range(2):
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, it)
        grabbed.clear()
        probe.abs_grad.clear()
        trainer.dis_update(*a)
        for scale, v in probe.abs_grad.items():
            src_terms["it%d/dgrad/cnns_src.%d.bias" % (it, scale)] = v
        for k, v in grabbed.items():
            out["it%d/dgrad/%s" % (it, k)] = v
        trainer.gen_update(*a)
        for k, p in trainer.gen.named_parameters():
            if it == 0 and p.grad is not None:
                flat = p.grad.detach().reshape(-1)
                d = flat.double()
                gnames.append(k)
                gsamples.append(t2n(flat[torch.from_numpy(sample_idx(flat.numel()))]))
                gstats.append([float(d.abs().max()), float(d.sum()), float((d * d).sum())])
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
        losses.append(mg.read_losses(trainer))
    out["it0/ggrad"] = np.concatenate(gsamples)
    out["it0/gstat"] = np.array(gstats, dtype=np.float64)
    init["it0/ggrad_names"] = np.frombuffer(json.dumps(gnames).encode(), dtype=np.uint8)
    return init, out, losses, frozen, src_terms


def gen_variant(ref_solver, ref_nets, name, gan_type, gp_w):
    cfg = tiny_gan_config(gan_type, gp_w)
    batch = synth.make_batch(3, 32, seed=BATCH_SEED)
    with DisProbe(ref_nets) as probe:
        init, rec, losses, frozen, src_terms = run_tiny(ref_solver, cfg, batch, probe)
        worst_src = probe.worst
        assert worst_src > 0.0 and len(src_terms) == 4, (worst_src, src_terms)
        if gan_type == "nsgan":
            assert worst_src < MAX_SRC, "nsgan: the reference's D reached |src| = %.3f >= %g: choose another batch seed" % (worst_src, MAX_SRC)
        # what one ulp of input noise does to the reference itself
        g = torch.Generator().manual_seed(5)
        noisy = dict(batch)
        noisy["x_real"] = batch["x_real"] * (1 + 2.0 ** -23 * torch.randn(batch["x_real"].shape, generator=g))
        _, rec2, losses2, _, _ = run_tiny(ref_solver, cfg, noisy, probe)
    out = dict(init)
    for k, v in batch.items():
        out["batch/%s" % k] = t2n(v)
    out.update(rec)
    out["losses_json"] = np.frombuffer(json.dumps(losses).encode(), dtype=np.uint8)
    out["frozen_json"] = np.frombuffer(json.dumps(frozen).encode(), dtype=np.uint8)
    out["max_abs_src"] = np.array(worst_src, dtype=np.float64)
    worst, sens = {}, {}
    for k, v in rec.items():
        if k == "it0/gstat":
            continue
        a, b = v.astype(np.float64), rec2[k].astype(np.float64)
        d = max(float(np.abs(a - b).max()), float(np.spacing(np.float32(np.abs(a).max()))))
        if k in src_terms:          # a cancelling sum: one spacing of the summands' total magnitude (module docstring)
            d = max(d, float(np.spacing(np.float32(src_terms[k]))))
        sens[k] = d
        kind = "/".join(k.split("/")[:2])
        worst[kind] = max(worst.get(kind, 0.0), d)
    for it in range(2):
        for k in losses[it]:
            d = abs(losses[it][k] - losses2[it][k])
            sens["it%d/loss/%s" % (it, k)] = max(d, float(np.spacing(np.float32(abs(losses[it][k])))))
    out["sens_json"] = np.frombuffer(json.dumps(sens).encode(), dtype=np.uint8)
    print("%s: largest |src| %.3e; sum |d loss / d src| per D step and scale %s; sensitivity (largest deviation per kind):"
          % (name, worst_src, {k: "%.4g" % v for k, v in sorted(src_terms.items())}), {k: "%.2e" % v for k, v in sorted(worst.items())},
          "losses", ["%.2e" % max(sens["it%d/loss/%s" % (it, k)] for k in losses[it]) for it in range(2)])
    path = os.path.join(HERE, "%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LIMIT_BYTES, (path, size)
    print("%s written (%d bytes); frozen: %s; losses: %s" % (os.path.basename(path), size, frozen,
                                                              [(l["loss_dis_all"], l["loss_gen_adv"], l["loss_gen_total"]) for l in losses]))


if __name__ == "__main__":
    ref = mg.import_reference()
    gen_variant(ref[0], ref[1], "tiny_nsgan", "nsgan", 0)
    gen_variant(ref[0], ref[1], "tiny_wgan_gp", "wgan", 10)
