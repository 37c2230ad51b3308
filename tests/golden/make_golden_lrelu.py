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
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_reference, build_ref_solver, read_losses, t2n; synth)

synth = mg.synth
t2n = mg.t2n
G_SAMPLE = 32


def tiny_lrelu_config(dis_norm):
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["activ"] = "lrelu"
    cfg["dis"]["norm"] = dis_norm
    return cfg


def sample_idx(n):
    """Element numbers of a flattened n-element gradient that the fixture keeps (at most G_SAMPLE, evenly spread)."""
    if n <= G_SAMPLE:
        return np.arange(n)
    return (np.arange(G_SAMPLE, dtype=np.int64) * n) // G_SAMPLE


def freeze_in_fed_biases(dis):
    """requires_grad_(False) on every convolution bias of D whose output goes straight into an instance norm."""
    frozen = []
    for n, m in dis.named_modules():
        if isinstance(getattr(m, "norm", None), torch.nn.InstanceNorm2d) and getattr(m.conv, "bias", None) is not None:
            m.conv.bias.requires_grad_(False)
            frozen.append(n + ".conv.bias")
    return frozen


def run_tiny(ref_solver, cfg, batch):
    trainer = mg.build_ref_solver(ref_solver, cfg)
    init = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    for net, mod in (("gen", trainer.gen), ("dis", trainer.dis)):
        sd = mod.state_dict()
        init["init_keys/%s" % net] = np.frombuffer(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode(), dtype=np.uint8)
        init["init_sums/%s" % net] = np.array([mg.checksum(v) for v in sd.values()], dtype=np.float64)
    frozen = freeze_in_fed_biases(trainer.dis)
    out, grabbed = {}, {}
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
        trainer.dis_update(*a)
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
    return init, out, losses, frozen


def gen_variant(ref_solver, dis_norm):
    cfg = tiny_lrelu_config(dis_norm)
    batch = synth.make_batch(3, 32, seed=4321)
    init, rec, losses, frozen = run_tiny(ref_solver, cfg, batch)
    out = dict(init)
    for k, v in batch.items():
        out["batch/%s" % k] = t2n(v)
    out.update(rec)
    out["losses_json"] = np.frombuffer(json.dumps(losses).encode(), dtype=np.uint8)
    out["frozen_json"] = np.frombuffer(json.dumps(frozen).encode(), dtype=np.uint8)

    # what one ulp of input noise does to the reference itself
    g = torch.Generator().manual_seed(5)
    noisy = dict(batch)
    noisy["x_real"] = batch["x_real"] * (1 + 2.0 ** -23 * torch.randn(batch["x_real"].shape, generator=g))
    _, rec2, losses2, _ = run_tiny(ref_solver, cfg, noisy)
    worst, sens = {}, {}
    for k, v in rec.items():
        if k == "it0/gstat":
            continue
        a, b = v.astype(np.float64), rec2[k].astype(np.float64)
        d = float(np.abs(a - b).max())
        # two fp32 recordings cannot show a deviation below the spacing of the values themselves (0 here means "under one ulp", not
        # "insensitive"): floored at one fp32 spacing of the key's largest magnitude
        d = max(d, float(np.spacing(np.float32(np.abs(a).max()))))
        sens[k] = d
        kind = "/".join(k.split("/")[:2])
        worst[kind] = max(worst.get(kind, 0.0), d)
    for it in range(2):
        for k in losses[it]:
            d = abs(losses[it][k] - losses2[it][k])
            sens["it%d/loss/%s" % (it, k)] = max(d, float(np.spacing(np.float32(abs(losses[it][k])))))
    out["sens_json"] = np.frombuffer(json.dumps(sens).encode(), dtype=np.uint8)
    print("dis.norm %s: sensitivity (largest deviation per kind):" % dis_norm, {k: "%.2e" % v for k, v in sorted(worst.items())},
          "losses", ["%.2e" % max(sens["it%d/loss/%s" % (it, k)] for k in losses[it]) for it in range(2)])
    path = os.path.join(HERE, "tiny_lrelu_%s.npz" % dis_norm)
    np.savez_compressed(path, **out)
    print("%s written (%d bytes); frozen: %s; losses: %s" % (os.path.basename(path), os.path.getsize(path), frozen,
                                                              [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses]))


if __name__ == "__main__":
    ref_solver = mg.import_reference()[0]
    for norm in ("in", "ln"):
        gen_variant(ref_solver, norm)
