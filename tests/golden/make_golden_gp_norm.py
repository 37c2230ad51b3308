#!/usr/bin/env python3
"""Record the gradient / R1 penalty fixtures of a discriminator with ``dis.norm: ln`` and ``in`` by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); the tests read the .npz files
it writes:

    python tests/golden/make_golden_gp_norm.py      # tiny_penalties_ln.npz, tiny_penalties_in.npz; seconds

Recipe and layout are those of ``gen_penalties`` in make_golden.py with ``dis.norm`` set: the tiny Solver (32x32, B = 3) from the
seed-1234 initialisation, batch seed 4321, ``dis_update`` at iteration 15 with gp_w = 10 and use_r1 (so that the R1 term is live):
``rng_state_after_init``, the four loss scalars, ``grad/<name>`` for every D parameter (grabbed in front of dis_opt.step) and
``meta``.  Added: ``x_hat``, the point at which the reference took the gradient penalty (so that a test without a generator can
repeat it), and, as in make_golden_gan.py: ``sens_json``, key -> the largest deviation of that key in a second run of the reference
on x_real * (1 + 2^-23 randn), floored at one fp32 spacing of the key's largest value.

The tests hold scalars to 2e-4 relative and every gradient to 2e-3 of its largest magnitude; a key whose TRUE value is zero (a conv
bias in front of an instance norm: the reference records rounding noise there) is held to 2e-3 of its layer's weight gradient.  The
script asserts every sensitivity below a QUARTER of that bound and walks BATCH_SEEDS until one holds; ``meta`` records the seed
(the tests build the batch from it).  Both variants hold at the first, 4321.  Each file stays below tiny_bn_step.npz.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_record as tr  # noqa: E402  (the recording itself; make_golden's import_reference)

BATCH_SEEDS = (4321, 4322, 4323, 4324)
SCALARS = tr.PENALTY_SCALARS


def run(ref_solver, norm, x_scale, batch_seed):
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = norm
    cfg["gp_w"], cfg["use_r1"] = 10.0, True

    def keep_x_hat(trainer, out):
        real_gp = trainer.gradient_penalty

        def gp_and_its_input(y, x):
            out["x_hat"] = tr.t2n(x)                   # (alpha and x_fake come from the recording's random stream and generator)
            return real_gp(y, x)
        trainer.gradient_penalty = gp_and_its_input
    return tr.penalties(ref_solver, cfg, tr.tiny_batch(batch_seed), x_scale=x_scale, setup=keep_x_hat)[1]


def bound(rec, k, norm):
    """The tests' absolute bound on key k."""
    if not k.startswith("grad/"):
        return 2e-4 * abs(float(rec[k]))
    if norm == "in" and k.endswith(".conv.bias") and k.split(".")[-3] != "0":      # (block 0 of a scale has no norm)
        return 2e-3 * float(np.abs(rec[k[:-4] + "weight"]).max())
    return 2e-3 * float(np.abs(rec[k]).max())


def gen_variant(ref_solver, norm):
    for seed in BATCH_SEEDS:
        rec = run(ref_solver, norm, 1.0, seed)
        g = torch.Generator().manual_seed(5)
        rec2 = run(ref_solver, norm, 1 + 2.0 ** -23 * torch.randn(3, 3, 32, 32, generator=g), seed)
        sens, worst = {}, 0.0
        for k in rec:
            if k in ("rng_state_after_init", "x_hat"):
                continue
            sens[k] = tr.deviation(rec[k], rec2[k])
            lim = bound(rec, k, norm)
            worst = max(worst, sens[k] / lim if lim > 0 else 0.0)
        print("norm %s, batch seed %d: largest sensitivity / bound %.3f" % (norm, seed, worst))
        if worst <= 0.25:
            break
    else:
        raise SystemExit("norm %s: no batch seed of %s keeps every sensitivity below a quarter of its bound" % (norm, BATCH_SEEDS))
    rec["sens_json"] = tr.json_bytes(sens)
    rec["meta"] = tr.json_bytes({"gp_w": 10.0, "use_r1": True, "iters": 15, "B": 3, "S": 32, "batch_seed": seed, "seed": 1234,
                                 "norm": norm})
    size = tr.write("tiny_penalties_%s" % norm, rec)
    print("tiny_penalties_%s.npz written (%d bytes):" % (norm, size), {k: float(rec[k]) for k in SCALARS})


if __name__ == "__main__":
    ref = tr.mg.import_reference()
    for norm in ("ln", "in"):
        gen_variant(ref[0], norm)
