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
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_reference, build_ref_solver, t2n; synth)

synth = mg.synth
BATCH_SEEDS = (4321, 4322, 4323, 4324)
LIMIT_BYTES = 290030          # tiny_bn_step.npz
SCALARS = ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1")


def run(ref_solver, norm, x_scale, batch_seed):
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = norm
    cfg["gp_w"], cfg["use_r1"] = 10.0, True
    trainer = mg.build_ref_solver(ref_solver, cfg)
    out = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    batch = synth.make_batch(3, 32, seed=batch_seed)
    grabbed = {}
    real_step = trainer.dis_opt.step

    def grab_then_step(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            grabbed["grad/" + k] = mg.t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = grab_then_step
    real_gp = trainer.gradient_penalty

    def gp_and_its_input(y, x):
        out["x_hat"] = mg.t2n(x)                       # (alpha and x_fake come from the recording's random stream and generator)
        return real_gp(y, x)
    trainer.gradient_penalty = gp_and_its_input
    x_real = batch["x_real"].clone() * x_scale        # (the reference sets requires_grad on the tensor it is handed)
    trainer.dis_update(x_real, batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                       batch["label_trg"], cfg, 15)
    out.update(grabbed)
    for k in SCALARS:
        out[k] = np.float64(float(getattr(trainer, k)))
    return out


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
            a, b = np.asarray(rec[k], dtype=np.float64), np.asarray(rec2[k], dtype=np.float64)
            sens[k] = max(float(np.abs(a - b).max()), float(np.spacing(np.float32(np.abs(a).max()))))
            lim = bound(rec, k, norm)
            worst = max(worst, sens[k] / lim if lim > 0 else 0.0)
        print("norm %s, batch seed %d: largest sensitivity / bound %.3f" % (norm, seed, worst))
        if worst <= 0.25:
            break
    else:
        raise SystemExit("norm %s: no batch seed of %s keeps every sensitivity below a quarter of its bound" % (norm, BATCH_SEEDS))
    rec["sens_json"] = np.frombuffer(json.dumps(sens).encode(), dtype=np.uint8)
    rec["meta"] = np.frombuffer(json.dumps({"gp_w": 10.0, "use_r1": True, "iters": 15, "B": 3, "S": 32, "batch_seed": seed,
                                            "seed": 1234, "norm": norm}).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "tiny_penalties_%s.npz" % norm)
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    assert size < LIMIT_BYTES, (path, size)
    print("%s written (%d bytes):" % (os.path.basename(path), size), {k: float(rec[k]) for k in SCALARS})


if __name__ == "__main__":
    ref = mg.import_reference()
    for norm in ("ln", "in"):
        gen_variant(ref[0], norm)
