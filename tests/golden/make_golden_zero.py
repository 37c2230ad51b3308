#!/usr/bin/env python3
"""Record the ``pad_type: zero`` fixture (zero padding in every Conv2dBlock of G and D) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py and make_golden_lrelu.py, whose helpers it imports); the tests
read the .npz file it writes:

    python tests/golden/make_golden_zero.py          # tiny_zero.npz; seconds

The tiny Solver (32x32, B = 3) with gen.pad_type = dis.pad_type = 'zero'.  The file holds what tiny_lrelu_*.npz hold (see
make_golden_lrelu.py): the random stream after construction and the checksums of the initial tensors, two iterations (loss scalars,
D gradients of both D steps, of iteration 0 the sampled G gradients and their statistics) and ``sens_json``, the deviation of every
key in a second run of the reference under one ulp of input noise.  It stays below tiny_bn_step.npz.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg            # noqa: E402
import make_golden_lrelu as ml      # noqa: E402  (run_tiny: the recording itself)

synth = mg.synth
t2n = mg.t2n


def tiny_zero_config():
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["pad_type"] = "zero"
    cfg["dis"]["pad_type"] = "zero"
    return cfg


def gen_zero(ref_solver):
    cfg = tiny_zero_config()
    batch = synth.make_batch(3, 32, seed=4321)
    init, rec, losses, frozen = ml.run_tiny(ref_solver, cfg, batch)
    out = dict(init)
    for k, v in batch.items():
        out["batch/%s" % k] = t2n(v)
    out.update(rec)
    out["losses_json"] = np.frombuffer(json.dumps(losses).encode(), dtype=np.uint8)
    out["frozen_json"] = np.frombuffer(json.dumps(frozen).encode(), dtype=np.uint8)

    # what one ulp of input noise does to the reference itself (make_golden_lrelu.gen_variant)
    g = torch.Generator().manual_seed(5)
    noisy = dict(batch)
    noisy["x_real"] = batch["x_real"] * (1 + 2.0 ** -23 * torch.randn(batch["x_real"].shape, generator=g))
    _, rec2, losses2, _ = ml.run_tiny(ref_solver, cfg, noisy)
    worst, sens = {}, {}
    for k, v in rec.items():
        if k == "it0/gstat":
            continue
        a, b = v.astype(np.float64), rec2[k].astype(np.float64)
        d = max(float(np.abs(a - b).max()), float(np.spacing(np.float32(np.abs(a).max()))))
        sens[k] = d
        kind = "/".join(k.split("/")[:2])
        worst[kind] = max(worst.get(kind, 0.0), d)
    for it in range(2):
        for k in losses[it]:
            d = abs(losses[it][k] - losses2[it][k])
            sens["it%d/loss/%s" % (it, k)] = max(d, float(np.spacing(np.float32(abs(losses[it][k])))))
    out["sens_json"] = np.frombuffer(json.dumps(sens).encode(), dtype=np.uint8)
    print("pad_type zero: sensitivity (largest deviation per kind):", {k: "%.2e" % v for k, v in sorted(worst.items())},
          "losses", ["%.2e" % max(sens["it%d/loss/%s" % (it, k)] for k in losses[it]) for it in range(2)])
    path = os.path.join(HERE, "tiny_zero.npz")
    np.savez_compressed(path, **out)
    print("%s written (%d bytes); frozen: %s; losses: %s" % (os.path.basename(path), os.path.getsize(path), frozen,
                                                              [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses]))


if __name__ == "__main__":
    gen_zero(mg.import_reference()[0])
