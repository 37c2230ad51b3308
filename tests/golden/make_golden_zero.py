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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_record as tr                                   # noqa: E402  (the recording itself; make_golden's import_reference)
from make_golden_lrelu import freeze_in_fed_biases         # noqa: E402  (finds nothing here: dis.norm is 'none')


def tiny_zero_config():
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["gen"]["pad_type"] = "zero"
    cfg["dis"]["pad_type"] = "zero"
    return cfg


def gen_zero(ref_solver):
    cfg = tiny_zero_config()
    batch = tr.tiny_batch()
    first, second = [tr.two_iterations(ref_solver, cfg, b, freeze=freeze_in_fed_biases) for b in (batch, tr.one_ulp(batch))]
    tr.write_with_sens("tiny_zero", "pad_type zero", batch, first, second)


if __name__ == "__main__":
    gen_zero(tr.mg.import_reference()[0])
