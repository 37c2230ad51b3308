#!/usr/bin/env python3
"""Record the spectral-normalisation fixtures (``norm='sn'``, reference networks.py:754-816) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); the tests read the .npz
files it writes:

    python tests/golden/make_golden_sn.py          # sn_ops.npz, tiny_sn_init.npz, tiny_sn_step.npz; seconds

* sn_ops.npz -- reference Conv2dBlock(norm='sn') cases: x, the initial u / v / W_bar, b; y after the 1st and the 3rd of three
  consecutive calls on x, u / v after each call; dx, dW_bar, db of sum_j <y_j, gy> over the three calls.
* tiny_sn_init.npz -- the tiny Solver with dis.norm = 'sn' (32x32, B = 3): the initial state_dicts and the random stream after
  construction (G's weights differ from the norm-none fixture's: weights_init draws after D is built).
* tiny_sn_step.npz -- the same Solver: two iterations with every loss scalar, every D gradient of each D step and every SN u / v after each dis_update
  and gen_update; one more D step from the same initialisation with gp_w = 10 and use_r1 (iteration 15).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiny_record as tr  # noqa: E402  (the recording itself; make_golden's import_reference)

t2n = tr.t2n

# (name, B, Cin, Cout, H, k, stride, pad, activation) -- reflect padding; tests/test_spectral_norm.py SN_CASES
SN_CASES = [
    ("k4s2_lrelu", 2, 16, 32, 16, 4, 2, 1, "lrelu"),       # the discriminator's layer
    ("k3s1_tanh", 2, 8, 16, 12, 3, 1, 1, "tanh"),
    ("k4s2_c14_sigmoid", 3, 8, 14, 8, 4, 2, 1, "sigmoid"),  # Cout not a multiple of 4 (padded to 16)
    ("k3s1_c6_none", 2, 16, 6, 10, 3, 1, 1, "none"),        # Cout not a multiple of 4 (padded to 8)
]


def tiny_sn_config():
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = "sn"
    return cfg


def sn_state(trainer):
    return {k: v for k, v in trainer.dis.state_dict().items() if k.endswith("weight_u") or k.endswith("weight_v")}


def gen_sn_ops(ref_nets):
    g = torch.Generator().manual_seed(77)
    out = {}
    for i, (name, B, ci, co, H, k, s, p, act) in enumerate(SN_CASES):
        torch.manual_seed(500 + i)
        blk = ref_nets.Conv2dBlock(ci, co, k, s, p, norm="sn", activation=act, pad_type="reflect")
        m = blk.conv.module
        rec = {"w": m.weight_bar, "b": m.bias, "u0": m.weight_u.clone(), "v0": m.weight_v.clone()}
        x = torch.randn(B, ci, H, H, generator=g).requires_grad_(True)
        ys = []
        for j in range(3):
            ys.append(blk(x))
            rec["u%d" % (j + 1)], rec["v%d" % (j + 1)] = m.weight_u.clone(), m.weight_v.clone()
        gy = torch.randn(ys[0].shape, generator=g)
        sum((y * gy).sum() for y in ys).backward()
        rec.update({"x": x, "y1": ys[0], "y3": ys[2], "gy": gy, "dx": x.grad, "dw": m.weight_bar.grad, "db": m.bias.grad})
        for kk, v in rec.items():
            out["%s/%s" % (name, kk)] = t2n(v)
    tr.write("sn_ops", out, limit=False)
    print("sn_ops.npz:", len(out), "arrays")


def record_uv(trainer, out, prefix):
    for k, v in sn_state(trainer).items():
        out[prefix + k] = t2n(v)


def gen_tiny_sn(ref_solver):
    cfg = tiny_sn_config()
    batch = tr.tiny_batch()
    init, rec, losses, _ = tr.two_iterations(ref_solver, cfg, batch, full_init=True, g_samples=False,
                                             after_dis=lambda it, trainer, out: record_uv(trainer, out, "it%d/after_dis/" % it),
                                             after_gen=lambda it, trainer, out: record_uv(trainer, out, "it%d/after_gen/" % it))
    tr.write("tiny_sn_init", init, limit=False)     # (a file of its own: each stays under 1 MiB)
    out = tr.assemble({"rng_state_after_init": init["rng_state_after_init"]}, batch, rec, losses)

    # gradient penalty + R1 (reference solver.py:337-350) on one D step from the same initialisation, iteration 15
    trainer, pen = tr.penalties(ref_solver, dict(cfg, gp_w=10.0, use_r1=True), batch, grad_prefix="pen/dgrad/", scalar_prefix="pen/")
    del pen["rng_state_after_init"]
    out.update(pen)
    record_uv(trainer, out, "pen/after_dis/")
    tr.write("tiny_sn_step", out, limit=False)
    print("tiny_sn_step.npz written; losses:", [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses])


if __name__ == "__main__":
    ref_solver, ref_nets, _, _, _ = tr.mg.import_reference()
    gen_sn_ops(ref_nets)
    gen_tiny_sn(ref_solver)
