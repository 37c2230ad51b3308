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

# (name, B, Cin, Cout, H, k, stride, pad, activation) -- reflect padding; tests/test_spectral_norm.py SN_CASES
SN_CASES = [
    ("k4s2_lrelu", 2, 16, 32, 16, 4, 2, 1, "lrelu"),       # the discriminator's layer
    ("k3s1_tanh", 2, 8, 16, 12, 3, 1, 1, "tanh"),
    ("k4s2_c14_sigmoid", 3, 8, 14, 8, 4, 2, 1, "sigmoid"),  # Cout not a multiple of 4 (padded to 16)
    ("k3s1_c6_none", 2, 16, 6, 10, 3, 1, 1, "none"),        # Cout not a multiple of 4 (padded to 8)
]


def tiny_sn_config():
    cfg = synth.make_config(image_size=32, tiny=True)
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
    np.savez_compressed(os.path.join(HERE, "sn_ops.npz"), **out)
    print("sn_ops.npz:", len(out), "arrays")


def gen_tiny_sn(ref_solver):
    cfg = tiny_sn_config()
    B = 3
    trainer = mg.build_ref_solver(ref_solver, cfg)
    init = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    for k, v in trainer.gen.state_dict().items():
        init["init/gen/%s" % k] = t2n(v)
    for k, v in trainer.dis.state_dict().items():
        init["init/dis/%s" % k] = t2n(v)
    np.savez_compressed(os.path.join(HERE, "tiny_sn_init.npz"), **init)     # (a file of its own: each stays under 1 MiB)
    out = {"rng_state_after_init": init["rng_state_after_init"]}
    batch = synth.make_batch(B, 32, seed=4321)
    for k, v in batch.items():
        out["batch/%s" % k] = t2n(v)
    grabbed = {}
    real_step = trainer.dis_opt.step

    def grab_then_step(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            if p.grad is not None:
                grabbed[k] = t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = grab_then_step
    losses = []
    for it in range(2):
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, it)
        grabbed.clear()
        trainer.dis_update(*a)
        for k, v in grabbed.items():
            out["it%d/dgrad/%s" % (it, k)] = v
        for k, v in sn_state(trainer).items():
            out["it%d/after_dis/%s" % (it, k)] = t2n(v)
        trainer.gen_update(*a)
        for k, v in sn_state(trainer).items():
            out["it%d/after_gen/%s" % (it, k)] = t2n(v)
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
        losses.append(mg.read_losses(trainer))
    out["losses_json"] = np.frombuffer(json.dumps(losses).encode(), dtype=np.uint8)

    # gradient penalty + R1 (reference solver.py:337-350) on one D step from the same initialisation, iteration 15
    cfg_p = dict(cfg, gp_w=10.0, use_r1=True)
    trainer = mg.build_ref_solver(ref_solver, cfg_p)
    real_step = trainer.dis_opt.step
    grabbed = {}

    def grab_then_step_p(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            if p.grad is not None:
                grabbed[k] = t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = grab_then_step_p
    x_real = batch["x_real"].clone()                  # (the reference sets requires_grad on the tensor it is handed)
    trainer.dis_update(x_real, batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                       batch["label_trg"], cfg_p, 15)
    for k, v in grabbed.items():
        out["pen/dgrad/%s" % k] = v
    for k in ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1"):
        out["pen/%s" % k] = np.float64(float(getattr(trainer, k)))
    for k, v in sn_state(trainer).items():
        out["pen/after_dis/%s" % k] = t2n(v)
    np.savez_compressed(os.path.join(HERE, "tiny_sn_step.npz"), **out)
    print("tiny_sn_step.npz written; losses:", [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses])


if __name__ == "__main__":
    ref_solver, ref_nets, _, _, _ = mg.import_reference()
    gen_sn_ops(ref_nets)
    gen_tiny_sn(ref_solver)
