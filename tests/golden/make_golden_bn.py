#!/usr/bin/env python3
"""Record the batch-normalisation fixtures (``norm='bn'``, reference networks.py:542 nn.BatchNorm2d) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); the tests read the .npz
files it writes:

    python tests/golden/make_golden_bn.py          # bn_ops.npz, tiny_bn_init.npz, tiny_bn_step.npz; seconds

* bn_ops.npz -- reference Conv2dBlock(norm='bn') cases, reflect padding: the parameters; three consecutive calls on x_a, x_b, x_a
  (B = 2): y of each call, the running statistics after each call, and dx_a (both x_a calls added, as autograd adds them), dx_b,
  dw, dgamma, dbeta of sum_j <y_j, gy_j> with the three gy_j.
* tiny_bn_init.npz -- the tiny Solver with dis.norm = 'bn' (32x32, B = 3): the initial state_dicts and the random stream after
  construction.
* tiny_bn_step.npz -- the same Solver, two iterations: every loss scalar, every D gradient of both D steps, every BN buffer after
  each dis_update and gen_update.  The convolution biases that feed a BatchNorm are frozen first: their true gradient is zero and
  the reference's rounding noise there becomes +-lr Adam steps that move everything recorded after iteration 0.  ``sens/<key>``:
  the largest deviation of that key in a second run of the reference on x_real * (1 + 2^-23 randn) -- what one ulp of input
  noise does to the reference itself, floored at one fp32 spacing of the key's largest value (what two fp32 recordings can resolve);
  the test's iteration-1 buffer tolerance is a multiple of it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tiny_record as tr  # noqa: E402  (the recording itself; make_golden's import_reference)

t2n = tr.t2n

# (name, B, Cin, Cout, H, k, stride, pad, activation) -- reflect padding; tests/test_batch_norm.py BN_CASES
BN_CASES = [
    ("k4s2_lrelu", 2, 16, 32, 16, 4, 2, 1, "lrelu"),       # the discriminator's layer
    ("k3s1_relu", 2, 8, 16, 12, 3, 1, 1, "relu"),
    ("k4s2_none", 2, 8, 16, 8, 4, 2, 1, "none"),
    ("k3s1_tanh", 2, 16, 8, 10, 3, 1, 1, "tanh"),           # the norm unfused, then the activation
]
MOMENTUM = 0.1
BUF_REL = 1e-5         # the test's iteration-0 buffer tolerance (relative to the buffer's largest magnitude)


def tiny_bn_config():
    cfg = tr.synth.make_config(image_size=32, tiny=True)
    cfg["dis"]["norm"] = "bn"
    return cfg


def bn_modules(dis):
    return [(n, m) for n, m in dis.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]


def bn_state(trainer):
    return {k: v for k, v in trainer.dis.state_dict().items()
            if k.endswith("running_mean") or k.endswith("running_var") or k.endswith("num_batches_tracked")}


def freeze_bn_fed_biases(dis):
    """requires_grad_(False) on every convolution bias whose output goes straight into a BatchNorm."""
    frozen = []
    for n, m in dis.named_modules():
        if isinstance(getattr(m, "norm", None), torch.nn.BatchNorm2d) and getattr(m.conv, "bias", None) is not None:
            m.conv.bias.requires_grad_(False)
            frozen.append(n + ".conv.bias")
    return frozen


def gen_bn_ops(ref_nets):
    g = torch.Generator().manual_seed(91)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    out = {}
    for name, B, ci, co, H, k, s, p, act in BN_CASES:
        blk = ref_nets.Conv2dBlock(ci, co, k, s, p, norm="bn", activation=act, pad_type="reflect")
        with torch.no_grad():
            blk.conv.weight.copy_(rnd(co, ci, k, k) * 0.2)
            blk.conv.bias.copy_(rnd(co) * 0.1)
            blk.norm.weight.copy_(torch.rand(co, generator=g) + 0.5)
            blk.norm.weight[1].neg_()                         # a negative scale
            blk.norm.bias.copy_(rnd(co) * 0.1)
        rec = {"w": blk.conv.weight, "b": blk.conv.bias, "bn_w": blk.norm.weight, "bn_b": blk.norm.bias}
        xa = rnd(B, ci, H, H).requires_grad_(True)
        xb = (rnd(B, ci, H, H) * 1.5 + 0.3).requires_grad_(True)
        ys = []
        for j, x in enumerate((xa, xb, xa)):
            ys.append(blk(x))                                 # training mode: this call's batch statistics, one buffer update
            rec["running_mean%d" % (j + 1)] = blk.norm.running_mean.clone()
            rec["running_var%d" % (j + 1)] = blk.norm.running_var.clone()
        gys = [rnd(*ys[0].shape) for _ in range(3)]
        sum((y * gy).sum() for y, gy in zip(ys, gys)).backward()
        rec.update({"xa": xa, "xb": xb, "dxa": xa.grad, "dxb": xb.grad, "dw": blk.conv.weight.grad, "dbn_w": blk.norm.weight.grad,
                    "dbn_b": blk.norm.bias.grad})
        for j in range(3):
            rec["y%d" % (j + 1)], rec["gy%d" % (j + 1)] = ys[j], gys[j]
        for kk, v in rec.items():
            out["%s/%s" % (name, kk)] = t2n(v)
    tr.write("bn_ops", out, limit=False)
    print("bn_ops.npz:", len(out), "arrays")


def record_bn(ref_solver, cfg, batch, call_stats=None):
    """The shared two-iteration recording with the BN-fed biases frozen and every BN buffer recorded after each dis_update and
    gen_update.  ``call_stats``: a list that receives, for every BN call of the FIRST dis_update, (module name, batch mean,
    unbiased batch variance)."""
    hooks = []

    def watch_calls(it, trainer):
        if it == 0 and call_stats is not None:
            for n, m in bn_modules(trainer.dis):
                hooks.append(m.register_forward_pre_hook(
                    lambda mod, inp, n=n: call_stats.append((n, inp[0].detach().double().mean((0, 2, 3)),
                                                             inp[0].detach().double().var((0, 2, 3), unbiased=True)))))

    def buffers(when):
        def record(it, trainer, out):
            while hooks:
                hooks.pop().remove()
            for k, v in bn_state(trainer).items():
                out["it%d/after_%s/%s" % (it, when, k)] = t2n(v)
        return record
    return tr.two_iterations(ref_solver, cfg, batch, full_init=True, freeze=freeze_bn_fed_biases, before_dis=watch_calls,
                             after_dis=buffers("dis"), after_gen=buffers("gen"), g_samples=False)


def replay(r0_mean, r0_var, stats, order):
    rm, rv = r0_mean.double().clone(), r0_var.double().clone()
    for j in order:
        rm = (1 - MOMENTUM) * rm + MOMENTUM * stats[j][0]
        rv = (1 - MOMENTUM) * rv + MOMENTUM * stats[j][1]
    return rm, rv


def gen_tiny_bn(ref_solver):
    cfg = tiny_bn_config()
    batch = tr.tiny_batch()
    calls = []
    init, rec, losses, frozen = record_bn(ref_solver, cfg, batch, calls)
    tr.write("tiny_bn_init", init, limit=False)     # (a file of its own: each stays under 1 MiB)
    out = tr.assemble({"rng_state_after_init": init["rng_state_after_init"]}, batch, rec, losses, frozen)

    # what one ulp of input noise does to the reference itself
    _, rec2, losses2, _ = record_bn(ref_solver, cfg, tr.one_ulp(batch))
    sens, worst = tr.sensitivity(rec, rec2, losses, losses2)
    for k in rec:
        out["sens/%s" % k] = np.float64(sens[k])
    for it in range(2):
        out["sens/it%d/losses" % it] = np.float64(max(abs(losses[it][k] - losses2[it][k]) for k in losses[it]))
    print("sensitivity (largest deviation per kind):", {k: "%.2e" % v for k, v in sorted(worst.items())},
          "losses", [float(out["sens/it%d/losses" % it]) for it in range(2)])

    # the recorded iteration-0 buffers must tell a wrong update order from the right one: the reference's D step calls
    # fake, real, fake1, real; the one-pass layout is [fake | fake1 | real] = calls (0, 2, 1/3)
    per_layer = {}
    for n, m, v in calls:
        per_layer.setdefault(n, []).append((m, v))
    for n, st in per_layer.items():
        assert len(st) == 4, (n, len(st))
        seg = [st[0], st[2], st[1]]                           # segments fake, fake1, real
        assert torch.allclose(st[1][0], st[3][0], rtol=0, atol=0), "the two x_real calls see the same batch"
        r0m, r0v = torch.from_numpy(init["init/dis/%s.running_mean" % n]), torch.from_numpy(init["init/dis/%s.running_var" % n])
        want_m = torch.from_numpy(rec["it0/after_dis/%s.running_mean" % n]).double()
        want_v = torch.from_numpy(rec["it0/after_dis/%s.running_var" % n]).double()
        tol_m, tol_v = BUF_REL * float(want_m.abs().max()), BUF_REL * float(want_v.abs().max())
        rm, rv = replay(r0m, r0v, seg, (0, 2, 1, 2))
        assert float((rm - want_m).abs().max()) <= tol_m and float((rv - want_v).abs().max()) <= tol_v, n
        for wrong in ((0, 1, 2, 2), (0, 1, 2)):
            rm, rv = replay(r0m, r0v, seg, wrong)
            ratio = max(float((rm - want_m).abs().max()) / tol_m, float((rv - want_v).abs().max()) / tol_v)
            print("%s: order %s is off by %.0f x the tolerance" % (n, wrong, ratio))
            assert ratio >= 100, (n, wrong, ratio)
    tr.write("tiny_bn_step", out, limit=False)
    print("tiny_bn_step.npz written; frozen:", frozen, "losses:", [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses])


if __name__ == "__main__":
    ref_solver, ref_nets, _, _, _ = tr.mg.import_reference()
    gen_bn_ops(ref_nets)
    gen_tiny_bn(ref_solver)
