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
    cfg = synth.make_config(image_size=32, tiny=True)
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
    np.savez_compressed(os.path.join(HERE, "bn_ops.npz"), **out)
    print("bn_ops.npz:", len(out), "arrays")


def run_tiny(ref_solver, cfg, batch, call_stats=None):
    """Two iterations of the reference's tiny Solver with the BN-fed biases frozen -> (trainer after construction's init record,
    flat record of losses / D gradients / buffers).  ``call_stats``: a list that receives, for every BN call of the FIRST dis_update,
    (module name, batch mean, unbiased batch variance)."""
    trainer = mg.build_ref_solver(ref_solver, cfg)
    init = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    for k, v in trainer.gen.state_dict().items():
        init["init/gen/%s" % k] = t2n(v)
    for k, v in trainer.dis.state_dict().items():
        init["init/dis/%s" % k] = t2n(v)
    frozen = freeze_bn_fed_biases(trainer.dis)
    out = {}
    grabbed = {}
    real_step = trainer.dis_opt.step

    def grab_then_step(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            if p.grad is not None:
                grabbed[k] = t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = grab_then_step
    hooks = []
    if call_stats is not None:
        for n, m in bn_modules(trainer.dis):
            hooks.append(m.register_forward_pre_hook(
                lambda mod, inp, n=n: call_stats.append((n, inp[0].detach().double().mean((0, 2, 3)),
                                                         inp[0].detach().double().var((0, 2, 3), unbiased=True)))))
    losses = []
    for it in range(2):
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, it)
        grabbed.clear()
        trainer.dis_update(*a)
        for h in hooks:
            h.remove()
        hooks = []
        for k, v in grabbed.items():
            out["it%d/dgrad/%s" % (it, k)] = v
        for k, v in bn_state(trainer).items():
            out["it%d/after_dis/%s" % (it, k)] = t2n(v)
        trainer.gen_update(*a)
        for k, v in bn_state(trainer).items():
            out["it%d/after_gen/%s" % (it, k)] = t2n(v)
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
        losses.append(mg.read_losses(trainer))
    return init, out, losses, frozen


def replay(r0_mean, r0_var, stats, order):
    rm, rv = r0_mean.double().clone(), r0_var.double().clone()
    for j in order:
        rm = (1 - MOMENTUM) * rm + MOMENTUM * stats[j][0]
        rv = (1 - MOMENTUM) * rv + MOMENTUM * stats[j][1]
    return rm, rv


def gen_tiny_bn(ref_solver):
    cfg = tiny_bn_config()
    B = 3
    batch = synth.make_batch(B, 32, seed=4321)
    calls = []
    init, rec, losses, frozen = run_tiny(ref_solver, cfg, batch, calls)
    np.savez_compressed(os.path.join(HERE, "tiny_bn_init.npz"), **init)     # (a file of its own: each stays under 1 MiB)
    out = {"rng_state_after_init": init["rng_state_after_init"]}
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
    worst = {}
    for k, v in rec.items():
        d = float(np.abs(v.astype(np.float64) - rec2[k].astype(np.float64)).max())
        if v.dtype == np.float32:
            # two fp32 recordings cannot show a deviation below the spacing of the values themselves (0 here means "under one
            # ulp", not "insensitive"): floored at one fp32 spacing of the key's largest magnitude
            d = max(d, float(np.spacing(np.float32(np.abs(v).max()))))
        out["sens/%s" % k] = np.float64(d)
        kind = k.split("/")[0] + "/" + k.split("/")[1]
        worst[kind] = max(worst.get(kind, 0.0), d)
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
    np.savez_compressed(os.path.join(HERE, "tiny_bn_step.npz"), **out)
    print("tiny_bn_step.npz written; frozen:", frozen, "losses:", [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses])


if __name__ == "__main__":
    ref_solver, ref_nets, _, _, _ = mg.import_reference()
    gen_bn_ops(ref_nets)
    gen_tiny_bn(ref_solver)
