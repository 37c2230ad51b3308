"""What the make_golden_*.py recipes of the tiny Solver (32x32, B = 3, seed 1234, synth.make_batch(3, 32, seed=4321)) share: the
init record, the D-gradient grab in front of dis_opt.step, the two-iteration recording, the one-D-step penalties recording, the
one-ulp second run with its ``sens``, and the writer.  The reference is imported at run time (make_golden.import_reference); each
recipe adds its configuration, its hooks and its file names.

tests/tiny_solver.py replays these recordings; the argument tuple, the G-gradient sampler and the member names come from there, so
that both sides have one definition.  The order in which keys enter a record is the order of the archive's members: keep it."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden as mg  # noqa: E402  (import_reference, build_ref_solver, read_losses, checksum, t2n; synth)
import tiny_solver as ts  # noqa: E402  (step_args, sample_idx, member names)

synth = mg.synth
t2n = mg.t2n
BATCH_SEED = 4321
PENALTY_SCALARS = ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1")


def tiny_batch(seed=BATCH_SEED):
    return synth.make_batch(3, 32, seed=seed)


def json_bytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def batch_record(batch):
    return {ts.BATCH + k: t2n(v) for k, v in batch.items()}


def init_record(trainer, full=False):
    """The random stream after construction and the initial state_dicts of G and D: per key, in order, shape and (sum, sum of
    squares) -- or, ``full``, the tensors themselves (tiny_bn_init.npz / tiny_sn_init.npz)."""
    init = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    for net, mod in (("gen", trainer.gen), ("dis", trainer.dis)):
        sd = mod.state_dict()
        if full:
            init.update({"init/%s/%s" % (net, k): t2n(v) for k, v in sd.items()})
        else:
            init["init_keys/%s" % net] = json_bytes([[k, list(v.shape)] for k, v in sd.items()])
            init["init_sums/%s" % net] = np.array([mg.checksum(v) for v in sd.values()], dtype=np.float64)
    return init


def grab_then_step(trainer, prefix=""):
    """-> dict that dis_opt.step fills, in front of the step, with prefix + name -> gradient of every D parameter that has one."""
    grabbed = {}
    real_step = trainer.dis_opt.step

    def step(*args, **kw):
        for k, p in trainer.dis.named_parameters():
            if p.grad is not None:
                grabbed[prefix + k] = t2n(p.grad)
        return real_step(*args, **kw)
    trainer.dis_opt.step = step
    return grabbed


def two_iterations(ref_solver, cfg, batch, full_init=False, freeze=None, before_dis=None, after_dis=None, after_gen=None,
                   g_samples=True):
    """Two iterations of the reference's tiny Solver -> (init record, flat record ``out``, loss scalars per iteration, frozen names).
    ``freeze(dis)`` -> names it set requires_grad_(False) on; ``before_dis(it, trainer)``; ``after_dis(it, trainer, out)`` behind the
    D gradients of that step, ``after_gen(it, trainer, out)`` behind gen_update.  ``g_samples``: of iteration 0, G_SAMPLE evenly
    spread entries of every G gradient in one array and (largest magnitude, sum, sum of squares) of each in another, in the order
    of ``it0/ggrad_names`` (an archive member costs some 300 bytes whatever it holds)."""
    trainer = mg.build_ref_solver(ref_solver, cfg)
    init = init_record(trainer, full_init)
    frozen = freeze(trainer.dis) if freeze is not None else []
    out = {}
    grabbed = grab_then_step(trainer)
    losses, gnames, gsamples, gstats = [], [], [], []
    for it in range(2):
        a = ts.step_args(batch, cfg, it)
        grabbed.clear()
        if before_dis is not None:
            before_dis(it, trainer)
        trainer.dis_update(*a)
        for k, v in grabbed.items():
            out[(ts.DGRAD % it) + k] = v
        if after_dis is not None:
            after_dis(it, trainer, out)
        trainer.gen_update(*a)
        if after_gen is not None:
            after_gen(it, trainer, out)
        for k, p in trainer.gen.named_parameters():
            if g_samples and it == 0 and p.grad is not None:
                flat = p.grad.detach().reshape(-1)
                d = flat.double()
                gnames.append(k)
                gsamples.append(t2n(flat[ts.sample_idx(flat.numel())]))
                gstats.append([float(d.abs().max()), float(d.sum()), float((d * d).sum())])
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
        losses.append(mg.read_losses(trainer))
    if g_samples:
        out[ts.GGRAD] = np.concatenate(gsamples)
        out[ts.GSTAT] = np.array(gstats, dtype=np.float64)
        init[ts.GGRAD_NAMES] = json_bytes(gnames)
    return init, out, losses, frozen


def penalties(ref_solver, cfg, batch, grad_prefix="grad/", scalar_prefix="", x_scale=1.0, setup=None, iters=15):
    """One dis_update of the reference with the penalties ``cfg`` switches on, at iteration 15 (so that (iters + 1) % d_reg_every
    == 0 and the R1 term is live) -> (trainer, record): the random stream after construction, what ``setup(trainer, out)`` makes
    the step add, every D gradient grabbed in front of dis_opt.step, the four loss scalars."""
    trainer = mg.build_ref_solver(ref_solver, cfg)
    out = {"rng_state_after_init": torch.get_rng_state().numpy().copy()}
    grabbed = grab_then_step(trainer, grad_prefix)
    if setup is not None:
        setup(trainer, out)
    x_real = batch["x_real"].clone() * x_scale        # (the reference sets requires_grad on the tensor it is handed)
    trainer.dis_update(*ts.step_args(dict(batch, x_real=x_real), cfg, iters))
    out.update(grabbed)
    for k in PENALTY_SCALARS:
        out[scalar_prefix + k] = np.float64(float(getattr(trainer, k)))
    return trainer, out


def one_ulp(batch):
    """The batch with one ulp of noise on x_real: what a second run of the reference on it shows is ``sens``."""
    g = torch.Generator().manual_seed(5)
    return dict(batch, x_real=batch["x_real"] * (1 + 2.0 ** -23 * torch.randn(batch["x_real"].shape, generator=g)))


def deviation(a, b, floor=True):
    """Largest |a - b|.  Two fp32 recordings cannot show a deviation below the spacing of the values themselves (0 means "under one
    ulp", not "insensitive"): floored at one fp32 spacing of a's largest magnitude."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = float(np.abs(a - b).max())
    return max(d, float(np.spacing(np.float32(np.abs(a).max())))) if floor else d


def sensitivity(rec, rec2, losses, losses2, floors=None):
    """-> (key -> deviation between the two runs, for every member of ``rec`` but the G statistics and for ``it<n>/loss/<name>``;
    the largest per kind of member).  ``floors``: key -> a value whose fp32 spacing that key's deviation is not to go below."""
    sens, worst = {}, {}
    for k, v in rec.items():
        if k == ts.GSTAT:
            continue
        d = deviation(v, rec2[k], floor=v.dtype == np.float32)
        if floors and k in floors:
            d = max(d, float(np.spacing(np.float32(floors[k]))))
        sens[k] = d
        kind = "/".join(k.split("/")[:2])
        worst[kind] = max(worst.get(kind, 0.0), d)
    for it in range(len(losses)):
        for k in losses[it]:
            sens["it%d/loss/%s" % (it, k)] = deviation(losses[it][k], losses2[it][k])
    return sens, worst


def assemble(init, batch, rec, losses, frozen=None):
    """init record | batch | recording | losses_json [| frozen_json], in the archives' member order."""
    out = dict(init)
    out.update(batch_record(batch))
    out.update(rec)
    out["losses_json"] = json_bytes(losses)
    if frozen is not None:
        out["frozen_json"] = json_bytes(frozen)
    return out


def write_with_sens(name, label, batch, first, second, floors=None, extra=None):
    """The archive of a recording with ``sens_json``: ``first`` / ``second`` are what two_iterations returned for ``batch`` and for
    one_ulp(batch); ``extra`` members go between frozen_json and sens_json."""
    init, rec, losses, frozen = first
    out = assemble(init, batch, rec, losses, frozen)
    out.update(extra or {})
    sens, worst = sensitivity(rec, second[1], losses, second[2], floors)
    out["sens_json"] = json_bytes(sens)
    print("%s: sensitivity (largest deviation per kind):" % label, {k: "%.2e" % v for k, v in sorted(worst.items())},
          "losses", ["%.2e" % max(sens["it%d/loss/%s" % (it, k)] for k in losses[it]) for it in range(2)])
    size = write(name, out)
    print("%s.npz written (%d bytes); frozen: %s; losses: %s" % (name, size, frozen,
                                                                 [(l["loss_dis_all"], l["loss_gen_total"]) for l in losses]))


def write(name, out, limit=True):
    """tests/golden/<name>.npz; ``limit``: it stays below tiny_bn_step.npz.  -> its size."""
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if limit:
        assert size < os.path.getsize(os.path.join(HERE, "tiny_bn_step.npz")), (path, size)
    return size
