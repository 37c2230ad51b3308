"""The tiny Solver (32x32, B = 3, seed 1234) replayed against a ``tiny_*.npz`` recording of the imported reference: what every
``gen.*`` / ``dis.*`` option's test shares.  Imported like tests/guarded_alloc.py; no conftest, no fixture.

tests/golden/tiny_record.py writes the recordings and imports from here what both sides must agree on: the argument tuple of
``dis_update`` / ``gen_update``, which entries of a G gradient are kept and the names of the archive members.  Importing this module
therefore needs neither the built library nor the package: ``hipdwc`` and ``solver`` are imported where they are used.

The comparison itself is three functions on plain tensors and floats (check_dgrads, check_losses, check_ggrads), held in place by
tests/test_tiny_solver_harness.py without a GPU; ``two_iterations`` and ``bf16_iteration0`` drive the HIP Solver through them.
The bounds are an argument (``Bounds``): SENS_BOUNDS for the recordings with a ``sens_json``, FIXED_BOUNDS for the older bn / sn ones."""
import collections
import contextlib
import json
import os

import numpy as np
import torch

T = torch.from_numpy
DEV = "cuda:0"
G_SAMPLE = 32
SENS_MULTIPLE = 16

# ---------------------------------------------------------------------------------------------------------------------------------
# shared with the recorder
# ---------------------------------------------------------------------------------------------------------------------------------
BATCH = "batch/"
DGRAD = "it%d/dgrad/"
GGRAD, GSTAT, GGRAD_NAMES = "it0/ggrad", "it0/gstat", "it0/ggrad_names"


def step_args(batch, cfg, it):
    """The arguments of Solver.dis_update / gen_update."""
    return (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"], batch["label_trg"],
            cfg, it)


def sample_idx(n):
    """Element numbers of a flattened n-element G gradient that a recording keeps (at most G_SAMPLE, evenly spread)."""
    return torch.arange(n) if n <= G_SAMPLE else (torch.arange(G_SAMPLE, dtype=torch.int64) * n) // G_SAMPLE


def checksum(t):
    t = t.detach().double()
    return [float(t.sum()), float((t * t).sum())]


def batch_of(npz, device="cpu"):
    return {k[len(BATCH):]: T(npz[k]).to(device) for k in npz.files if k.startswith(BATCH)}


# ---------------------------------------------------------------------------------------------------------------------------------
# recordings
# ---------------------------------------------------------------------------------------------------------------------------------
class Fixture:
    """A ``tiny_*.npz`` archive (``npz``) with its JSON members decoded; a member the archive does not hold is None."""

    def __init__(self, golden_dir, name):
        self.name = name
        self.path = os.path.join(golden_dir, name + ".npz")
        self.npz = np.load(self.path)
        self.losses, self.sens, self.gnames = self._json("losses_json"), self._json("sens_json"), self._json(GGRAD_NAMES)
        frozen = self._json("frozen_json")
        self.frozen = None if frozen is None else set(frozen)

    def _json(self, key):
        return json.loads(bytes(self.npz[key]).decode()) if key in self.npz.files else None

    def batch(self, device="cpu"):
        return batch_of(self.npz, device)

    def dgrads(self, it):
        return {k[len(DGRAD % it):]: T(self.npz[k]) for k in self.npz.files if k.startswith(DGRAD % it)}


def load(golden_dir, name):
    return Fixture(golden_dir, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the Solver under test
# ---------------------------------------------------------------------------------------------------------------------------------
def build(cfg, device="cpu", seed=1234):
    from solver import Solver
    torch.manual_seed(seed)
    s = Solver(cfg, torch.device(device), None)
    if device != "cpu":
        s = s.to(device)
    s.copy_nets()
    return s


def check_init(s, fx):
    """Same state_dict keys and shapes, in order, and the checksums of the reference's initial tensors."""
    for net, mod in (("gen", s.gen), ("dis", s.dis)):
        want = json.loads(bytes(fx.npz["init_keys/%s" % net]).decode())
        sd = mod.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == want, net
        sums = fx.npz["init_sums/%s" % net]
        for (k, v), w in zip(sd.items(), sums):
            got = checksum(v.cpu())
            assert abs(got[0] - w[0]) <= 1e-9 * max(1.0, abs(w[0])) and abs(got[1] - w[1]) <= 1e-9 * max(1.0, abs(w[1])), (net, k, got, w)


def grab_dis(s):
    """-> dict that every dis_opt.step refills, in front of the step, with name -> gradient of each D parameter (None: no gradient)."""
    grabbed = {}
    real_step = s.dis_opt.step

    def grab(*a, **k):
        grabbed.clear()
        grabbed.update({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in s.dis.named_parameters()})
        return real_step(*a, **k)
    s.dis_opt.step = grab
    return grabbed


def gen_grads(s):
    """name -> gradient that gen_update left on each G parameter.  Convolution biases in front of an instance norm are flagged
    ``_dwc_zero_grad`` and get no gradient tensor -- the identically-zero gradient that the reference computes as rounding noise --:
    zeros stand for it."""
    out = {}
    for k, p in s.gen.named_parameters():
        if p.grad is not None:
            out[k] = p.grad
        elif getattr(p, "_dwc_zero_grad", False):
            out[k] = torch.zeros_like(p)
    return out


def read_losses(s, names):
    return {k: float(torch.as_tensor(getattr(s, k)).detach()) for k in names}


@contextlib.contextmanager
def host_noise():
    from hipdwc import host
    host.set_noise(host.HostNoise())
    try:
        yield
    finally:
        host.set_noise(host.DeviceNoise())


@contextlib.contextmanager
def precision(p):
    from hipdwc import ops
    ops.set_precision(p)
    try:
        yield
    finally:
        ops.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds and the three comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
# dgrad(it, largest |reference gradient|, sens of the key) / loss(it, reference value, sens of the key) / ggrad(largest |reference
# gradient|) -> the absolute limit (ggrad None: the recording holds no G gradients).  ``frozen``, the D parameters outside the
# recorded gradients: "zeros" -- exactly the recording's frozen_json, each None or all zeros; "none" -- the same keys, each None;
# "rest" -- whatever the recording does not hold, each None.
Bounds = collections.namedtuple("Bounds", "dgrad loss ggrad frozen")

SENS_BOUNDS = Bounds(dgrad=lambda it, amax, sens: 2e-3 * amax + 1e-6 if it == 0 else SENS_MULTIPLE * sens,
                     loss=lambda it, v, sens: 2e-4 * max(1.0, abs(v)) if it == 0 else SENS_MULTIPLE * sens,
                     ggrad=lambda amax: 5e-3 * amax + 1e-6, frozen="zeros")
FIXED_BOUNDS = Bounds(dgrad=lambda it, amax, sens: (2e-3, 2e-2)[it] * amax + 1e-6,
                      loss=lambda it, v, sens: (2e-4, 5e-3)[it] * max(1.0, abs(v)),
                      ggrad=None, frozen="zeros")


def _worst(worst, key, ratio):
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), ratio)


def ratios(worst, ggrad=False):
    """``worst`` for a test's summary line; the sampled G gradients' share of their limit (no ratio to ``sens``) on request."""
    return {k: "%.2f" % v for k, v in sorted(worst.items()) if ggrad or k != "it0 ggrad / limit"}


def check_dgrads(fx, it, grabbed, bounds, worst=None):
    """The D gradients of iteration ``it`` (name -> tensor or None, as grab_dis leaves them) against the recording."""
    ref_g = fx.dgrads(it)
    frozen = set(grabbed) - set(ref_g) if bounds.frozen == "rest" else fx.frozen
    assert set(ref_g) | frozen == set(grabbed) and not set(ref_g) & frozen
    for k in sorted(frozen):
        assert grabbed[k] is None or (bounds.frozen == "zeros" and not grabbed[k].any()), k
    for k, want in ref_g.items():
        assert grabbed[k] is not None, k
        got, want = grabbed[k].detach().double().cpu(), want.double()
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert not torch.isnan(got).any(), "it%d dgrad %s: NaN" % (it, k)
        err = (got - want).abs().max().item()
        sk = fx.sens[(DGRAD % it) + k] if fx.sens else None
        lim = bounds.dgrad(it, want.abs().max().item(), sk)
        if sk is None:
            print("it%d dgrad %s: max err %.3e, limit %.3e" % (it, k, err, lim))
        else:
            _worst(worst, "it%d dgrad" % it, err / sk)
            print("it%d dgrad %s: max err %.3e, limit %.3e, ratio to sens %.2f" % (it, k, err, lim, err / sk))
        assert err <= lim, "it%d dgrad %s: max err %.3e > %.3e" % (it, k, err, lim)


def check_losses(fx, it, got, bounds, worst=None):
    """The loss scalars after iteration ``it`` (name -> float) against the recording."""
    want = fx.losses[it]
    assert set(got) == set(want)
    for k, v in want.items():
        sk = fx.sens["it%d/loss/%s" % (it, k)] if fx.sens else None
        lim = bounds.loss(it, v, sk)
        if sk is None:
            print("it%d %s: %.7g against %.7g, limit %.3e" % (it, k, got[k], v, lim))
        else:
            _worst(worst, "it%d loss" % it, abs(got[k] - v) / sk)
            print("it%d %s: %.7g against %.7g, limit %.3e, ratio to sens %.2f" % (it, k, got[k], v, lim, abs(got[k] - v) / sk))
        assert abs(got[k] - v) <= lim, (it, k, got[k], v, lim)


def check_ggrads(fx, grads, bounds, worst=None):
    """The G gradients of iteration 0 (name -> tensor, as gen_grads leaves them) against the recorded samples."""
    assert sorted(grads) == sorted(fx.gnames)
    want = fx.npz[GGRAD]
    off = 0
    for k, (amax, _, _) in zip(fx.gnames, fx.npz[GSTAT]):
        flat = grads[k].detach().reshape(-1).cpu()
        idx = sample_idx(flat.numel())
        w = T(want[off:off + idx.numel()])
        off += idx.numel()
        err = (flat[idx] - w).abs().max().item()
        lim = bounds.ggrad(amax)
        _worst(worst, "it0 ggrad / limit", err / lim)
        print("it0 ggrad %s: max err %.3e, limit %.3e" % (k, err, lim))
        assert err <= lim, "it0 ggrad %s: max err %.3e > %.3e" % (k, err, lim)
    assert off == want.shape[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the replays
# ---------------------------------------------------------------------------------------------------------------------------------
def two_iterations(fx, cfg, bounds=SENS_BOUNDS, init=True, before_loop=None, after_dis=None, after_gen=None, worst=None):
    """Two iterations of the HIP Solver (fp32, HostNoise: the reference's random stream) against recording ``fx``: the
    initialisation (``init``: the recording holds its checksums), the D gradients of both D steps, the sampled G gradients of
    iteration 0 where ``bounds`` has a limit for them, the loss scalars.  ``before_loop(s)`` runs after construction,
    ``after_dis(it, s)`` / ``after_gen(it, s)`` behind the two updates.  -> ``worst``, largest ratios to ``sens`` (filled in place:
    a caller that hands in the dict still has it when an assertion fails)."""
    worst = {} if worst is None else worst
    with precision("fp32"), host_noise():
        s = build(cfg, DEV)
        if init:
            check_init(s, fx)
        assert torch.equal(torch.get_rng_state(), T(fx.npz["rng_state_after_init"]))
        batch = fx.batch(DEV)
        grabbed = grab_dis(s)
        if before_loop is not None:
            before_loop(s)
        for it in range(2):
            a = step_args(batch, cfg, it)
            s.dis_update(*a)
            if after_dis is not None:
                after_dis(it, s)
            check_dgrads(fx, it, grabbed, bounds, worst)
            s.gen_update(*a)
            if after_gen is not None:
                after_gen(it, s)
            if it == 0 and bounds.ggrad is not None:
                check_ggrads(fx, gen_grads(s), bounds, worst)
            s.smooth_moving()
            s.update_learning_rate()
            s.update_attention_status(it)
            check_losses(fx, it, read_losses(s, fx.losses[it]), bounds, worst)
    return worst


def bf16_iteration0(fx, cfg):
    """Iteration 0 under bf16 activations: the 16 loss scalars are finite and within the bound the whole-iteration bf16 comparison
    against the reference at the c2 shape applies (tests/test_bf16_parity.py::test_bf16_full_iteration_b128): every scalar within
    3e-2 of max(1, |value|), loss_dis_all and loss_gen_total within 2e-2 relative."""
    want = fx.losses[0]
    assert len(want) == 16
    with precision("bf16"), host_noise():
        s = build(cfg, DEV)
        a = step_args(fx.batch(DEV), cfg, 0)
        s.dis_update(*a)
        s.gen_update(*a)
        torch.cuda.synchronize()
        got = read_losses(s, want)
        for k, v in want.items():
            print("%s: %.6g against %.6g (%.2e of max(1, |value|))" % (k, got[k], v, abs(got[k] - v) / max(1.0, abs(v))))
            assert np.isfinite(got[k]), k
            assert abs(got[k] - v) <= 3e-2 * max(1.0, abs(v)), (k, got[k], v)
        for k in ("loss_dis_all", "loss_gen_total"):
            assert abs(got[k] - want[k]) <= 2e-2 * abs(want[k]), (k, got[k], want[k])
