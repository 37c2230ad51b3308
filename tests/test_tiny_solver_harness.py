"""tests/tiny_solver.py holds the comparisons of every tiny-Solver test against its recording; this file holds THEM in place, without
a GPU.  Each comparison is fed the recording's own values (passes), then one value moved by 1.01 x its limit (AssertionError) and
by 0.99 x (passes).  The limits are written out here as the formulas the tests' docstrings state -- not read from the module:
  SENS_BOUNDS   iteration 0: D gradients 2e-3 max|g| + 1e-6, losses 2e-4 max(1, |v|), sampled G gradients 5e-3 max|g| + 1e-6;
                iteration 1: D gradients and losses 16 x sens[key];
  FIXED_BOUNDS  D gradients 2e-3 / 2e-2 of max|g| + 1e-6, losses 2e-4 / 5e-3 of max(1, |v|)   (iteration 0 / 1).
Values are moved in float64 (the comparisons convert to it): 1 % of 16 fp32 spacings is not a float32 step."""
import functools

import pytest
import torch

import test_gan_solver
import test_lrelu_solver
import test_zero_pad_solver
import tiny_solver as ts

CONFIGS = {"tiny_zero": test_zero_pad_solver._config,
           "tiny_lrelu_in": lambda: test_lrelu_solver._config("in"), "tiny_lrelu_ln": lambda: test_lrelu_solver._config("ln"),
           "tiny_nsgan": lambda: test_gan_solver._config("tiny_nsgan"), "tiny_wgan_gp": lambda: test_gan_solver._config("tiny_wgan_gp")}
SENS_CASES = [("tiny_zero", ts.SENS_BOUNDS), ("tiny_lrelu_in", ts.SENS_BOUNDS), ("tiny_wgan_gp", test_gan_solver.BOUNDS)]


@functools.lru_cache(maxsize=None)
def _gen_numel(name):
    return {k: p.numel() for k, p in ts.build(CONFIGS[name]()).gen.named_parameters()}


def _own_dgrads(fx, it):
    grabbed = {k: g.double() for k, g in fx.dgrads(it).items()}
    grabbed.update({k: None for k in fx.frozen})
    return grabbed


def _own_ggrads(fx):
    """Full-size G gradients that hold the recorded samples where the recording took them."""
    grads, off = {}, 0
    for k in fx.gnames:
        flat = torch.zeros(_gen_numel(fx.name)[k], dtype=torch.float64)
        idx = ts.sample_idx(flat.numel())
        flat[idx] = ts.T(fx.npz[ts.GGRAD][off:off + idx.numel()]).double()
        off += idx.numel()
        grads[k] = flat
    return grads


def _moved(values, key, by):
    out = dict(values)
    if torch.is_tensor(out[key]):
        out[key] = out[key].clone()
        out[key].view(-1)[0] += by
    else:
        out[key] += by
    return out


def _at_the_limit(check, values, key, lim):
    """``check(values)`` passes with values[key] (its first element) 0.99 x lim off, on either side, and raises 1.01 x lim off."""
    for sign in (1.0, -1.0):
        check(_moved(values, key, sign * 0.99 * lim))
        with pytest.raises(AssertionError):
            check(_moved(values, key, sign * 1.01 * lim))


@pytest.mark.parametrize("name,bounds", SENS_CASES, ids=[c[0] for c in SENS_CASES])
def test_sens_bounds_hold_where_the_tests_say(golden_dir, name, bounds):
    fx = ts.load(golden_dir, name)
    for it in range(2):
        own = _own_dgrads(fx, it)
        ts.check_dgrads(fx, it, own, bounds)
        k, g = next(iter(fx.dgrads(it).items()))
        lim = 2e-3 * g.abs().max().item() + 1e-6 if it == 0 else 16 * fx.sens["it%d/dgrad/%s" % (it, k)]
        _at_the_limit(lambda v: ts.check_dgrads(fx, it, v, bounds), own, k, lim)

        own = dict(fx.losses[it])
        ts.check_losses(fx, it, own, bounds)
        for k in ("loss_dis_all", "loss_gen_total"):
            v = fx.losses[it][k]
            lim = 2e-4 * max(1.0, abs(v)) if it == 0 else 16 * fx.sens["it%d/loss/%s" % (it, k)]
            _at_the_limit(lambda v: ts.check_losses(fx, it, v, bounds), own, k, lim)

    own = _own_ggrads(fx)
    ts.check_ggrads(fx, own, bounds)
    for row in (0, len(fx.gnames) - 1):
        lim = 5e-3 * fx.npz["it0/gstat"][row][0] + 1e-6
        _at_the_limit(lambda v: ts.check_ggrads(fx, v, bounds), own, fx.gnames[row], lim)


def test_fixed_bounds_hold_where_the_tests_say(golden_dir):
    fx = ts.load(golden_dir, "tiny_bn_step")
    assert fx.sens is None and fx.gnames is None and ts.FIXED_BOUNDS.ggrad is None
    for it in range(2):
        own = _own_dgrads(fx, it)
        ts.check_dgrads(fx, it, own, ts.FIXED_BOUNDS)
        k, g = next(iter(fx.dgrads(it).items()))
        _at_the_limit(lambda v: ts.check_dgrads(fx, it, v, ts.FIXED_BOUNDS), own, k, (2e-3, 2e-2)[it] * g.abs().max().item() + 1e-6)
        own = dict(fx.losses[it])
        ts.check_losses(fx, it, own, ts.FIXED_BOUNDS)
        for k in ("loss_dis_all", "loss_gen_total"):
            _at_the_limit(lambda v: ts.check_losses(fx, it, v, ts.FIXED_BOUNDS), own, k, (2e-4, 5e-3)[it] * max(1.0, abs(fx.losses[it][k])))


@pytest.mark.parametrize("name,bounds", SENS_CASES + [("tiny_bn_step", ts.FIXED_BOUNDS)], ids=[c[0] for c in SENS_CASES] + ["tiny_bn_step"])
def test_key_sets_nan_and_shape(golden_dir, name, bounds):
    fx = ts.load(golden_dir, name)
    own = _own_dgrads(fx, 0)
    k = next(iter(fx.dgrads(0)))
    dropped = dict(own)
    del dropped[k]
    wrong = {"dropped": dropped, "extra": dict(own, bogus=own[k]), "without a gradient": dict(own, **{k: None}),
             "NaN": _moved(own, k, float("nan")), "shape": dict(own, **{k: own[k].reshape(-1)[:1]})}
    for what, grabbed in wrong.items():
        with pytest.raises(AssertionError):
            ts.check_dgrads(fx, 0, grabbed, bounds)
            pytest.fail("a D gradient %s went through" % what)
    losses = dict(fx.losses[0])
    del losses["loss_kl_x"]
    with pytest.raises(AssertionError):
        ts.check_losses(fx, 0, losses, bounds)
    with pytest.raises(AssertionError):
        ts.check_losses(fx, 0, dict(fx.losses[0], loss_bogus=0.0), bounds)


def test_frozen_parameters(golden_dir):
    """A frozen parameter: no gradient under "none" (gan); none or exact zeros under "zeros" (lrelu 'in', bn); under "rest" (sn)
    every parameter outside the recording has none."""
    fx = ts.load(golden_dir, "tiny_wgan_gp")
    assert fx.frozen == {"cnns_src.0.bias", "cnns_src.1.bias"}
    zeros = dict(_own_dgrads(fx, 0), **{"cnns_src.0.bias": torch.zeros(1)})
    with pytest.raises(AssertionError):
        ts.check_dgrads(fx, 0, zeros, test_gan_solver.BOUNDS)
    ts.check_dgrads(fx, 0, zeros, ts.SENS_BOUNDS)
    with pytest.raises(AssertionError):
        ts.check_dgrads(fx, 0, dict(zeros, **{"cnns_src.0.bias": torch.full((1,), 1e-30)}), ts.SENS_BOUNDS)

    fx = ts.load(golden_dir, "tiny_sn_step")
    rest = ts.FIXED_BOUNDS._replace(frozen="rest")
    assert fx.frozen is None
    own = {k: g.double() for k, g in fx.dgrads(0).items()}
    ts.check_dgrads(fx, 0, dict(own, weight_u=None), rest)
    with pytest.raises(AssertionError):
        ts.check_dgrads(fx, 0, dict(own, weight_u=torch.zeros(1)), rest)
    k = next(iter(own))
    with pytest.raises(AssertionError):
        ts.check_dgrads(fx, 0, dict(own, **{k: None}), rest)


def test_ggrad_names_and_length(golden_dir):
    fx = ts.load(golden_dir, "tiny_zero")
    own = _own_ggrads(fx)
    dropped = dict(own)
    del dropped[fx.gnames[0]]
    with pytest.raises(AssertionError):
        ts.check_ggrads(fx, dropped, ts.SENS_BOUNDS)
    with pytest.raises(AssertionError):
        ts.check_ggrads(fx, dict(own, bogus=own[fx.gnames[0]]), ts.SENS_BOUNDS)
    fx.gnames[0], fx.gnames[1] = fx.gnames[1], fx.gnames[0]          # the samples are packed in the order of the names
    with pytest.raises(AssertionError):
        ts.check_ggrads(fx, own, ts.SENS_BOUNDS)


def test_sample_idx():
    assert ts.G_SAMPLE == 32
    for n in (1, 32, 33, 1000, 4096):
        want = torch.arange(n) if n <= 32 else (torch.arange(32) * n) // 32
        got = ts.sample_idx(n)
        assert got.dtype == torch.int64 and torch.equal(got, want), n


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_ggrad_length_is_the_sum_of_the_samples(golden_dir, name):
    fx = ts.load(golden_dir, name)
    numel = _gen_numel(name)
    assert len(fx.gnames) == len(fx.npz["it0/gstat"])
    assert fx.npz["it0/ggrad"].shape[0] == sum(len(ts.sample_idx(numel[k])) for k in fx.gnames)
