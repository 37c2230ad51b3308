"""``dis.gan_type: nsgan / wgan`` on the one-launch adversarial loss tails (csrc/pointwise.hip adv_tail_*_kernel<GAN>,
dwc_adv_tail_gan_fwd / _bwd, hipdwc.ops.adv_tail(..., gan_type=)).

The reference expression is the reference's own, on the CPU in fp32 (networks.py:130-138, :157-163): per segment
``F.binary_cross_entropy(torch.sigmoid(src), all0 | all1)`` for nsgan, ``-+ src.mean()`` for wgan, ``((src - target) ** 2).mean()`` for
lsgan, plus ``orc.bce_with_logits_mean`` for the attribute term; autograd gives the gradients.  Bounds are those of
tests/test_hip_parity.py::test_adv_tail_and_weighted_sum_vs_oracle: value 2e-6 * max(1, |want|), gradients 1e-5 of the largest
magnitude.  nsgan's value bound gets one more term, computed from the inputs in float64: sum_s w_src[s] * mean_i(2^-23 / q_i) with q_i the
argument of the logarithm (p or 1 - p) -- what two units in the last place of p do to the reference's own value (d log q = dq / q,
ulp(p) <= 2^-24 for p < 1).  src is clamped to |x| <= 6, where the reference's fp32 value is within 2.5e-7 relative of the exact softplus
mean.

nsgan follows the reference as written, NOT the stable softplus: once sigmoid(x) has rounded to 0 or 1 the element costs exactly 100 or 0
and has no gradient (test_nsgan_saturation_elementwise).

The tests without the ``gpu`` mark (end of the file) need the built library only."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as ga

from hipdwc import _lib, ops, penalty, spectral, synth          # noqa: E402
from oracle import dwcgan_oracle as orc                          # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
GAN_TYPES = ["nsgan", "wgan", "lsgan"]
# (B, hw, segs): (2, 2, 4) the spectral-norm layout; (5, 8, 3) 320 elements per segment, a strided loop with a tail; (48, 16, 3) more
# than 64 x 256 elements, the backward's grid-stride loop
SHAPES = [(3, 1, 1), (4, 4, 3), (16, 2, 2), (2, 2, 4), (5, 8, 3), (48, 16, 3)]
# targets, w_src, w_cls per number of segments: G step / mixed / the D step without a norm (zero class weights on the fakes, and one
# zero src weight) / the D step with spectral norm
SPECS = {1: ((1.0,), (1.0,), (1.0,)),
         2: ((1.0, 0.0), (1.0, 0.7), (0.3, 0.0)),
         3: ((0.0, 0.0, 1.0), (1.0, 0.0, 2.0), (0.0, 0.3, 2.0)),
         4: ((0.0, 1.0, 0.0, 1.0), (0.5,) * 4, (0.0, 1.0, 0.0, 1.0))}
MAX_SRC = 6.0


def ids_x(s):
    return "x".join(str(v) for v in s)


def close(a, b, rel, msg=""):
    """max|a - b| <= rel * max|b| (tests/test_hip_parity.py::close without its absolute term)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err, lim = (a - b).abs().max().item(), rel * b.abs().max().item()
    print("%-28s max err %.3e (limit %.3e)" % (msg, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


def dev(t, grad=False):
    return t.detach().clone().to(DEV).requires_grad_(grad)


def ref_src_term(seg, target, gan_type):
    """The reference's src term of one segment (networks.py:130-138, :157-163)."""
    if gan_type == "lsgan":
        return ((seg - target) ** 2).mean()
    if gan_type == "wgan":
        return -seg.mean() if target else seg.mean()
    return F.binary_cross_entropy(torch.sigmoid(seg), torch.ones_like(seg) if target else torch.zeros_like(seg))


def ref_tail(src, cls, labels, B, targets, w_src, w_cls, gan_type):
    want = 0
    for s in range(len(targets)):
        want = want + w_src[s] * ref_src_term(src[s * B:(s + 1) * B], targets[s], gan_type) \
            + w_cls[s] * orc.bce_with_logits_mean(cls[s * B:(s + 1) * B], labels)
    return want


def nsgan_ulp_term(src, B, targets, w_src):
    """sum_s w_src[s] * mean_i(2^-23 / q_i) in float64, q_i = p_i (target 1) or 1 - p_i (target 0)."""
    extra = 0.0
    for s in range(len(targets)):
        p = torch.sigmoid(src[s * B:(s + 1) * B].double())
        extra += abs(w_src[s]) * float((2.0 ** -23 / (p if targets[s] else 1 - p)).mean())
    return extra


def make_case(B, hw, segs):
    g = torch.Generator().manual_seed(B * 10 + hw + segs)
    src = (torch.randn(segs * B, 1, hw, hw, generator=g) * 2.5).clamp(-MAX_SRC, MAX_SRC)
    cls = torch.randn(segs * B, 8, generator=g) * 2
    labels = (torch.rand(B, 8, generator=g) > 0.5).float()
    return (src, cls, labels) + SPECS[segs]


_REF = {}


def reference(B, hw, segs, gan_type):
    """Inputs, the CPU value and d(1.7 * value) / d src, d cls of one case; computed once and shared (read-only)."""
    key = (B, hw, segs, gan_type)
    if key not in _REF:
        src, cls, labels, targets, w_src, w_cls = make_case(B, hw, segs)
        sr, cr = src.clone().requires_grad_(True), cls.clone().requires_grad_(True)
        want = ref_tail(sr, cr, labels, B, targets, w_src, w_cls, gan_type)
        (want * 1.7).backward()
        _REF[key] = (src, cls, labels, targets, w_src, w_cls, float(want), sr.grad, cr.grad)
    return _REF[key]


# ---- a. values and gradients against the reference expression --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gan_type", GAN_TYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids_x)
def test_gan_tail_vs_reference_expression(shape, gan_type):
    B, hw, segs = shape
    src, cls, labels, targets, w_src, w_cls, want, dsrc, dcls = reference(B, hw, segs, gan_type)
    assert float(src.abs().max()) <= MAX_SRC
    sd, cd = dev(src, True), dev(cls, True)
    got = ops.adv_tail(sd, cd, labels.to(DEV), B, targets, w_src, w_cls, gan_type=gan_type)
    lim = 2e-6 * max(1.0, abs(want))
    if gan_type == "nsgan":
        lim += nsgan_ulp_term(src, B, targets, w_src)
    print("%s %s: %.8g against %.8g, err %.3e (limit %.3e)" % (gan_type, shape, float(got), want, abs(float(got) - want), lim))
    assert abs(float(got) - want) <= lim
    (got * 1.7).backward()
    close(sd.grad, dsrc, rel=1e-5, msg="dsrc")
    close(cd.grad, dcls, rel=1e-5, msg="dcls")


# ---- b. nsgan where the sigmoid saturates ------------------------------------------------------------------------------------------------
SAT_X = [30.0, -30.0, 90.0, -90.0, 0.0]


@gpu
@pytest.mark.parametrize("target", [0.0, 1.0])
def test_nsgan_saturation_elementwise(target):
    """x in {+-30, +-90, 0} against both targets: the loss of a one-element segment and every gradient equal the CPU expression within
    1e-5 relative, and the exact cases are exact -- 100 where the logarithm's argument has rounded to 0 (the clamp at -100), 0 where
    it has rounded to 1, gradient 0 in both (the backward multiplies by p (1 - p) = 0).  x = -30 against target 1 is NOT saturated in
    that sense: p = 9.4e-14 is a normal fp32 number, the loss is 30 and the gradient -1e12 p = -0.0936 (the 1e-12 clamp of the
    denominator), as in the reference.
    Every input stays out of 8 < |x| < 25: there 1 - p has only a few significant bits, the reference itself is off by 1e-2 (11.991 for
    an exact 12.000), and one bit of expf decides the result -- no tolerance short of that error would hold on two exp implementations."""
    assert all(not 8 < abs(x) < 25 for x in SAT_X)
    cls, labels = torch.zeros(1, 8), torch.zeros(1, 8)
    exact = 0
    for x in SAT_X:                                     # one-element segments: the loss of the element itself
        xr = torch.tensor([[[[x]]]], requires_grad=True)
        want = ref_src_term(xr, target, "nsgan")
        want.backward()
        xd = dev(xr, True)
        got = ops.adv_tail(xd, cls.to(DEV), labels.to(DEV), 1, (target,), (1.0,), (0.0,), gan_type="nsgan")
        got.backward()
        w, gw, gg = float(want), float(xr.grad), float(xd.grad)
        print("x %+5.0f target %d: loss %.7g against %.7g, gradient %.7g against %.7g" % (x, target, float(got), w, gg, gw))
        assert abs(float(got) - w) <= 1e-5 * abs(w) and abs(gg - gw) <= 1e-5 * abs(gw)
        if w in (0.0, 100.0):
            assert float(got) == w and gg == 0.0 and gw == 0.0
            exact += 1
    assert exact == 3                                   # +-90 and the x = +-30 whose sigmoid rounds to the OTHER label
    # the five as one segment of five samples: every gradient element, and the mean
    xr = torch.tensor(SAT_X).reshape(5, 1, 1, 1).requires_grad_(True)
    want = ref_src_term(xr, target, "nsgan")
    (want * 5).backward()
    xd = dev(xr, True)
    got = ops.adv_tail(xd, cls.repeat(5, 1).to(DEV), labels.repeat(5, 1).to(DEV), 5, (target,), (1.0,), (0.0,), gan_type="nsgan")
    (got * 5).backward()
    assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want))
    for x, a, b in zip(SAT_X, xd.grad.flatten().tolist(), xr.grad.flatten().tolist()):
        assert abs(a - b) <= 1e-5 * abs(b), (x, a, b)


def test_reference_expression_at_saturation():
    """What the kernel is held to above, on the CPU alone: loss 100 and gradient 0 at x = 30 against target 0; loss 30 and gradient
    -0.0936 at x = -30 against target 1."""
    x = torch.tensor([30.0], requires_grad=True)
    loss = ref_src_term(x, 0.0, "nsgan")
    loss.backward()
    assert float(loss) == 100.0 and float(x.grad) == 0.0
    x = torch.tensor([-30.0], requires_grad=True)
    loss = ref_src_term(x, 1.0, "nsgan")
    loss.backward()
    assert abs(float(loss) - 30.0) <= 1e-5 and abs(float(x.grad) + 0.0936) <= 1e-4


# ---- c. lsgan through the new entry points ----------------------------------------------------------------------------------------------
def _gan_entry_points(src, cls, labels, B, targets, w_src, w_cls, code, dout):
    """dwc_adv_tail_gan_fwd / _bwd called directly (ops.adv_tail sends lsgan to the entry points it always used)."""
    lib = _lib.load()
    segs, sps, ncls = src.shape[0] // B, src[0].numel(), cls[0].numel()
    spec = _lib.AdvSpec()
    for s in range(segs):
        spec.target[s], spec.w_src[s], spec.w_cls[s] = targets[s], w_src[s], w_cls[s]
    out, dsrc, dcls = torch.empty((), device=DEV), torch.empty_like(src), torch.empty_like(cls)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.dwc_adv_tail_gan_fwd(src.data_ptr(), cls.data_ptr(), labels.data_ptr(), out.data_ptr(), segs, B, sps, ncls, spec, code,
                                        stream), "adv_tail_gan_fwd")
    _lib.check(lib.dwc_adv_tail_gan_bwd(src.data_ptr(), cls.data_ptr(), labels.data_ptr(), dout.data_ptr(), dsrc.data_ptr(),
                                        dcls.data_ptr(), segs, B, sps, ncls, spec, code, stream), "adv_tail_gan_bwd")
    return out, dsrc, dcls


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids_x)
def test_lsgan_through_gan_entry_points_is_bit_equal(shape):
    B, hw, segs = shape
    src, cls, labels, targets, w_src, w_cls = make_case(B, hw, segs)
    sd, cd, ld = dev(src, True), dev(cls, True), labels.to(DEV)
    want = ops.adv_tail(sd, cd, ld, B, targets, w_src, w_cls)
    want.backward(torch.tensor(1.7, device=DEV))
    got, dsrc, dcls = _gan_entry_points(sd.detach(), cd.detach(), ld, B, targets, w_src, w_cls, ops.GAN_TYPES["lsgan"],
                                        torch.tensor(1.7, device=DEV))
    assert torch.equal(got, want.detach()) and torch.equal(dsrc, sd.grad) and torch.equal(dcls, cd.grad)
    named = ops.adv_tail(sd.detach(), cd.detach(), ld, B, targets, w_src, w_cls, gan_type="lsgan")
    assert torch.equal(named, want.detach())


# ---- d. run-to-run reproducibility --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gan_type", GAN_TYPES)
def test_two_launches_are_bit_equal(gan_type):
    B, hw, segs = 48, 16, 3
    src, cls, labels, targets, w_src, w_cls = make_case(B, hw, segs)
    runs = []
    for _ in range(2):
        sd, cd = dev(src, True), dev(cls, True)
        got = ops.adv_tail(sd, cd, labels.to(DEV), B, targets, w_src, w_cls, gan_type=gan_type)
        (got * 1.7).backward()
        runs.append((got.detach(), sd.grad, cd.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- e. output bounds -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def guards(monkeypatch):
    """tests/test_memory_contracts.py::guards: every output between guard zones."""
    alloc = ga.GuardedAllocator()
    proxy = ga.TorchProxy(alloc)
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    for mod in (ops, spectral, penalty):
        monkeypatch.setattr(mod, "torch", proxy)
    yield alloc
    alloc.forget()


@gpu
@pytest.mark.parametrize("gan_type", ["nsgan", "wgan"])
@pytest.mark.parametrize("shape", [(3, 1, 1), (4, 4, 3)], ids=ids_x)
def test_gan_tail_memory_contract(guards, shape, gan_type):
    B, hw, segs = shape
    src, cls, labels, targets, w_src, w_cls, want, dsrc, dcls = reference(B, hw, segs, gan_type)
    gi = lambda t, **k: ga.guarded_input(t, device=DEV, **k)                                     # noqa: E731
    sd, cd = gi(src, channels_last=False).requires_grad_(True), gi(cls).requires_grad_(True)
    got = ops.adv_tail(sd, cd, gi(labels), B, targets, w_src, w_cls, gan_type=gan_type)
    guards.verify()
    assert guards.handed.get("torch.empty", 0) == 1, guards.handed            # the value itself sat between guards
    assert not torch.isnan(got), "adv_tail is NaN"
    lim = 2e-6 * max(1.0, abs(want)) + (nsgan_ulp_term(src, B, targets, w_src) if gan_type == "nsgan" else 0.0)
    assert abs(float(got.detach()) - want) <= lim
    got.backward(gi(torch.tensor(1.7)))
    guards.verify()
    assert guards.handed.get("torch.empty_like", 0) == 2, guards.handed       # ... and so did both gradients
    assert not torch.isnan(sd.grad).any() and not torch.isnan(cd.grad).any()
    close(sd.grad, dsrc, rel=1e-5, msg="dsrc")
    close(cd.grad, dcls, rel=1e-5, msg="dcls")


# ---- f. without a GPU: declarations, argument checks, routing ---------------------------------------------------------------------------
NEW_SYMBOLS = ("dwc_adv_tail_gan_fwd", "dwc_adv_tail_gan_bwd")


def test_gan_tail_symbols_declared_bound_and_exported():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    for name, code in (("LSGAN", 0), ("NSGAN", 1), ("WGAN", 2)):
        assert re.search(r"#define DWC_GAN_%s %d\b" % (name, code), header)
        assert ops.GAN_TYPES[name.lower()] == code
    assert re.search(r"#define DWC_ABI_VERSION 11\b", header) and _lib.load().dwc_version() == 11      # additive: no new ABI number


@pytest.mark.parametrize("code", [3, -1])
def test_gan_entry_points_refuse_unknown_gan_type(code):
    """DWC_EINVAL in front of everything else -- null pointers, nothing launched, no device needed."""
    lib = _lib.load()
    assert lib.dwc_adv_tail_gan_fwd(None, None, None, None, 1, 1, 1, 1, _lib.AdvSpec(), code, None) == -1
    assert lib.dwc_adv_tail_gan_bwd(None, None, None, None, None, None, 1, 1, 1, 1, _lib.AdvSpec(), code, None) == -1


@pytest.mark.parametrize("code", [0, 1, 2])
def test_gan_entry_points_refuse_null_pointers(code):
    lib = _lib.load()
    assert lib.dwc_adv_tail_gan_fwd(None, None, None, None, 1, 1, 1, 1, _lib.AdvSpec(), code, None) == -1
    assert lib.dwc_adv_tail_gan_bwd(None, None, None, None, None, None, 1, 1, 1, 1, _lib.AdvSpec(), code, None) == -1


def test_adv_tail_refuses_unknown_gan_type():
    src, cls, labels = torch.zeros(2, 1, 1, 1), torch.zeros(2, 8), torch.zeros(2, 8)
    with pytest.raises(ValueError):
        ops.adv_tail(src, cls, labels, 2, (1.0,), (1.0,), (1.0,), gan_type="hinge")


def _tiny_dis(gan_type, dataset):
    from networks.networks import MsImageDis
    params = dict(synth.make_config(image_size=32, tiny=True)["dis"], gan_type=gan_type, dataset=dataset)
    return MsImageDis(3, params)


def test_adv_loss_raises_for_what_the_tail_does_not_take(monkeypatch):
    outs, labels = [[torch.zeros(2, 1, 1, 1), torch.zeros(2, 8)]], torch.zeros(2, 8)
    args = (outs, 2, labels, (1.0,), (1.0,), (1.0,))
    assert ops.ADV_TAIL_GAN == int(os.environ.get("DWC_ADV_TAIL_GAN", "1"))
    monkeypatch.setattr(ops, "ADV_TAIL_GAN", 1)
    for gan_type in GAN_TYPES:
        assert _tiny_dis(gan_type, "CelebA").adv_tail_ok() and _tiny_dis(gan_type, "CUB200").adv_tail_ok()
        with pytest.raises(NotImplementedError):
            _tiny_dis(gan_type, "AwA2").adv_loss(*args)           # a softmax-class dataset
    assert not _tiny_dis("hinge", "CelebA").adv_tail_ok()
    monkeypatch.setattr(ops, "ADV_TAIL_GAN", 0)
    assert _tiny_dis("lsgan", "CelebA").adv_tail_ok()
    for gan_type in ("nsgan", "wgan"):
        with pytest.raises(NotImplementedError):
            _tiny_dis(gan_type, "CelebA").adv_loss(*args)
