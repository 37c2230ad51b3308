"""Every absmax-slot producer held to the tensor its tag describes (fp32, DWC_X3_PLANES=2).

The two-plane f16 kernels scale each activation operand by a power of two read from an "absmax slot", 64 bits of
(epoch << 32) | bits(max|t|).  Most slots are raised by the kernel that WRITES the tensor (dwc_*_amax entry points) and attached with
``ops.set_amax``; ``ops.pass_amax`` lets resampling inherit its source's slot.  ``h2_scale`` maps the reported maximum into
[2^13, 2^14) and f16 ends just under 2^16, so a producer that under-reports by up to ~4x changes nothing a parity test on Gaussian
data can see -- until the first outlier lands in the region it skipped.

Here ``ops.set_amax`` / ``ops.pass_amax`` are wrapped by a recorder (tensor, slot, epoch, call site -- tensors that never leave a
backward included: g_out, dx, dz).  After each op: ONE synchronize, one copy of the slot pool, one stacked reduction of the recorded
tensors, then per record
  * epoch:     word >> 32 == the tag's epoch;
  * written:   word & 0xffffffff == the int32 bits of max|t| of the tensor the kernel wrote (all padded channels).  EQUALITY is the
               derived bound: every producer folds the very fp32 values it stores;
  * inherited: the slot holds max|source| bitwise and max|t| <= max|source|;
  * non-finite tensors: slot bits >= 0x7f800000.
The comparison is always against the produced tensor, never a reference op (what y should BE is the parity tests' business).

Inputs are noise plus ONE element 64x larger, planted so that the output's peak falls in turn on each region a kernel could skip
(REGIONS below); each sweep asserts that argmax|t| of the produced tensor really lay in every targeted region, and -- for the small
shapes -- that the float64 torch form of the op puts it there too.  No producer was found that publishes a bound instead of the
maximum: every site is held to equality.  The last test asserts that every ``set_amax(`` / ``pass_amax(`` call site of hipdwc was
reached."""
import collections
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_spectral_norm import SN_CASES, _block as _sn_block

pytestmark = pytest.mark.gpu

from hipdwc import _lib, host, ops, spectral, synth          # noqa: E402
from oracle import dwcgan_oracle as orc                       # noqa: E402

DEV = "cuda:0"
PEAK = 64.0
_PKG = os.path.dirname(os.path.abspath(ops.__file__))


# ---- call sites, bookkeeping of the cases ------------------------------------------------------------------------------------------
def _scan_sites():
    sites = {}
    for name in ("ops.py", "spectral.py", "penalty.py"):
        with open(os.path.join(_PKG, name)) as f:
            for no, line in enumerate(f, 1):
                if re.search(r"\b(set_amax|pass_amax)\(", line) and not line.lstrip().startswith("def "):
                    sites[(name, no)] = line.strip()
    return sites


SITES = _scan_sites()
# (file, text that identifies ONE call site): reason.  The site inside amax_of + at most one more.
EXEMPT = {
    ("ops.py", "set_amax(t, slot, ep)"): "inside amax_of: tags what dwc_absmax measured, not a producer (tests/test_h2_parity.py measures "
                                         "with dwc_absmax throughout); reached or not, it is not judged here",
}
SEEN = set()
EXPECTED, RAN = set(), set()
SUMMARY = collections.OrderedDict()      # producer -> set of regions whose planted peak matched bitwise


def cases(argname, values, ids):
    """pytest.mark.parametrize that also registers the case names: the coverage test at the end only judges a run of all of them."""
    values = list(values)
    names = [ids(v) for v in values]
    assert len(set(names)) == len(names), names

    def deco(fn):
        EXPECTED.update("%s[%s]" % (fn.__name__, n) for n in names)
        return pytest.mark.parametrize(argname, values, ids=names)(fn)
    return deco


def single(fn):
    EXPECTED.add(fn.__name__)
    return fn


def ids_x(s):
    return "x".join(str(v) for v in s)


# ---- recorder ----------------------------------------------------------------------------------------------------------------------
class Rec:
    __slots__ = ("kind", "t", "slot", "ep", "site", "src", "tag")

    def __init__(self, kind, t, slot, ep, site, src=None):
        self.kind, self.t, self.slot, self.ep, self.site, self.src, self.tag = kind, t, slot, ep, site, src, None

    @property
    def text(self):
        return SITES.get(self.site, "<test>")


class Recorder:
    def __init__(self):
        self.recs, self.details, self.verified, self._pending, self.keep = [], [], [], 0, True

    def take(self):
        out, self.recs = self.recs, []
        return out

    def add(self, t, slot, ep):
        """A record for an entry point the test called itself (no ops call site)."""
        self.recs.append(Rec("set", t, slot, ep, ("<test>", 0)))


def _site(frame):
    return os.path.basename(frame.f_code.co_filename), frame.f_lineno


@pytest.fixture
def rec(monkeypatch, request):
    """ops.set_amax / ops.pass_amax (looked up through the module at call time by ops.py and spectral.py) wrapped: the originals run,
    the recorder keeps (tensor, slot, epoch, file and line of the caller).  ops._timed and ops._amax_verify are wrapped too: the
    detail string names the launch form a case took, and a verification is booked on the launch that follows it."""
    ops.set_precision("fp32")
    assert ops.X3_PLANES == 2 and ops.X3 == 2, "the two-plane f16 path is the default fp32 path"
    r = Recorder()
    real_set, real_pass, real_verify, real_timed = ops.set_amax, ops.pass_amax, ops._amax_verify, ops._timed

    def set_amax(t, slot, ep):
        f = sys._getframe(1)
        site = _site(f)
        SEEN.add(site)
        if f.f_code.co_name != "pass_amax" and r.keep:          # (pass_amax's own record follows)
            r.recs.append(Rec("set", t, slot, ep, site))
        return real_set(t, slot, ep)

    def pass_amax(src, dst):
        site = _site(sys._getframe(1))
        SEEN.add(site)
        out = real_pass(src, dst)
        c = ops.amax_live(dst)
        if c is not None and r.keep:
            r.recs.append(Rec("pass", dst, c[0], c[1], site, src))
        return out

    def verify(t, c):
        r._pending += 1
        return real_verify(t, c)

    def timed(tag, flops, fn, scope_name=None, detail="", exec_flops=None):
        r.details.append(detail)
        if r._pending:
            r.verified.append((detail, r._pending))
            r._pending = 0
        return real_timed(tag, flops, fn, scope_name, detail, exec_flops)

    monkeypatch.setattr(ops, "set_amax", set_amax)
    monkeypatch.setattr(ops, "pass_amax", pass_amax)
    monkeypatch.setattr(ops, "_amax_verify", verify)
    monkeypatch.setattr(ops, "_timed", timed)
    yield r
    RAN.add(request.node.name)


def check(recs):
    """The contract of the module docstring for every record; returns argmax|t| of each record's tensor as an (n, c, h, w) index (or
    a flat one for tensors of another rank).  One synchronize, one copy of the pool, one stacked reduction."""
    assert recs, "nothing was recorded"
    tens = [r.t.detach() for r in recs] + [r.src.detach() for r in recs if r.src is not None]
    mags = torch.stack([t.abs().max() for t in tens])
    args = torch.stack([t.abs().reshape(-1).argmax() for t in tens])
    torch.cuda.synchronize()
    pool = ops._AMAX[torch.cuda.current_device()][0]
    words = pool.cpu().numpy()                                                # as ops._amax_verify indexes it
    mags = mags.view(torch.int32).cpu().numpy()
    args = args.cpu().numpy()
    out, k_src = [], len(recs)
    for i, r in enumerate(recs):
        word = int(words[(r.slot - pool.data_ptr()) // 8])
        bits, true_bits = word & 0xffffffff, int(mags[i])
        where = "%s:%d  %s%s" % (r.site[0], r.site[1], r.text, ("  [%s]" % (r.tag,)) if r.tag else "")
        assert (word >> 32) == r.ep, "%s: slot epoch %d, tag says %d" % (where, word >> 32, r.ep)
        idx = tuple(int(v) for v in np.unravel_index(int(args[i]), tuple(r.t.shape)))
        if r.kind == "pass":
            src_bits = int(mags[k_src])
            k_src += 1
            assert bits == src_bits, "%s: inherited slot holds %#x, max|source| is %#x" % (where, bits, src_bits)
            assert true_bits <= src_bits, "%s: max|t| %#x above its source's %#x" % (where, true_bits, src_bits)
        elif true_bits >= 0x7f800000:
            assert bits >= 0x7f800000, "%s: non-finite tensor, slot holds the finite %#x" % (where, bits)
        else:
            assert bits == true_bits, "%s: slot holds %#x (%g), max|t| is %#x (%g) at %s of %s" % (
                where, bits, np.int32(bits).view(np.float32), true_bits, np.int32(true_bits).view(np.float32), idx, tuple(r.t.shape))
        out.append(idx)
    return out


def _of(recs, what):
    """The one record whose call-site text names ``what`` (e.g. 'set_amax(dx'), or whose tensor IS ``what``."""
    if isinstance(what, str):
        hit = [r for r in recs if what in r.text]
    else:           # (a channel slice of a channels-last buffer starts at the buffer's address)
        hit = [r for r in recs if r.t.data_ptr() == what.data_ptr() and r.t.shape[2:] == what.shape[2:]]
    assert len(hit) == 1, (what if isinstance(what, str) else "tensor", [r.text for r in recs])
    return hit[0]


# ---- regions -----------------------------------------------------------------------------------------------------------------------
# Region predicates over idx = (n, c, h, w) of argmax|t| in a produced [B, C, H, W] tensor.  g (``geo``): B, C, H, W, rpc (rows per
# row chunk of the kernel's launch plan), lcr (first row of the last chunk) and ``glob`` (True: rows count over the B*H*W rows of the
# whole tensor -- act backward, SN epilogue -- False: over the H*W rows of each sample).
def geo(B, C, H, W, rpc=0, chunks=1, glob=False, lcr=None):
    return dict(B=B, C=C, H=H, W=W, rpc=rpc, glob=glob, lcr=(chunks - 1) * rpc if lcr is None else lcr)


def _row(idx, g):
    n, c, h, w = idx
    p = h * g["W"] + w
    return n * g["H"] * g["W"] + p if g["glob"] else p


REGIONS = {
    "first pixel": lambda i, g: i[0] == 0 and i[2] == 0 and i[3] == 0,
    "last pixel": lambda i, g: i[0] == g["B"] - 1 and i[2] == g["H"] - 1 and i[3] == g["W"] - 1,
    "last row of first chunk": lambda i, g: (g["glob"] or i[0] == 0) and _row(i, g) == g["rpc"] - 1,
    "first row of last chunk": lambda i, g: (g["glob"] or i[0] == g["B"] - 1) and _row(i, g) == g["lcr"],
    "channel 0": lambda i, g: i[1] == 0,
    "last channel quad": lambda i, g: i[1] >= g["C"] - 4,
    "last sample": lambda i, g: i[0] == g["B"] - 1,
    # convolutions (16 x 16-pixel tiles)
    "corner": lambda i, g: i[2] in (0, g["H"] - 1) and i[3] in (0, g["W"] - 1),
    "edge": lambda i, g: (i[2] in (0, g["H"] - 1)) != (i[3] in (0, g["W"] - 1)),
    "tile boundary 15": lambda i, g: 15 in (i[2], i[3]),
    "tile boundary 16": lambda i, g: 16 in (i[2], i[3]),
    "interior": lambda i, g: 0 < i[2] < g["H"] - 1 and 0 < i[3] < g["W"] - 1 and i[2] % 16 not in (0, 15) and i[3] % 16 not in (0, 15),
}


def row_targets(g):
    """(region, (n, c, h, w)) for the row-chunked kernels (norms, act backward, SN epilogue)."""
    B, C, H, W, rpc = g["B"], g["C"], g["H"], g["W"], g["rpc"]
    cm = min(C - 1, 5) if C > 8 else 1                    # a channel that is neither 0 nor in the last quad (C = 8: quad 0)

    def at(row, n=0):
        if g["glob"]:
            n, row = divmod(row, H * W)
        return n, row // W, row % W
    pm = (H // 2) * W + W // 2 - 1
    t = [("first pixel", (0, cm, 0, 0)), ("last pixel", (B - 1, cm, H - 1, W - 1))]
    n, h, w = at(rpc - 1)
    t.append(("last row of first chunk", (n, cm, h, w)))
    n, h, w = at(g["lcr"], B - 1)
    t.append(("first row of last chunk", (n, cm, h, w)))
    t += [("channel 0", (0, 0) + divmod(pm, W)), ("last channel quad", (0, C - 1) + divmod(pm, W)),
          ("last sample", (B - 1, cm) + divmod(pm, W))]
    return t


def conv_targets(B, C, H, W, c_real=None):
    """(region, (n, co, h, w)) for a convolution output [B, C, H, W] (C padded, c_real real channels)."""
    cr = C if c_real is None else c_real
    cm = min(cr - 1, 21)
    t = [("first pixel", (0, cm, 0, 0)), ("last pixel", (B - 1, cm, H - 1, W - 1)), ("corner", (0, cm, H - 1, 0)),
         ("edge", (0, cm, 0, W // 2 + 1)), ("interior", (0, cm, H // 2 + 1, W // 2 + 2)), ("channel 0", (0, 0, H // 2, 3)),
         ("last channel quad", (0, cr - 1, 2, W // 2)), ("last sample", (B - 1, cm, H // 2 + 1, 5))]
    if W > 16:
        t += [("tile boundary 15", (0, cm, 3, 15)), ("tile boundary 16", (B - 1, cm, 5, 16))]
    elif H > 16:
        t += [("tile boundary 15", (0, cm, 15, 3)), ("tile boundary 16", (B - 1, cm, 16, 5))]
    else:
        t += [("tile boundary 15", (0, cm, 15, 7))]
    return t


def in_regions(producer, geom, hits):
    """``hits``: (region aimed at, argmax found).  Every targeted region must hold the peak of its run; booked for the summary."""
    assert hits
    for region, idx in hits:
        assert REGIONS[region](idx, geom), "%s: the peak aimed at '%s' was found at %s of %s" % (
            producer, region, idx, (geom["B"], geom["C"], geom["H"], geom["W"]))
    SUMMARY.setdefault(producer, set()).update(r for r, _ in hits)


def _argmax(t):
    t = t.detach().abs()
    return tuple(int(v) for v in np.unravel_index(int(t.reshape(-1).argmax()), tuple(t.shape)))


def noise(shape, seed, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * amp


def dcl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


# ---- norms -------------------------------------------------------------------------------------------------------------------------
def plan_apply(B, HW, C, V=4):
    """csrc/norm.hip plan_apply: (chunks, rows per chunk, column groups cq, row groups) of the multi-pass apply kernels."""
    cq = max(C // V, 1)
    groups = max(256 // cq, 1)
    rpc = groups * 32
    while rpc > groups * 4 and B * ((HW + rpc - 1) // rpc) < 1024:
        rpc //= 2
    while B * ((HW + rpc - 1) // rpc) > 16384 and rpc < HW:
        rpc *= 2
    rpc = min(rpc, HW)
    return (HW + rpc - 1) // rpc, rpc, cq, groups


def in_resident_hw(HW, C):
    """csrc/norm.hip in_resident_hw<float>: the plane size when the resident-plane kernels take the shape, else 0."""
    return HW if (C % 32 == 0 and HW in (256, 1024)) else 0


def norm_geom(B, C, H, resident):
    if resident:      # no row chunks (a workgroup holds whole planes): the two 'chunk' regions are the middle rows of the plane
        return geo(B, C, H, H, H * H // 2, 2)
    chunks, rpc, _, _ = plan_apply(B, H * H, C)
    return geo(B, C, H, H, rpc, chunks)


def _in_ref(x, gamma, beta, res, relu):
    B, C = x.shape[:2]
    t = orc.instance_norm(x)
    if gamma is not None:
        t = t * gamma.view(B, C, 1, 1) + beta.view(B, C, 1, 1)
    if relu:
        t = torch.relu(t)
    return t if res is None else t + res


IN_RESIDENT = [(2, 32, 16), (2, 32, 32)]
IN_MULTI = [(2, 64, 12), (3, 8, 6), (2, 256, 8)]
IN_CASES = [s + (res, relu, aff) for s in IN_RESIDENT + IN_MULTI for res in (0, 1) for relu in (0, 1) for aff in (0, 1)]


@cases("case", IN_CASES, ids_x)
def test_instance_norm_slots(rec, case):
    """Instance norm forward (peak planted in x) and backward (planted in dy, at an element with y > 0), every launch plan: resident
    256 / 1024 planes x residual x ReLU x affine (separate template instances) and the multi-pass apply kernels at (2,64,12) -- 144 rows
    are no multiple of the row split --, (3,8,6) -- cq = 2, 128 row groups for 36 rows: most threads walk no row but must reach the
    publish barrier -- and (2,256,8) -- cq = 64, 4 row groups."""
    B, C, H, res, relu, aff = case
    HW = H * H
    resident = (B, C, H) in IN_RESIDENT
    assert bool(in_resident_hw(HW, C)) == resident, "the shape does not take the launch plan it is listed under"
    chunks, rpc, cq, groups = plan_apply(B, HW, C)
    if (B, C, H) == (2, 64, 12):
        assert HW % rpc != 0 and chunks > 1
    if (B, C, H) == (3, 8, 6):
        assert cq == 2 and groups == 128 and groups > HW
    if (B, C, H) == (2, 256, 8):
        assert cq == 64 and groups == 4
    geom = norm_geom(B, C, H, resident)
    seed = sum(case) * 7 + H
    gamma = (1.0 + noise((B * C,), seed + 1, 0.1)) if aff else None
    beta = noise((B * C,), seed + 2, 0.1) if aff else None
    resid = noise((B, C, H, H), seed + 3, 0.5) if res else None
    gd, bd = (gamma.to(DEV), beta.to(DEV)) if aff else (None, None)
    rd = dcl(resid) if res else None
    tagged, aims = [], []
    for k, (region, (n, c, h, w)) in enumerate(row_targets(geom)):
        x = noise((B, C, H, H), seed + 10 + k)
        x[n, c, h, w] = PEAK
        ref = _in_ref(x.double(), None if gamma is None else gamma.double(), None if beta is None else beta.double(),
                      None if resid is None else resid.double(), relu)
        assert _argmax(ref) == (n, c, h, w), "planting recipe (forward): float64 puts the peak at %s" % (_argmax(ref),)
        xd = dcl(x).requires_grad_(True)
        y = ops.instance_norm(xd, gd, bd, rd, relu=bool(relu))
        r = _of(rec.recs, y)
        r.tag = ("fwd", region)
        aims.append(("fwd", region))
        # backward: x is noise with +1 at the planted element (y > 0 there: the ReLU mask passes), dy = noise + the peak
        x2 = noise((B, C, H, H), seed + 40 + k)
        x2[n, c, h, w] = 1.0
        dy = noise((B, C, H, H), seed + 70 + k)
        dy[n, c, h, w] = PEAK
        xr = x2.double().requires_grad_(True)
        _in_ref(xr, None if gamma is None else gamma.double(), None if beta is None else beta.double(),
                None if resid is None else resid.double(), relu).backward(dy.double())
        assert _argmax(xr.grad) == (n, c, h, w), "planting recipe (backward): float64 puts the peak at %s" % (_argmax(xr.grad),)
        before = len(rec.recs)
        xd2 = dcl(x2).requires_grad_(True)
        ops.instance_norm(xd2, gd, bd, rd, relu=bool(relu)).backward(dcl(dy))
        r = _of(rec.recs[before:], "set_amax(dx")
        r.tag = ("bwd", region)
        aims.append(("bwd", region))
    recs = rec.take()
    found = check(recs)
    name = "instance norm %s" % ("resident %d" % HW if resident else "multi-pass")
    for way in ("fwd", "bwd"):
        in_regions("%s %s" % (name, way), geom, [(r.tag[1], i) for r, i in zip(recs, found) if r.tag and r.tag[0] == way])
    assert {r.tag for r in recs if r.tag} == set(aims)


LN_CASES = [s + (relu,) for s in [(3, 8, 6), (1, 64, 12), (2, 128, 16)] for relu in (0, 1)]


@cases("case", LN_CASES, ids_x)
def test_layer_norm_slots(rec, case):
    """Layer norm (per-sample statistics, per-channel affine) forward and backward on the multi-pass apply kernels, as the instance
    norm above."""
    B, C, H, relu = case
    chunks, rpc, cq, groups = plan_apply(B, H * H, C)
    geom = geo(B, C, H, H, rpc, chunks)
    seed = sum(case) * 11
    gamma, beta = 1.0 + noise((C,), seed + 1, 0.1), noise((C,), seed + 2, 0.1)
    gd, bd = gamma.to(DEV), beta.to(DEV)

    def ref(x):
        t = orc.layer_norm_munit(x, gamma.double(), beta.double())
        return torch.relu(t) if relu else t
    for k, (region, (n, c, h, w)) in enumerate(row_targets(geom)):
        x = noise((B, C, H, H), seed + 10 + k)
        x[n, c, h, w] = PEAK
        assert _argmax(ref(x.double())) == (n, c, h, w), "planting recipe (forward)"
        y = ops.layer_norm_munit(dcl(x).requires_grad_(True), gd, bd, relu=bool(relu))
        _of(rec.recs, y).tag = ("fwd", region)
        x2 = noise((B, C, H, H), seed + 40 + k)
        x2[n, c, h, w] = 1.0
        dy = noise((B, C, H, H), seed + 70 + k)
        dy[n, c, h, w] = PEAK
        xr = x2.double().requires_grad_(True)
        ref(xr).backward(dy.double())
        assert _argmax(xr.grad) == (n, c, h, w), "planting recipe (backward)"
        before = len(rec.recs)
        g2, b2 = gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
        ops.layer_norm_munit(dcl(x2).requires_grad_(True), g2, b2, relu=bool(relu)).backward(dcl(dy))
        _of(rec.recs[before:], "set_amax(dx").tag = ("bwd", region)
    recs = rec.take()
    found = check(recs)
    for way in ("fwd", "bwd"):
        hits = [(r.tag[1], i) for r, i in zip(recs, found) if r.tag and r.tag[0] == way]
        assert len(hits) == len(row_targets(geom))
        in_regions("layer norm %s" % way, geom, hits)


# ---- activation backward -----------------------------------------------------------------------------------------------------------
def act_plan(rows):
    """csrc/pointwise.hip act_plan: (chunks, rows per chunk) over the B*H*W rows."""
    c = min(max(rows // 32, 1), 1024)
    rpc = (rows + c - 1) // c
    return (rows + rpc - 1) // rpc, rpc


ACT_CASES = [(2, 9, 9, "relu"), (2, 9, 9, "lrelu"), (2, 12, 10, "tanh"), (2, 12, 10, "sigmoid"), (2, 12, 10, "relu")]


@cases("case", ACT_CASES, ids_x)
def test_act_backward_slot_through_conv2d(rec, case):
    """dwc_act_bwd_bias_amax in ops.conv2d's backward: g = dy * act'(y), 64 channels (16 column groups x 16 row groups), 162 / 240 rows
    in chunks of 33 / 35 rows -- odd against the 2 x 16 rows a pass of the two-row loop takes, so every chunk ends in the tail loop.
    The bias (+0.5) keeps y > 0 except in channel 1 (-0.5: y = 0 under ReLU, negative under LeakyReLU), where a DECOY of 2 x the peak
    sits in dy: a kernel that folded dy instead of g would publish the decoy."""
    B, H, W, act = case
    C, rows = 64, B * H * W
    chunks, rpc = act_plan(rows)
    assert rpc % 2 == 1 and chunks > 2, (chunks, rpc)
    geom = geo(B, C, H, W, rpc, chunks, glob=True)
    seed = B + H * 3 + W * 5 + len(act)
    w = noise((C, C, 3, 3), seed, 0.002)
    b = torch.full((C,), 0.5)
    b[1] = -0.5
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    x = noise((B, C, H, W), seed + 1)
    for k, (region, (n, c, h, w_)) in enumerate(row_targets(geom)):
        dy = noise((B, C, H, W), seed + 10 + k)
        dy[n, c, h, w_] = PEAK
        if act in ("relu", "lrelu"):
            dy[n, 1, h, w_] = 2 * PEAK
        yv = orc.conv_block(x.double(), w.double(), b.double(), 1, 1, act=act)            # float64 form of g: dy * act'(y)
        dact = {"relu": (yv > 0).double(), "lrelu": torch.where(yv > 0, 1.0, 0.1).double(), "tanh": 1 - yv * yv,
                "sigmoid": yv * (1 - yv)}[act]
        assert _argmax(dy.double() * dact) == (n, c, h, w_), "planting recipe: float64 puts the peak of g elsewhere"
        before = len(rec.recs)
        xd = dcl(x).requires_grad_(True)
        ops.conv2d(xd, wd, bd, 1, 1, act).backward(dcl(dy))
        _of(rec.recs[before:], "set_amax(g_out").tag = region
    recs = rec.take()
    found = check(recs)
    hits = [(r.tag, i) for r, i in zip(recs, found) if r.tag]
    assert len(hits) == len(row_targets(geom))
    in_regions("act backward (%s)" % act, geom, hits)


@single
def test_act_backward_slot_wide_channels(rec):
    """cq >= 256: no convolution shape of the networks reaches 1024 channels, so the entry point is called directly -- 2048 channels
    (cq = 512: two column blocks of 256 threads, one row group each), 70 rows in two chunks of 35."""
    lib = _lib.load()
    rows, C, act = 70, 2048, ops.ACT["lrelu"]
    chunks, rpc = act_plan(rows)
    assert C // 4 >= 256 and chunks == 2 and rpc == 35
    geom = geo(1, C, rows, 1, rpc, chunks, glob=True)
    ws = torch.empty(lib.dwc_act_bwd_bias_ws_bytes(rows, C), dtype=torch.uint8, device=DEV)
    y = noise((rows, C), 5).abs() + 0.1
    y[:, 1] = -1.0
    yd = y.to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    extra = [("last channel quad", (0, 1023, 3, 0)), ("channel 0", (0, 1024, 40, 0))]      # the seam of the two column blocks
    targets = row_targets(geom) + extra
    for k, (region, (n, c, h, w_)) in enumerate(targets):
        dy = noise((rows, C), 10 + k)
        dy[h, c] = PEAK
        dy[h, 1] = 2 * PEAK
        dyd = dy.to(DEV)
        g = torch.empty_like(dyd)
        db = torch.empty(C, device=DEV)
        slot, ep = ops.amax_slot(g.device)
        _lib.check(lib.dwc_act_bwd_bias_amax(dyd.data_ptr(), yd.data_ptr(), g.data_ptr(), db.data_ptr(), rows, C, act, ws.data_ptr(), ws.numel(),
                                             slot, ep, st), "act_bwd_bias_amax")
        rec.add(g.view(1, rows, 1, C).permute(0, 3, 1, 2), slot, ep)
        rec.recs[-1].tag = (region, (n, c, h, w_))
    recs = rec.take()
    found = check(recs)
    for r, idx in zip(recs, found):
        assert idx == r.tag[1], (r.tag, idx)
    in_regions("act backward (2048 channels, direct)", geom, [(r.tag[0], i) for r, i in zip(recs, found)][:len(row_targets(geom))])


# ---- convolutions ------------------------------------------------------------------------------------------------------------------
def _conv_sweep(rec, producer, run, B, Cin, Cout, H, W, K, stride, act, bias, seed):
    """Impulse sweeps of one convolution layer.  Filter = low noise + ONE centre-most tap of 1.0 from input channel 2 to output channel
    co, input = low noise + one impulse of 64 in channel 2: the output's peak sits at (n, co, the impulse's pixel / stride).
    ``run(x, w, b, act)`` -> the op's output (channel slice of the padded buffer).  The float64 form of the layer confirms the recipe
    in the test itself (the torch fp32 form from 3e8 multiply-adds on)."""
    dt = torch.float64 if B * Cout * (H // stride) * (W // stride) * Cin * K * K < 3e8 else torch.float32
    Ho, Wo = H // stride, W // stride
    cop = (Cout + 3) // 4 * 4
    geom = geo(B, cop, Ho, Wo)
    ci = 2
    kc = (K - 1) // 2                                        # 3x3 / 5x5: the centre; 4x4 stride 2 pad 1: tap (1, 1) reads pixel (2h, 2w)
    b = None
    if bias:
        b = noise((Cout,), seed + 1, 0.05).to(DEV)
    hits = []
    for k, (region, (n, co, h, w_)) in enumerate(conv_targets(B, cop, Ho, Wo, Cout)):
        wt = noise((Cout, Cin, K, K), seed + 100 + k, 0.02 / (Cin * K * K) ** 0.5)
        wt[co, ci, kc, kc] = 1.0
        x = noise((B, Cin, H, W), seed + 200 + k, 0.5)
        x[n, ci, h * stride, w_ * stride] = PEAK
        pad = 1 if stride == 2 else K // 2
        yr = orc.activation(F.conv2d(F.pad(x.to(dt), (pad,) * 4, mode="reflect" if run.reflect else "constant"), wt.to(dt),
                                     None if b is None else b.cpu().to(dt), stride=stride), act)
        assert _argmax(yr) == (n, co, h, w_), "planting recipe: the reference puts the peak at %s, aimed at %s" % (_argmax(yr), (n, co, h, w_))
        before = len(rec.recs)
        y = run(dcl(x), wt.to(DEV), b, act)
        assert y.shape == (B, Cout, Ho, Wo)
        r = _of(rec.recs[before:], y)
        assert r.t.shape[1] == cop, "the slot is held to the padded buffer"
        r.tag = region
    recs = rec.take()
    found = check(recs)
    hits = [(r.tag, i) for r, i in zip(recs, found) if r.tag]
    assert len(hits) == len(conv_targets(B, cop, Ho, Wo, Cout))
    in_regions(producer, geom, hits)


def _conv2d(x, w, b, act, stride=1):
    with torch.no_grad():
        return ops.conv2d(x, w, b, stride, 1 if stride == 2 else w.shape[2] // 2, act)


_conv2d.reflect = True

# (B, Cin, Cout, H, W, K, act, bias)
H2_S1 = [
    (2, 64, 64, 16, 16, 3, "none", 0),              # one workgroup per image
    (2, 64, 64, 16, 16, 3, "relu", 1),
    (1, 64, 62, 16, 48, 3, "lrelu", 1),             # Cout 62 in a padded buffer of 64; three tiles per image
    (1, 64, 64, 32, 32, 3, "tanh", 1),
    (2, 64, 62, 16, 32, 3, "sigmoid", 0),           # (the padded channels hold sigmoid(0) = 0.5)
    (2, 64, 64, 16, 32, 5, "relu", 1),              # 5x5
    (4, 128, 256, 32, 32, 3, "none", 1),            # contraction split (tests/test_h2_parity.py test_h2_contraction_split_of_small_launches)
    (2, 256, 128, 32, 32, 5, "lrelu", 1),           # contraction split, 5x5
]


@cases("case", H2_S1, ids_x)
def test_h2_stride1_forward_slot(rec, case):
    """The stride-1 'same' two-plane forward through ops.conv2d: y's slot is raised in the store loop behind bias, activation and (in
    a split launch) the partner's half sums -- a split tile's first arriver has left before the store and must not be missed."""
    B, Cin, Cout, H, W, K, act, bias = case
    lib = _lib.load()
    cop = (Cout + 3) // 4 * 4
    assert lib.dwc_x3_conv2d_same_ok(B, H, W, Cin, cop, K)
    split = lib.dwc_x3_conv2d_ksplit_ws_bytes(B, H, W, Cin, cop, K, 1) != 0
    assert split == (Cin >= 128), "the shape does not take the launch form (contraction split or not) it is listed for"
    _conv_sweep(rec, "h2 forward stride 1%s" % (" (contraction split)" if split else ""), _conv2d, B, Cin, Cout, H, W, K, 1, act, bias,
                sum(case[:6]))
    assert rec.details and all(d.startswith("fwd-h2 ") for d in rec.details), set(rec.details)


# the smallest shapes that pass the >= 160 workgroup gate of _Conv2d.forward: B * (H // 32) * (W // 32) * (Cout // 64)
H2_S2 = [(10, 16, 256, 64, 64, 4, "lrelu", 1), (40, 64, 256, 32, 32, 4, "none", 0)]      # (the second: one 16 x 16 tile per image, contraction split)


@cases("case", H2_S2, ids_x)
def test_h2_stride2_forward_slot(rec, case):
    """The stride-2 4x4 two-plane forward at exactly the 160 workgroups _Conv2d.forward asks for: 64 x 64 images (two tiles a side of
    the 32 x 32 output: the tile boundary regions), and 32 x 32 images with 64 input channels (one tile per image, contraction split)."""
    B, Cin, Cout, H, W, K, act, bias = case
    lib = _lib.load()
    assert B * (H // 32) * (W // 32) * (Cout // 64) == 160 and lib.dwc_x3_conv2d_s2_ok(B, H, W, Cin, Cout)
    split = lib.dwc_x3_conv2d_ksplit_ws_bytes(B, H, W, Cin, Cout, 4, 2) != 0
    assert split == (Cin == 64)
    run = lambda x, w, b, a: _conv2d(x, w, b, a, stride=2)
    run.reflect = True
    _conv_sweep(rec, "h2 forward stride 2%s" % (" (contraction split)" if split else ""), run, B, Cin, Cout, H, W, K, 2, act, bias,
                sum(case[:6]))
    assert rec.details and all(d.startswith("fwd-h2s2 ") for d in rec.details), set(rec.details)


@cases("case", [(2, 64, 64, 16, 32, 3, "relu", 1), (1, 64, 62, 32, 32, 3, "none", 0)], ids_x)
def test_zeropad_forward_slot(rec, case):
    """ops.conv2d_zeropad (the frozen VGG layers): the same kernel under the zero rule, its own call site."""
    B, Cin, Cout, H, W, K, act, bias = case

    def run(x, w, b, a):
        with torch.no_grad():
            return ops.conv2d_zeropad(x, w, b, 1, a)
    run.reflect = False
    _conv_sweep(rec, "zero-pad forward", run, B, Cin, Cout, H, W, K, 1, act, bias, sum(case[:6]))
    assert rec.details and all(d.startswith("fwd-h2 ") and d.endswith("zeropad") for d in rec.details), set(rec.details)


@cases("case", [(3, 20, 36, "relu"), (2, 16, 16, "none")], ids_x)
def test_stem_forward_slot(rec, case):
    """dwc_x3_conv2d_stem_amax: the fp32 7x7 stem on an NHWC4 image (3 real planes + a zero plane), 64 outputs; 20 x 36 pixels are
    no whole 16 x 16 blocks."""
    B, H, W, act = case
    assert _lib.load().dwc_x3_conv2d_stem_ok(B, H, W, H, W, 7, ops.ACT[act])
    geom = geo(B, 64, H, W)
    seed = B + H + W
    b = noise((64,), seed, 0.05).to(DEV)
    for k, (region, (n, co, h, w_)) in enumerate(conv_targets(B, 64, H, W)):
        wt = noise((64, 3, 7, 7), seed + 100 + k, 0.02 / 147 ** 0.5)
        wt[co, 2, 3, 3] = 1.0
        x = torch.zeros(B, 4, H, W)
        x[:, :3] = noise((B, 3, H, W), seed + 200 + k, 0.5)
        x[n, 2, h, w_] = PEAK
        yr = orc.activation(F.conv2d(F.pad(x[:, :3].double(), (3,) * 4, mode="reflect"), wt.double(), b.double().cpu()), act)
        assert _argmax(yr) == (n, co, h, w_), "planting recipe"
        before = len(rec.recs)
        with torch.no_grad():
            y = ops.conv2d(dcl(x), wt.to(DEV), b, 1, 3, act)
        _of(rec.recs[before:], y).tag = region
    assert rec.details and all(d.startswith("fwd-stem-x3 ") for d in rec.details), set(rec.details)
    recs = rec.take()
    found = check(recs)
    in_regions("fp32 stem", geom, [(r.tag, i) for r, i in zip(recs, found) if r.tag])


# ---- SN epilogue -------------------------------------------------------------------------------------------------------------------
def sn_bwd_plan(rps, S, cq):
    """csrc/spectral_norm.hip sn_bwd_plan: (chunks, rows per chunk) of one segment."""
    RL = 256 // cq
    ch = max(min((1024 + S - 1) // S, (rps + RL - 1) // RL), 1)
    rpc = (rps + ch - 1) // ch
    return (rps + rpc - 1) // rpc, rpc


@cases("case", [c + (S,) for c in SN_CASES for S in (1, 3)], lambda c: "%s-S%d" % (c[0], c[-1]))
def test_sn_block_slots(rec, golden_dir, case):
    """The SN block of tests/test_spectral_norm.py (convolution on W_bar + segmented epilogue), S = 1 and S = 3, forward and backward:
    every tag the block attaches (y, dz and whatever the convolution tags) describes its tensor."""
    S = case[-1]
    gold = np.load(os.path.join(golden_dir, "sn_ops.npz"))
    blk, gg = _sn_block(case[:-1], gold)
    x = gg("x").to(DEV).requires_grad_(True)
    y = blk(torch.cat([x] * S), segments=S) if S > 1 else blk(x)
    (y * torch.cat([gg("gy")] * S).to(DEV)).sum().backward()
    recs = rec.take()
    assert any("set_amax(y" in r.text and r.site[0] == "spectral.py" for r in recs)
    assert any("set_amax(dz" in r.text for r in recs)
    check(recs)


@cases("case", [(c[0], c[1], (c[3] + 3) // 4 * 4, c[4] // c[6], c[8], S) for c in SN_CASES for S in (1, 3)], ids_x)
def test_sn_epilogue_planted(rec, case):
    """The epilogue alone on the block shapes' Z (so that the peak can be steered): y = act(Z r_s + b) planted in Z, dZ = dy act'(y) r_s
    planted in dy; r_s differs per segment."""
    name, Bs, cp, H, act, S = case
    N = Bs * S
    rps = Bs * H * H
    chunks, rpc = sn_bwd_plan(rps, S, cp // 4)
    seed = N + cp + H
    r = torch.tensor([0.8, 1.0, 1.25][:S]).to(DEV)
    b = noise((cp,), seed, 0.05).to(DEV)
    w_bar = torch.empty(cp, 1, device=DEV)
    a = ops.ACT[act]
    # forward: a flat grid-stride loop (no row chunks); backward: (chunks, S) workgroups over the rows of each segment
    # (forward: the 'chunks' are the segments, where r_s changes; backward: the last chunk of the last segment)
    gf = geo(N, cp, H, H, rps, S, glob=True)
    gb = geo(N, cp, H, H, rpc, glob=True, lcr=(S - 1) * rps + (chunks - 1) * rpc)
    for way, geom in (("fwd", gf), ("bwd", gb)):
        for k, (region, (n, c, h, w_)) in enumerate(row_targets(geom)):
            z = noise((N, cp, H, H), seed + 10 + k, 0.3)
            dy = noise((N, cp, H, H), seed + 50 + k)
            if way == "fwd":
                z[n, c, h, w_] = PEAK
            else:
                dy[n, c, h, w_] = PEAK
            rs = r.cpu().double()[torch.arange(N) // Bs].view(N, 1, 1, 1)
            zr = z.double().requires_grad_(True)
            yr = orc.activation(zr * rs + b.cpu().double().view(1, -1, 1, 1), act)
            yr.backward(dy.double())
            assert _argmax(yr if way == "fwd" else zr.grad) == (n, c, h, w_), "planting recipe (%s)" % way
            before = len(rec.recs)
            zd = dcl(z).requires_grad_(True)
            y = spectral._SNEpilogue.apply(zd, b, w_bar, None, None, r, S, a)
            if way == "fwd":
                _of(rec.recs[before:], y).tag = (way, region)
            else:
                y.backward(dcl(dy))
                _of(rec.recs[before:], "set_amax(dz").tag = (way, region)
    recs = rec.take()
    found = check(recs)
    for way, geom in (("fwd", gf), ("bwd", gb)):
        in_regions("SN epilogue %s" % way, geom, [(t.tag[1], i) for t, i in zip(recs, found) if t.tag and t.tag[0] == way])


# ---- inherited tags ----------------------------------------------------------------------------------------------------------------
@single
def test_resampling_inherits_the_source_slot(rec):
    """ops.upsample2x / ops.downsample_half of a tagged tensor (tagged by a producer: an instance norm; and by amax_of): the slot is
    the source's, it holds max|source| bitwise, and the resampled tensor -- convex combinations -- does not exceed it.  An untagged
    source passes nothing on."""
    x = noise((2, 32, 12, 12), 3)
    x[1, 7, 5, 6] = PEAK
    with torch.no_grad():
        src = ops.instance_norm(dcl(x))
        up = ops.upsample2x(src)
        down = ops.downsample_half(src)
        meas = dcl(x)
        ops.amax_of(meas)
        up2, down2 = ops.upsample2x(meas), ops.downsample_half(meas)
        plain = ops.upsample2x(dcl(x))
    assert ops.amax_live(up)[0] == ops.amax_live(src)[0] == ops.amax_live(down)[0]
    assert ops.amax_live(up2)[0] == ops.amax_live(meas)[0] == ops.amax_live(down2)[0]
    assert ops.amax_live(plain) is None
    recs = rec.take()
    assert sum(r.kind == "pass" for r in recs) == 4
    check(recs)
    SUMMARY.setdefault("pass_amax (upsample2x, downsample_half)", set()).add("inherited")


# ---- filter slots ------------------------------------------------------------------------------------------------------------------
@single
def test_filter_slots_after_refresh(rec):
    """dwc_weight_refresh_multi raises each two-plane filter's own slot (the 8 bytes behind {s_w, 1/s_w} in the prepared tensor) in
    its first launch and derives s_w from it in the second.  After ops.refresh_prepared, and again after an in-place update that
    raises one filter's largest magnitude 8x: the slot carries the refresh's epoch and max|w| bitwise, and s_w is the power of two
    with s_w * max|w| in [2^13, 2^14) (the rule of h2_scale).  (tests/test_h2_parity.py test_h2_planes_reconstruct_the_weight holds the
    planes themselves and the same rule on the single-layout path, dwc_h2_weight_prepare; not repeated here.)"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(8)
    filters = [(torch.randn(64, 64, 3, 3, generator=g) * 0.05, ("h2_fwd", "h2_dgrad")),
               (torch.randn(128, 64, 4, 4, generator=g) * 3e-4, ("h2_fwd",)),
               (torch.randn(64, 128, 5, 5, generator=g) * 40.0, ("h2_fwd", "h2_dgrad"))]
    params = [torch.nn.Parameter(w.to(DEV)) for w, _ in filters]

    def tails():
        out = []
        for p, (_, kinds) in zip(params, filters):
            co, ci, K, _ = p.shape
            for kind in kinds:
                rows, kdim = (ci, co) if kind == "h2_dgrad" else (co, ci)
                prep = ops._prepped(p, kind, co, ci, 1)
                n = lib.dwc_h2_weight_prepared_elems(rows, kdim, K) - 8
                assert prep.numel() == n + 8
                out.append((p, kind, prep[n:n + 4].view(torch.float32), prep[n + 4:n + 8].view(torch.int64)))
        return out

    first = tails()                                        # lazily built: single-layout path, pool slots
    for round_ in range(2):
        with torch.no_grad():
            for i, p in enumerate(params):
                if round_ == 0:
                    p.mul_(1.0 + 0.01 * i)
                else:                                      # one element to 8x the filter's largest magnitude
                    p.view(-1)[17 + i] = -8.0 * p.abs().max()
        assert ops.refresh_prepared(params) == len(first)
        now = tails()
        assert all(a[2].data_ptr() == b[2].data_ptr() for a, b in zip(first, now)), "refreshed in place: no lazy rebuild behind it"
        wmax = torch.stack([p.detach().abs().max() for p, _, _, _ in now])
        sv = torch.stack([t for _, _, t, _ in now])
        words = torch.stack([s[0] for _, _, _, s in now])
        torch.cuda.synchronize()
        wbits, sv, words = wmax.view(torch.int32).cpu().numpy(), sv.double().cpu().numpy(), words.cpu().numpy()
        for k, (p, kind, _, _) in enumerate(now):
            word = int(words[k])
            assert (word >> 32) == ops._REFRESH_EPOCH, (kind, word >> 32, ops._REFRESH_EPOCH)
            assert (word & 0xffffffff) == int(wbits[k]), "%s %s: slot %#x, max|w| %#x" % (tuple(p.shape), kind, word & 0xffffffff, int(wbits[k]))
            s, inv = float(sv[k][0]), float(sv[k][1])
            m = float(np.int32(wbits[k]).view(np.float32))
            assert s > 0 and np.frexp(s)[0] == 0.5 and s * inv == 1.0, (s, inv)
            assert 2.0 ** 13 <= s * m < 2.0 ** 14, (kind, s, m)
    SUMMARY.setdefault("filter slots (dwc_weight_refresh_multi)", set()).add("refresh, 8x in-place update")


# ---- zero and non-finite outputs ---------------------------------------------------------------------------------------------------
@single
def test_all_zero_outputs_carry_the_epoch(rec):
    """A producer whose output is identically zero must still publish (magnitude 0 at the tag's epoch): ReLU over an all-negative
    pre-activation, dy == 0 for the backwards.  A consumer fed such a tensor -- one h2 forward -- returns finite values, not the NaN
    poison of a slot left at an old epoch."""
    B, C, H = 2, 64, 16
    x = noise((B, C, H, H), 1)
    w = (noise((C, C, 3, 3), 2, 0.05)).to(DEV)
    outs = []
    with torch.no_grad():
        outs.append(ops.instance_norm(dcl(x), torch.full((B * C,), 0.1, device=DEV), torch.full((B * C,), -5.0, device=DEV), relu=True))
        outs.append(ops.instance_norm(dcl(x[:, :, :12, :12]), torch.full((B * C,), 0.1, device=DEV), torch.full((B * C,), -5.0, device=DEV),
                                      relu=True))
        outs.append(ops.layer_norm_munit(dcl(x), torch.full((C,), 0.1, device=DEV), torch.full((C,), -5.0, device=DEV), relu=True))
        outs.append(ops.conv2d(dcl(x), w, torch.full((C,), -50.0, device=DEV), 1, 1, "relu"))
        outs.append(ops.conv2d_zeropad(dcl(x), w, torch.full((C,), -50.0, device=DEV), 1, "relu"))
        z = dcl(x)
        outs.append(spectral._SNEpilogue.apply(z, torch.full((C,), -50.0, device=DEV), torch.empty(C, 1, device=DEV), None, None,
                                               torch.ones(1, device=DEV), 1, ops.ACT["relu"]))
        n_launch = len(rec.details)
        fed = [ops.conv2d(y, w, None, 1, 1, "none") for y in outs]
    assert sum(d.startswith("fwd-h2 ") for d in rec.details[n_launch:]) >= len(outs) - 1      # (12 x 12 pixels: no two-plane form)
    for y in outs:
        assert ops.amax_live(y) is not None
    # backwards with dy == 0
    zero = torch.zeros(B, C, H, H, device=DEV).contiguous(memory_format=torch.channels_last)
    xd = dcl(x).requires_grad_(True)
    ops.instance_norm(xd, relu=True).backward(zero)
    xm = dcl(x[:, :, :12, :12]).requires_grad_(True)
    ops.instance_norm(xm).backward(zero[:, :, :12, :12].contiguous(memory_format=torch.channels_last))
    xl = dcl(x).requires_grad_(True)
    ops.layer_norm_munit(xl, torch.ones(C, device=DEV).requires_grad_(True), torch.zeros(C, device=DEV).requires_grad_(True)).backward(zero)
    xc = dcl(x).requires_grad_(True)
    ops.conv2d(xc, w.clone().requires_grad_(True), torch.zeros(C, device=DEV).requires_grad_(True), 1, 1, "lrelu").backward(zero)
    xs = dcl(x).requires_grad_(True)
    spectral._SNEpilogue.apply(xs, torch.zeros(C, device=DEV), torch.empty(C, 1, device=DEV), None, None, torch.ones(1, device=DEV), 1,
                               ops.ACT["tanh"]).backward(zero)
    recs = rec.take()
    fwd = {o.data_ptr() for o in outs + fed}
    bwd = [r for r in recs if any(k in r.text for k in ("set_amax(dx", "set_amax(g_out", "set_amax(dz"))]
    assert len(bwd) == 5, [r.text for r in bwd]
    zeros = bwd + [r for r in recs if r.t.data_ptr() in fwd]
    assert len(zeros) >= 2 * len(outs) - 1 + 5, [r.text for r in zeros]
    stack = torch.stack([r.t.detach().abs().max() for r in zeros])
    check(recs)
    assert float(stack.max()) == 0.0, "the cases are meant to produce all-zero tensors"
    for y in fed:
        assert torch.isfinite(y).all(), "a consumer of an all-zero tagged tensor returned non-finite values"


@cases("bad", [float("nan"), float("inf")], lambda v: str(v))
def test_non_finite_tensors_read_as_such(rec, bad):
    """One NaN / one inf in the input of an instance-norm apply (multi-pass and resident) and of an act backward: the produced tensor
    is non-finite and its slot says so (bits >= 0x7f800000), so that consumers pass the value on instead of scaling by a finite bound."""
    B, C = 2, 64
    for H in (12, 16):
        x = noise((B, C, H, H), 4)
        x[1, 9, 3, 4] = bad
        with torch.no_grad():
            y = ops.instance_norm(dcl(x))
        assert not torch.isfinite(y).all()
        xd = dcl(noise((B, C, H, H), 5)).requires_grad_(True)
        dy = noise((B, C, H, H), 6)
        dy[0, 63, H - 1, H - 1] = bad
        ops.instance_norm(xd).backward(dcl(dy))
        assert not torch.isfinite(xd.grad).all()
    xc = dcl(noise((B, C, 9, 9), 7)).requires_grad_(True)
    dy = noise((B, C, 9, 9), 8)
    dy[1, 0, 8, 8] = bad
    before = len(rec.recs)
    ops.conv2d(xc, noise((C, C, 3, 3), 9, 0.05).to(DEV), torch.full((C,), 0.5, device=DEV), 1, 1, "tanh").backward(dcl(dy))
    g = _of(rec.recs[before:], "set_amax(g_out")
    assert not torch.isfinite(g.t).all()
    recs = rec.take()
    check(recs)
    nonfinite = torch.stack([(~torch.isfinite(r.t)).any() for r in recs]).sum()
    assert int(nonfinite) >= 5


# ---- the whole step ----------------------------------------------------------------------------------------------------------------
@single
def test_whole_step_under_amax_check(rec, monkeypatch):
    """One dis_update + gen_update of the shipped network at 64 x 64, batch 4 (set up as tests/test_hip_parity.py
    test_full_size_iteration_vs_oracle) with DWC_AMAX_CHECK on: every tagged tensor is re-measured where a two-plane kernel consumes it.
    Covers the invariant of ops.set_amax -- nothing writes into a tensor after it was tagged -- in the real graph, which the per-op
    cases cannot; it must not raise, and the check must really have run in front of each kind of two-plane consumer."""
    from solver import Solver
    monkeypatch.setattr(ops, "AMAX_CHECK", 1)
    rec.keep = False
    S, B = 64, 4
    cfg = synth.make_config(image_size=S, lstm_dropout=0.0)
    host.set_noise(host.HostNoise())
    try:
        torch.manual_seed(1234)
        s = Solver(cfg, torch.device(DEV), None).to(DEV)
        s.copy_nets()
        batch = synth.make_batch(B, S, seed=11)
        db = {k: v.to(DEV) for k, v in batch.items()}
        a = (db["x_real"], db["c_src"], db["c_trg"], db["txt"], db["txt_lens"], db["label_src"], db["label_trg"], cfg, 0)
        s.dis_update(*a)
        s.gen_update(*a)
        torch.cuda.synchronize()
    finally:
        host.set_noise(host.DeviceNoise())
    assert np.isfinite(float(s.loss_dis_all.detach())) and np.isfinite(float(s.loss_gen_total.detach()))
    kinds = collections.Counter()
    for detail, n in rec.verified:
        word = detail.split()[0]
        stride2 = word.endswith("s2") or detail.split()[-1] == "s2"
        if word.startswith("wgrad-h2"):
            kinds["weight gradient"] += n
        if word in ("fwd-h2", "dgrad-h2"):
            kinds["stride-1"] += n
        if stride2 and "h2" in word:
            kinds["stride-2"] += n
    print("DWC_AMAX_CHECK verifications per consumer kind:", dict(kinds), "launch forms:", sorted({d.split()[0] for d, _ in rec.verified}))
    for kind in ("stride-1", "stride-2", "weight gradient"):
        assert kinds[kind] > 0, "no tagged operand was verified in front of a %s two-plane consumer: %s" % (kind, dict(kinds))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_amax_call_site_was_reached():
    """Every ``set_amax(`` / ``pass_amax(`` call site of hipdwc/ops.py, spectral.py and penalty.py was reached by a case above -- a
    producer added later cannot stay untested.  Exempt: the site inside amax_of (named in EXEMPT).  Judges only a run of all the
    module's cases."""
    missing = EXPECTED - RAN
    if missing:
        pytest.skip("%d of the module's %d cases did not run (a selection with -k?)" % (len(missing), len(EXPECTED)))
    assert len(EXEMPT) <= 2
    exempt = set()
    for (name, text), reason in EXEMPT.items():
        hits = [site for site, line in SITES.items() if site[0] == name and line == text]
        assert len(hits) == 1 and reason, (name, text, hits)
        exempt.add(hits[0])
    assert len(SITES) >= 12, "the scan lost call sites: %s" % sorted(SITES)
    missed = sorted(set(SITES) - SEEN - exempt)
    assert not missed, "set_amax / pass_amax call sites no case reached: " + "; ".join("%s:%d  %s" % (s[0], s[1], SITES[s]) for s in missed)
    print("\nproducer | regions whose planted peak matched bitwise")
    for k, v in SUMMARY.items():
        print("%s | %s" % (k, ", ".join(sorted(v))))
