"""GPU tests of the shared entry layer of the im2col convolutions (csrc/conv_im2col_entry.h, stamped for fp32 in conv_igemm.hip and
for bf16 in conv_bf16.hip): every export is called through the C ABI itself, so that no path selection of ops.py stands between the
test and the export, with prepared weights from ops._prepped and scratch of exactly the size the *_ws_bytes function returns.

Forward and weight-gradient cases first ask the plan queries (dwc_conv2d_fwd_plan / dwc_conv2d_bwd_weight_plan and their bf16 twins)
which tile, split and reduce the entry point will run and assert that it is the one the case is listed for: no test carries a copy
of the planner, and a planner change that moves a case off its branch fails the case instead of silently un-covering the branch.
test_forward_cases_cover_every_variant / test_weight_gradient_cases_cover_every_variant hold the union of the cases against the
list of variants that launch_gemm / wgrad_launch / wgrad_reduce can dispatch.

Reference: float64 torch.nn.functional.conv2d on the reflect-padded (zero-padded for the zeropad export) input, its weight gradient
from autograd in float64; for bf16 the activations, upstream gradients and weights are rounded to bf16 first.  Tolerances, relative
to the largest reference magnitude over the whole tensor: fp32 y 2e-5, fp32 dw 5e-5, stored bf16 y 6e-3, fp32 dw of the bf16 path
3e-4 (those of tests/test_hip_parity.py and tests/test_bf16_parity.py).

The bf16 128x128 tile is narrow ground: the 256-row tiles win nearly everywhere, and it is selected only where about 510 of its
workgroups exactly fill the chip twice (M near 10 800 rows with Cout 648..864 among the shapes of at most 8M outputs; found by
stepping Cout in eights through dwc_bf16_conv2d_fwd_plan).  Its cases sit there.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hipdwc import ops                       # noqa: E402
from hipdwc import _lib as _lib_mod          # noqa: E402

DEV = "cuda:0"
PREFIX = {"fp32": "dwc_", "bf16": "dwc_bf16_"}
# relative to the largest reference magnitude, whole tensor
TOL = {("fp32", "y"): 2e-5, ("fp32", "dw"): 5e-5, ("bf16", "y"): 6e-3, ("bf16", "dw"): 3e-4}
EINVAL, EWORKSPACE = -1, -2


def close(a, b, rel=2e-5, atol=1e-6, msg=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = rel * b.abs().max().item() + atol
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


def _rnd(prec):
    return (lambda t: t.to(torch.bfloat16).float()) if prec == "bf16" else (lambda t: t)


def _check(tag, prec, what, got, ref, plan):
    """Whole-tensor comparison at TOL; prints the figure the summary table is made of before asserting."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()          # (NaN -- an element the kernel left unwritten -- fails the comparison below)
    tol = TOL[(prec, what)]
    print("IM2COL-ENTRY %s %s plan=%s err/tol=%.3f" % (tag, what, plan, err / (tol * scale)))
    assert scale > 0 and err <= tol * scale, "%s %s: max err %.3e of scale, tolerance %.1e" % (tag, what, err / scale, tol)


class _x3_mode:
    """dwc_x3_gemm_mode is process-wide: set it for one launch and put the old value back."""

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.old = self.lib.dwc_x3_gemm_mode(-1)
        if self.mode is not None:
            self.lib.dwc_x3_gemm_mode(self.mode(self.old))
        return self

    def __exit__(self, *exc):
        self.lib.dwc_x3_gemm_mode(self.old)


# =====================================================================================================================================
# data gradient (moved from tests/test_hip_parity.py, unchanged)
# =====================================================================================================================================
# (entry point[:branch], k, stride, pad, Cin, Cout in fp32, Cout in bf16) at B = 1, H = W = 8; Cin 0: an image (4 / 8 planes).
# Cout is the smallest count that takes the branch: the split-K fold needs 8 K-slabs (9 * 32 / 32, 9 * 64 / 64), same_dgrad_geom
# needs Cout >= 32 and >= one K-slab (32 / 64), image_dgrad_geom Cout >= 32.
IM2COL_DGRAD_CASES = [
    ("bwd_data_fold:direct", 3, 1, 1, 8, 8, 8),
    ("bwd_data_fold:splitk", 3, 1, 1, 8, 32, 64),
    ("bwd_data_same", 3, 1, 1, 8, 32, 64),
    ("bwd_data_same", 5, 1, 2, 8, 32, 64),
    ("bwd_data_ring", 3, 1, 1, 8, 32, 64),
    ("bwd_data_ring", 5, 1, 2, 8, 32, 64),
    ("bwd_data_s2_ring", 4, 2, 1, 8, 8, 8),
    ("bwd_data_image", 7, 1, 3, 0, 32, 32),
]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", IM2COL_DGRAD_CASES, ids=lambda c: "%s-k%d" % (c[0].replace(":", "-"), c[1]))
def test_im2col_data_gradient_entry_points(case, prec):
    """Every data-gradient entry point of the im2col files (csrc/conv_im2col_entry.h), called through the C ABI itself so that no
    path selection of ops.py stands between the test and the export, in both precisions and on both branches of bwd_data_fold
    (direct: interior cropped into dx + band fold; split-K: padded image + whole-image fold).  Against the float64 gradient of the
    reflect-padded convolution.  The ring entry points add the folded border ring to a dx that already holds the interior: the test
    supplies the float64 interior (the crop of the padded image's gradient)."""
    what, k, s, p, ci, co32, co16 = case
    half = prec == "bf16"
    B, H = 1, 8
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        dt = ops.act_dtype()
        co, ci = (co16 if half else co32), ci or ops.image_planes(dt)
        rnd = (lambda t: t.to(torch.bfloat16).float()) if half else (lambda t: t)
        g = torch.Generator().manual_seed(k + 10 * p + co)
        w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (co * k * k) ** 0.5)
        Ho = (H + 2 * p - k) // s + 1
        gy = rnd(torch.randn(B, co, Ho, Ho, generator=g))
        xr = torch.zeros(B, ci, H, H, dtype=torch.float64, requires_grad=True)       # (the gradient does not depend on x)
        xp = torch.nn.functional.pad(xr, (p, p, p, p), mode="reflect")
        xp.retain_grad()
        (torch.nn.functional.conv2d(xp, rnd(w).double(), None, stride=s) * gy.double()).sum().backward()
        ref, inner = xr.grad.float(), xp.grad[:, :, p:-p, p:-p].float()
        assert (ref - inner).abs().max().item() > 0.1 * ref.abs().max().item()       # the ring matters at this size

        gd = gy.to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
        wd = w.to(DEV)
        dx = ops.empty_cl(B, ci, H, H, gd.device, dt)
        st, Hp = ops._stream(), H + 2 * p
        fn = lambda name: ops._fn(lib, "conv2d_" + name, gd)
        prepped = lambda kind: ops._prepped(wd, kind, co, ci, s, None, half).data_ptr()
        scratch = lambda n: torch.empty(max(int(n), 1), dtype=torch.uint8, device=DEV)
        name = what.split(":")[0]
        if name == "bwd_data_fold":
            nws = fn("bwd_data_ws_bytes")(B, H, H, ci, co, k, k, s, p)
            assert (nws > 0) == what.endswith("splitk"), (what, nws)
            dxp, ws = scratch(B * Hp * Hp * ci * dx.element_size()), scratch(nws)
            rc = fn(name)(gd.data_ptr(), prepped("dgrad"), dxp.data_ptr(), dx.data_ptr(), B, H, H, ci, co, k, k, s, p,
                          ws.data_ptr() if nws else None, nws, st)
        elif name in ("bwd_data_same", "bwd_data_ring"):
            nws = fn("bwd_data_same_ws_bytes")(B, H, H, ci, co, k, k, p)
            assert nws > 0
            ws = scratch(nws)
            if name == "bwd_data_ring":
                dx.copy_(inner)
            rc = fn(name)(gd.data_ptr(), prepped("dgrad"), prepped("dgrad_t"), dx.data_ptr(), B, H, H, ci, co, k, k, p, ws.data_ptr(),
                          nws, st)
        elif name == "bwd_data_s2_ring":
            dxp = scratch(B * Hp * Hp * ci * dx.element_size())
            dx.copy_(inner)
            rc = fn(name)(gd.data_ptr(), prepped("dgrad"), dxp.data_ptr(), dx.data_ptr(), B, H, H, ci, co, st)
        else:
            nws = fn("bwd_data_image_ws_bytes")(B, H, H, co, k, k, p)
            assert nws > 0
            ws = scratch(nws)
            rc = fn(name)(gd.data_ptr(), prepped("dgrad_image"), dx.data_ptr(), B, H, H, co, k, k, p, ws.data_ptr(), nws, st)
        _lib_mod.check(rc, name)
        # (the dx tolerances of test_conv_forward_backward and of tests/test_bf16_parity.py: a stored bf16 tensor)
        close(dx, ref, rel=6e-3 if half else 5e-5, msg=what)
    finally:
        ops.set_precision("fp32")


# =====================================================================================================================================
# forward
# =====================================================================================================================================
# A forward geometry is (B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w); the epilogue "bias+lrelu" or "none" (no bias).
def _sq(B, H, W, ci, co, k=3, s=1, p=1):
    return (B, H, W, ci, co, k, k, s, s, p, p)


def _out_hw(geom):
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    return (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1


@functools.lru_cache(maxsize=2)
def _fwd_reference(prec, geom, epi, zeropad):
    """(x, w, bias or None, float64 y) of one case; the cases of one geometry follow each other and share it."""
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    rnd = _rnd(prec)
    g = torch.Generator().manual_seed(sum(geom) * 7 + len(epi))
    x = rnd(torch.randn(B, ci, H, W, generator=g))
    w = torch.randn(co, ci, kh, kw, generator=g) * (1.0 / (ci * kh * kw) ** 0.5)
    b = torch.randn(co, generator=g) * 0.5 if epi == "bias+lrelu" else None
    xp = x.double()
    if ph or pw:
        xp = F.pad(xp, (pw, pw, ph, ph), mode="constant" if zeropad else "reflect")
    y = F.conv2d(xp, rnd(w).double(), None if b is None else b.double(), stride=(sh, sw))
    if epi == "bias+lrelu":
        y = F.leaky_relu(y, 0.1)
    return x, w, b, y


def _launch_fwd(lib, prec, export, geom, x, w, b, epi, ws_mode):
    """Calls dwc_[bf16_]conv2d_<export>; returns (rc, y as it left the device, filled with NaN beforehand)."""
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    half, dt = prec == "bf16", ops.act_dtype()
    Ho, Wo = _out_hw(geom)
    xd = x.to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
    wd = w.to(DEV)
    wp = ops._prepped(wd, "fwd", co, ci, 1, None, half)
    bd = None if b is None else b.to(DEV)
    y = ops.empty_cl(B, co, Ho, Wo, DEV, dt)
    y.fill_(float("nan"))
    act = ops.ACT["lrelu" if epi == "bias+lrelu" else "none"]
    fn = lambda name: ops._fn(lib, "conv2d_" + name, xd)
    head = (xd.data_ptr(), wp.data_ptr(), None if bd is None else bd.data_ptr(), y.data_ptr(), B, H, W, ci, co, kh, kw)
    if export == "fwd_ex":
        rc = fn(export)(*head, sh, sw, ph, pw, act, ops._stream())
    else:
        assert sh == sw and ph == pw
        nws = fn("fwd_ws_bytes")(B, H, W, ci, co, kh, kw, sh, ph)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=DEV)
        if ws_mode == "none":
            rc = fn(export)(*head, sh, ph, act, None, 0, ops._stream())
        else:
            rc = fn(export)(*head, sh, ph, act, ws.data_ptr() if nws else None, nws, ops._stream())
    torch.cuda.synchronize()
    return rc, y


# fp32 variants of launch_gemm: "native" = the fp32 MFMA kernels because K < 128, "x3" = the split-product kernels (K >= 128, bit 0 of
# dwc_x3_gemm_mode on: a 128x128 plan runs on the 128x64 kernel), "mode0" = the native kernels on the K >= 128 shapes through
# dwc_x3_gemm_mode(0).  bf16 has the one variant.
X3_MODES = {"native": None, "x3": lambda old: old | 1, "mode0": lambda old: 0, "bf16": None}

# (B, H, W, Cout), epilogue, the tile the shape is listed for: 3x3 reflect-pad-1 convolutions, unsplit.  Per large tile one map whose Wo
# and Ho*Wo are powers of two (fwd_geom's shifts) and one odd map with M % bm != 0; Cout leaves a partial column tile; B > 1.
_F32_UNSPLIT = [
    ((5, 64, 64, 264), "bias+lrelu", (128, 128)),
    ((4, 111, 113, 96), "none", (128, 128)),
    ((2, 128, 128, 96), "none", (128, 64)),
    ((2, 111, 113, 96), "bias+lrelu", (128, 64)),
    ((2, 16, 16, 40), "bias+lrelu", (64, 64)),
    ((2, 21, 19, 40), "none", (64, 64)),
    ((2, 16, 16, 8), "none", (128, 32)),
    ((2, 21, 19, 8), "bias+lrelu", (128, 32)),
]
_BF16_UNSPLIT = [
    ((5, 128, 64, 136), "bias+lrelu", (256, 256)),
    ((3, 127, 93, 136), "none", (256, 256)),
    ((5, 75, 61, 264), "bias+lrelu", (256, 256)),          # two column tiles
    ((3, 128, 64, 136), "none", (256, 128)),
    ((4, 97, 95, 96), "bias+lrelu", (256, 128)),
    ((3, 60, 60, 648), "bias+lrelu", (128, 128)),          # 85 row tiles (the last holds 48 rows) x 6 column tiles (the last 8 columns)
    ((85, 16, 8, 648), "none", (128, 128)),
    ((1, 128, 128, 96), "bias+lrelu", (128, 64)),
    ((2, 75, 61, 96), "none", (128, 64)),
    ((2, 16, 16, 40), "bias+lrelu", (64, 64)),
    ((2, 21, 19, 40), "none", (64, 64)),
    ((2, 16, 16, 8), "none", (128, 32)),
    ((2, 21, 19, 8), "bias+lrelu", (128, 32)),
]
# split-K: (B, H, W, Cin, Cout, k, stride, pad), tile.  Long contractions on few rows ('valid' 4x4 heads on a 4x4 map: K = 4096 / 8192),
# ragged reflect-padded 3x3 maps, and the 1x1 convolutions on which the fp32 planner splits its 128-row tiles (M % 128 and Cout % bn
# both non-zero).  Every case runs with bias + lrelu (applied by splitk_reduce) and again with ws = NULL (the unsplit fallback).
_F32_SPLIT = [
    ((3, 4, 4, 256, 128, 4, 1, 0), (64, 64)),
    ((5, 9, 7, 128, 104, 3, 1, 1), (64, 64)),
    ((3, 4, 4, 512, 8, 4, 1, 0), (128, 32)),
    ((5, 9, 7, 128, 24, 3, 1, 1), (128, 32)),
    ((7, 31, 33, 256, 488, 1, 1, 0), (128, 64)),
    ((7, 31, 33, 256, 1000, 1, 1, 0), (128, 128)),
]
_BF16_SPLIT = [
    ((3, 4, 4, 256, 128, 4, 1, 0), (64, 64)),
    ((5, 9, 7, 128, 104, 3, 1, 1), (64, 64)),
    ((3, 4, 4, 512, 8, 4, 1, 0), (128, 32)),
    ((5, 9, 7, 128, 24, 3, 1, 1), (128, 32)),
]

# (precision, variant, geometry, epilogue, (bm, bn), split plan?, "exact" scratch or "none")
FWD_CASES = []
for (_B, _H, _W, _co), _epi, _tile in _F32_UNSPLIT:
    for _mode, _ci in (("native", 8), ("x3", 16), ("mode0", 16)):
        FWD_CASES.append(("fp32", _mode, _sq(_B, _H, _W, _ci, _co), _epi, _tile, False, "exact"))
for (_B, _H, _W, _co), _epi, _tile in _BF16_UNSPLIT:
    FWD_CASES.append(("bf16", "bf16", _sq(_B, _H, _W, 16, _co), _epi, _tile, False, "exact"))
for _prec, _table in (("fp32", _F32_SPLIT), ("bf16", _BF16_SPLIT)):
    for (_B, _H, _W, _ci, _co, _k, _s, _p), _tile in _table:
        for _mode in (("x3", "mode0") if _prec == "fp32" else ("bf16",)):
            for _ws in ("exact", "none"):
                FWD_CASES.append((_prec, _mode, _sq(_B, _H, _W, _ci, _co, _k, _s, _p), "bias+lrelu", _tile, True, _ws))


def _fwd_id(c):
    prec, mode, geom, epi, tile, split, ws = c
    return "%s-%dx%d%s%s-%s-%s" % (mode if prec == "fp32" else prec, tile[0], tile[1], "-split" if split else "",
                                    "-nows" if ws == "none" else "", "x".join(str(v) for v in geom[:5]) + "k%d" % geom[5], epi)


def _fwd_plan(prec, geom):
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    assert sh == sw and ph == pw
    return _lib_mod.plan(PREFIX[prec] + "conv2d_fwd_plan", B, H, W, ci, co, kh, kw, sh, ph)


def _fwd_state(plan, ws):
    return "unsplit" if plan[2] == 1 else ("split" if ws == "exact" else "fallback")


@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_forward_every_tile_and_split(case):
    """dwc_conv2d_fwd / dwc_bf16_conv2d_fwd on every kernel instantiation launch_gemm can dispatch: the plan query names the tile and
    split before the launch, the result is held to float64 over the whole tensor.  A split plan is run with its exact scratch (partials
    summed, bias and activation applied by splitk_reduce) and with ws = NULL, where the launch must fall back to the unsplit kernel,
    return DWC_OK and meet the same tolerance."""
    prec, mode, geom, epi, tile, split, ws = case
    K = geom[3] * geom[5] * geom[6]
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        plan = _fwd_plan(prec, geom)
        assert plan[:2] == tile and (plan[2] > 1) == split, (case, plan)
        assert (K < 128) == (mode == "native") or prec == "bf16", (mode, K)
        nws = getattr(lib, PREFIX[prec] + "conv2d_fwd_ws_bytes")(*geom[:7], geom[7], geom[9])
        Ho, Wo = _out_hw(geom)
        assert nws == (plan[2] * geom[0] * Ho * Wo * geom[4] * 4 if split else 0)
        x, w, b, ref = _fwd_reference(prec, geom, epi, False)
        with _x3_mode(lib, X3_MODES[mode]):
            if mode == "x3":
                assert lib.dwc_x3_gemm_mode(-1) & 1
            elif mode == "mode0":
                assert lib.dwc_x3_gemm_mode(-1) == 0
            rc, y = _launch_fwd(lib, prec, "fwd", geom, x, w, b, epi, ws)
        assert rc == 0, rc
        _check(_fwd_id(case), prec, "y", y, ref, "%dx%d s%d kt%d %s" % (plan + (_fwd_state(plan, ws),)))
    finally:
        ops.set_precision("fp32")


def _is_pow2(n):
    return n > 0 and n & (n - 1) == 0


def test_forward_cases_cover_every_variant():
    """The union of FWD_CASES, with the plan of each case taken from the query: every TileCand of both policies in every variant and
    split state launch_gemm can dispatch it in, and on each large tile the edges where tiled GEMMs go wrong."""
    seen, edges = set(), {}
    for prec, mode, geom, epi, tile, split, ws in FWD_CASES:
        plan = _fwd_plan(prec, geom)
        seen.add((prec, mode, plan[0], plan[1], _fwd_state(plan, ws)))
        Ho, Wo = _out_hw(geom)
        M, N = geom[0] * Ho * Wo, geom[4]
        e = edges.setdefault((prec, plan[0], plan[1]), set())
        e.update(["M%bm" if M % plan[0] else "M|bm", "N%bn" if N % plan[1] else "N|bn",
                  "pow2 map" if _is_pow2(Wo) and _is_pow2(Ho * Wo) else "odd map", epi, "B>1" if geom[0] > 1 else "B=1"])
    f32_tiles = [(128, 128), (128, 64), (64, 64), (128, 32)]                        # Im2colF32::TILES
    bf16_tiles = [(256, 256), (256, 128), (128, 128), (128, 64), (64, 64), (128, 32)]   # Im2colBF16::TILES
    want = set()
    for bm, bn in f32_tiles:
        want.add(("fp32", "native", bm, bn, "unsplit"))
        for mode in ("x3", "mode0"):                       # every fp32 tile can be split
            want.update(("fp32", mode, bm, bn, state) for state in ("unsplit", "split", "fallback"))
    for bm, bn in bf16_tiles:
        want.add(("bf16", "bf16", bm, bn, "unsplit"))
    for bm, bn in ((64, 64), (128, 32)):                   # the tiles the bf16 planner can split
        want.update(("bf16", "bf16", bm, bn, state) for state in ("split", "fallback"))
    assert not want - seen, sorted(want - seen)
    for key in [("fp32",) + t for t in f32_tiles[:2]] + [("bf16",) + t for t in bf16_tiles[:4]]:
        missing = {"M%bm", "N%bn", "pow2 map", "odd map", "bias+lrelu", "none", "B>1"} - edges[key]
        assert not missing, (key, sorted(missing))


# ---- zero-padded forward ------------------------------------------------------------------------------------------------------------
# (precision, geometry, epilogue, tile): one large tile with a ragged last row tile and one small ragged map each
ZEROPAD_CASES = [
    ("fp32", _sq(4, 111, 113, 16, 96), "bias+lrelu", (128, 128)),
    ("fp32", _sq(2, 21, 19, 16, 40), "none", (64, 64)),
    ("bf16", _sq(4, 97, 95, 16, 96), "bias+lrelu", (256, 128)),
    ("bf16", _sq(2, 21, 19, 16, 40), "none", (64, 64)),
]


@pytest.mark.parametrize("case", ZEROPAD_CASES, ids=lambda c: "%s-%dx%d" % (c[0], c[3][0], c[3][1]))
def test_forward_zeropad(case):
    """dwc_conv2d_fwd_zeropad (the zero rule of the same kernels: nn.Conv2d(padding=1)) away from VGG's own shapes, against float64 on
    the zero-padded input.  It plans as dwc_conv2d_fwd does."""
    prec, geom, epi, tile = case
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        plan = _fwd_plan(prec, geom)
        assert plan[:2] == tile and plan[2] == 1, (case, plan)
        x, w, b, ref = _fwd_reference(prec, geom, epi, True)
        top = x[:1, :, :3].double()                          # (the two pad rules differ on the border: first output row of image 0)
        assert (F.conv2d(F.pad(top, (1, 1, 1, 0), mode="reflect"), w.double()) - F.conv2d(F.pad(top, (1, 1, 1, 0)), w.double())).abs().max() > 0.1
        rc, y = _launch_fwd(lib, prec, "fwd_zeropad", geom, x, w, b, epi, "exact")
        assert rc == 0, rc
        _check("zeropad-%s-%dx%d" % ((prec,) + tile), prec, "y", y, ref, "%dx%d s%d kt%d" % plan)
    finally:
        ops.set_precision("fp32")


# ---- per-axis stride and pad --------------------------------------------------------------------------------------------------------
# The geometry of the 8-pixels-per-row image heads as ops.py calls it (7 x 14 filter bank, stride (1, 8), pad (3, 3), 32 columns), on a
# map 40 wide (5 groups of 8: no multiple of a row tile), and a stride that differs between the axes.
# (name, geometry, epilogue, the tile the case is listed for in both precisions)
EX_CASES = [
    ("heads-s1x8", (2, 13, 40, 16, 32, 7, 14, 1, 8, 3, 3), "bias+lrelu", (128, 32)),
    ("s2x1", (3, 17, 15, 16, 40, 3, 3, 2, 1, 1, 1), "none", (64, 64)),
    ("s1x3-pad2x0", (2, 9, 14, 16, 96, 5, 2, 1, 3, 2, 0), "bias+lrelu", (64, 64)),
]


def _ex_as_valid(geom):
    """The 'valid' stride-1 convolution with the M, K and N of an _ex geometry: the planners see only those, so the plain plan queries
    answer for the _ex exports too."""
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    Ho, Wo = _out_hw(geom)
    return (B, Ho + kh - 1, Wo + kw - 1, ci, co, kh, kw, 1, 0)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", EX_CASES, ids=lambda c: c[0])
def test_forward_ex(case, prec):
    """dwc_conv2d_fwd_ex: per-axis stride and reflect pad, never split (it takes no scratch).  The tile is asserted from the plan
    query of the 'valid' convolution with the same M, K and N (launch_gemm plans from g.M, o.N and g.K alone)."""
    name, geom, epi, tile = case
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        plan = _lib_mod.plan(PREFIX[prec] + "conv2d_fwd_plan", *_ex_as_valid(geom))
        assert plan[:2] == tile, (case, prec, plan)
        x, w, b, ref = _fwd_reference(prec, geom, epi, False)
        rc, y = _launch_fwd(lib, prec, "fwd_ex", geom, x, w, b, epi, "none")
        assert rc == 0, rc
        _check("fwd_ex-%s-%s" % (prec, name), prec, "y", y, ref, "%dx%d s%d kt%d (run unsplit)" % plan)
    finally:
        ops.set_precision("fp32")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_ex_rejects_a_second_reflection(prec):
    """A pad as large as the map would need a second reflection: DWC_EINVAL, and nothing is launched (y keeps its fill)."""
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        for geom in ((1, 6, 5, 16, 32, 3, 11, 1, 1, 1, 5), (1, 3, 9, 16, 32, 7, 3, 1, 1, 3, 1)):
            B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
            dt = ops.act_dtype()
            xd = torch.zeros((B, ci, H, W), dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last)
            wp = torch.zeros(co * 2048, dtype=dt, device=DEV)
            y = torch.full((B * co * 64 * 64,), 7.0, dtype=dt, device=DEV)
            rc = ops._fn(lib, "conv2d_fwd_ex", xd)(xd.data_ptr(), wp.data_ptr(), None, y.data_ptr(), B, H, W, ci, co, kh, kw, sh, sw, ph, pw,
                                                   0, ops._stream())
            torch.cuda.synchronize()
            assert rc == EINVAL, (geom, rc)
            assert bool((y == 7.0).all())
    finally:
        ops.set_precision("fp32")


# =====================================================================================================================================
# weight gradient
# =====================================================================================================================================
# (B, H, W) of 3x3 reflect-pad-1 convolutions by the number of pixel ranges they are listed for; bf16 slabs are 64 pixels, so the bf16
# maps hold about twice the pixels.  "below": M under one slab; "one": one range, M no multiple of the slab; "few": 2..15 ranges
# (plain reduce), the last one short; "many": >= 16 ranges.
_WG_MAPS = {
    "fp32": {"below": (1, 3, 5), "one": (3, 3, 5), "few": (3, 13, 15), "many": (3, 37, 41)},
    "bf16": {"below": (1, 3, 5), "one": (5, 3, 5), "few": (5, 13, 15), "many": (3, 64, 61)},
}
# fp32 runs with bit 1 of dwc_x3_gemm_mode on ("x3": split products) and off ("native")
WG_MODES = {"native": lambda old: old & ~2, "x3": lambda old: old | 2, "bf16": None}

# (precision, variant, (B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w), cin_real, cout_real, bn, splits class, wide reduce)
WGRAD_CASES = []
for _prec in ("fp32", "bf16"):
    for _mode in (("x3", "native") if _prec == "fp32" else ("bf16",)):
        for _co, _bn in ((96, 128), (40, 64), (24, 32)):
            for _cls in ("below", "one", "few", "many"):
                WGRAD_CASES.append((_prec, _mode, _sq(*_WG_MAPS[_prec][_cls], 16, _co), 16, _co, _bn, _cls, _cls == "many"))
        # seven ranges (the other "few" cases have two), a full 128-column tile
        WGRAD_CASES.append((_prec, _mode, _sq(2 if _prec == "fp32" else 4, 32, 31, 16, 128), 16, 128, 128, "few", False))
        # >= 16 ranges of more than 262144 elements: the plain reduce
        WGRAD_CASES.append((_prec, _mode, _sq(*_WG_MAPS[_prec]["many"], 128, 256), 128, 256, 128, "many", False))
        # an image with 3 real planes and one real output channel, reduced by the plain and by the wide form
        _pl = 4 if _prec == "fp32" else 8
        WGRAD_CASES.append((_prec, _mode, _sq(*_WG_MAPS[_prec]["few"], _pl, _pl), 3, 1, 32, "few", False))
        WGRAD_CASES.append((_prec, _mode, _sq(*_WG_MAPS[_prec]["many"], _pl, _pl), 3, 1, 32, "many", True))
        # the _ex form on the geometry of the image heads (stride (1, 8))
        WGRAD_CASES.append((_prec, _mode, (2, 13, 40, 16, 32, 7, 14, 1, 8, 3, 3), 16, 32, 32, "one", False))


def _wg_id(c):
    prec, mode, geom, cir, cor, bn, cls, wide = c
    return "%s-bn%d-%s%s-%s-real%dx%d" % (mode, bn, cls, "-wide" if wide else "", "x".join(str(v) for v in geom[:5]) + "k%dx%d" % geom[5:7],
                                          cir, cor)


def _wg_is_ex(geom):
    return geom[7] != geom[8] or geom[9] != geom[10]


def _wg_plan(prec, geom):
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    shape = _ex_as_valid(geom) if _wg_is_ex(geom) else (B, H, W, ci, co, kh, kw, sh, ph)
    return _lib_mod.plan(PREFIX[prec] + "conv2d_bwd_weight_plan", *shape)


def _wg_class(prec, geom, plan):
    Ho, Wo = _out_hw(geom)
    M, slab = geom[0] * Ho * Wo, 32 if prec == "fp32" else 64
    if plan[1] == 1:
        return "below" if M < slab else "one"
    return "few" if plan[1] < 16 else "many"


@functools.lru_cache(maxsize=2)
def _wg_reference(prec, geom):
    """(x, dy, float64 dw) of one case: dw from autograd through the float64 convolution of the reflect-padded input."""
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    rnd = _rnd(prec)
    Ho, Wo = _out_hw(geom)
    g = torch.Generator().manual_seed(sum(geom) * 11)
    x = rnd(torch.randn(B, ci, H, W, generator=g))
    gy = rnd(torch.randn(B, co, Ho, Wo, generator=g))
    w = torch.zeros(co, ci, kh, kw, dtype=torch.float64, requires_grad=True)
    (F.conv2d(F.pad(x.double(), (pw, pw, ph, ph), mode="reflect"), w, None, stride=(sh, sw)) * gy.double()).sum().backward()
    return x, gy, w.grad


SENTINEL = -12345.0


def _launch_wgrad(lib, prec, geom, x, gy, cir, cor, short=0):
    """Calls dwc_[bf16_]conv2d_bwd_weight[_ex] with scratch of exactly *_ws_bytes (minus `short`); returns (rc, the dw buffer, which
    is the padded filter's size and pre-filled with SENTINEL, the count of elements the contract lets the export write)."""
    B, H, W, ci, co, kh, kw, sh, sw, ph, pw = geom
    dt = ops.act_dtype()
    xd = x.to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
    gd = gy.to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
    dw = torch.full((co * ci * kh * kw + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    fn = lambda name: ops._fn(lib, "conv2d_" + name, xd)
    if _wg_is_ex(geom):
        nws = fn("bwd_weight_ex_ws_bytes")(B, H, W, ci, co, kh, kw, sh, sw, ph, pw)
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        rc = fn("bwd_weight_ex")(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), B, H, W, ci, co, kh, kw, sh, sw, ph, pw, cir, cor,
                                 ws.data_ptr(), nws - short, ops._stream())
    else:
        nws = fn("bwd_weight_ws_bytes")(B, H, W, ci, co, kh, kw, sh, ph)
        ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        rc = fn("bwd_weight")(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), B, H, W, ci, co, kh, kw, sh, ph, cir, cor, ws.data_ptr(),
                              nws - short, ops._stream())
    torch.cuda.synchronize()
    return rc, dw, cor * cir * kh * kw, nws


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_wg_id)
def test_weight_gradient_every_kernel_and_reduce(case):
    """dwc_conv2d_bwd_weight / _ex and their bf16 twins on the three kernels of wgrad_launch crossed with one range, a few ranges (plain
    reduce) and many (wide reduce, or plain above 262144 elements), the plan asserted from the query.  dw is [cout_real][cin_real][KH][KW]
    densely (wgrad_reduce_kernel and its wide form skip the padded channels): the buffer is as large as the padded filter and pre-filled,
    and everything behind the real part must keep the fill -- padded channels of x and dy hold random values here, which must reach
    neither the real rows nor the tail."""
    prec, mode, geom, cir, cor, bn, cls, wide = case
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        plan = _wg_plan(prec, geom)
        assert plan[0] == bn and _wg_class(prec, geom, plan) == cls and bool(plan[3]) == wide, (case, plan)
        Ho, Wo = _out_hw(geom)
        M = geom[0] * Ho * Wo
        assert M % plan[2] != 0, "the last range is meant to be short"
        x, gy, ref = _wg_reference(prec, geom)
        with _x3_mode(lib, WG_MODES[mode]):
            if prec == "fp32":
                assert bool(lib.dwc_x3_gemm_mode(-1) & 2) == (mode == "x3")
            rc, dw, real, nws = _launch_wgrad(lib, prec, geom, x, gy, cir, cor)
        assert rc == 0, rc
        assert nws == plan[1] * geom[3] * geom[4] * geom[5] * geom[6] * 4
        assert bool((dw[real:] == SENTINEL).all()), "written behind the real filter"
        got = dw[:real].view(cor, cir, geom[5], geom[6])
        _check(_wg_id(case), prec, "dw", got, ref[:cor, :cir], "bn%d s%d chunk%d %s" % (plan[:3] + ("wide" if plan[3] else "plain",)))
    finally:
        ops.set_precision("fp32")


def test_weight_gradient_cases_cover_every_variant():
    """The union of WGRAD_CASES by the plan query: each of the three kernels x {below one slab, one range, 2..15 ranges, >= 16 ranges
    on the wide reduce} in fp32 with split products, fp32 native and bf16, and >= 16 ranges on the plain reduce once per variant."""
    seen = set()
    for prec, mode, geom, cir, cor, bn, cls, wide in WGRAD_CASES:
        plan = _wg_plan(prec, geom)
        seen.add((mode, plan[0], _wg_class(prec, geom, plan), bool(plan[3])))
    want = set()
    for mode in ("x3", "native", "bf16"):
        for bn in (128, 64, 32):
            want.update((mode, bn, cls, False) for cls in ("below", "one", "few"))
            want.add((mode, bn, "many", True))
        want.add((mode, 128, "many", False))
    assert not want - seen, sorted(want - seen)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_weight_gradient_return_codes(prec):
    """DWC_EWORKSPACE with scratch one byte short, for a single range and for many, and DWC_EINVAL for 4 output channels in bf16: both
    return before any launch (dw keeps its fill)."""
    ops.set_precision(prec)
    try:
        lib = _lib_mod.load()
        for cls in ("one", "many"):
            geom = _sq(*_WG_MAPS[prec][cls], 16, 40)
            Ho, Wo = _out_hw(geom)
            x, gy = torch.zeros(geom[0], 16, geom[1], geom[2]), torch.zeros(geom[0], 40, Ho, Wo)
            rc, dw, real, nws = _launch_wgrad(lib, prec, geom, x, gy, 16, 40, short=1)
            assert rc == EWORKSPACE, (cls, rc)
            assert bool((dw == SENTINEL).all())
        if prec == "bf16":
            geom = _sq(2, 8, 8, 8, 4)
            with pytest.raises(_lib_mod.HipKernelError):
                _wg_plan(prec, geom)
            dt = ops.act_dtype()
            xd = torch.zeros((2, 8, 8, 8), dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last)
            gd = torch.zeros((2, 4, 8, 8), dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last)
            dw = torch.full((4 * 8 * 9,), SENTINEL, dtype=torch.float32, device=DEV)
            ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
            rc = lib.dwc_bf16_conv2d_bwd_weight(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), 2, 8, 8, 8, 4, 3, 3, 1, 1, 8, 4, ws.data_ptr(),
                                                ws.numel(), ops._stream())
            torch.cuda.synchronize()
            assert rc == EINVAL, rc
            assert bool((dw == SENTINEL).all())
    finally:
        ops.set_precision("fp32")
