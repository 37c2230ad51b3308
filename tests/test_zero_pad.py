"""``pad_type: zero`` inside the HIP convolutions: the zero rule of the im2col entry points (stride-2 forward, weight gradient, data
gradient with the scatter's crop), of ops.conv2d(pad_mode='zero') on the halo kernels that take the rule, and of Conv2dBlock /
ResBlock / the fused image heads.

Reference: float64 ``F.conv2d(x, w, b, stride, padding=p)`` and its autograd on the CPU; for bf16 the activations, upstream gradients
and weights are rounded to bf16 first.  Tolerances are those the reflect forms of the same kernels are held to, relative to the
largest reference magnitude over the whole tensor -- the zero rule replaces products by exact zeros, so none is loosened:
  * im2col entries (tests/test_im2col_entry_points.py::_check and its data-gradient test): fp32 y 2e-5, dx 5e-5, dw 5e-5; stored bf16
    y and dx 6e-3, fp32 dw of the bf16 path 3e-4;
  * two-plane f16 halo kernels (tests/test_h2_parity.py, tests/test_x3_parity.py): y 5e-6, the data-gradient interior (stride 1 and
    the four parity classes of stride 2) 2e-6;
  * bf16 halo kernels (tests/test_bf16_parity.py): stored bf16 y and dx 6e-3, fp32 dw 3e-4;
  * Conv2dBlock (tests/test_hip_parity.py::test_conv_block_beyond_shipped_configs_vs_reference, tests/test_spectral_norm.py): y 5e-5
    (+2e-6), every gradient 3e-4 (+2e-6);
  * ResBlock grouped against concatenated (tests/test_lrelu_fused.py): y 2e-6, gradients 2e-5 of the tensor's largest magnitude.
"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from hipdwc import ops                       # noqa: E402
from hipdwc import _lib as _lib_mod          # noqa: E402

DEV = "cuda:0"
PREFIX = {"fp32": "dwc_", "bf16": "dwc_bf16_"}
TOL = {("fp32", "y"): 2e-5, ("fp32", "dx"): 5e-5, ("fp32", "dw"): 5e-5, ("bf16", "y"): 6e-3, ("bf16", "dx"): 6e-3, ("bf16", "dw"): 3e-4}
EINVAL = -1
NEW_SYMBOLS = [p + n for p in PREFIX.values() for n in ("conv2d_bwd_weight_zeropad_ws_bytes", "conv2d_bwd_weight_zeropad",
                                                       "conv2d_bwd_data_crop_ws_bytes", "conv2d_bwd_data_crop")]
NEW_SYMBOLS += ["dwc_x3_conv2d_wgrad_zeropad", "dwc_h2_conv2d_wgrad_zeropad", "dwc_bf16_conv2d_wgrad_halo_zeropad",
                "dwc_x3_conv2d_s2_ws_zeropad", "dwc_h2_conv2d_s2_ws_zeropad", "dwc_bf16_conv2d_s2_halo_zeropad"]


# =====================================================================================================================================
# without a GPU
# =====================================================================================================================================
def test_new_symbols_in_header_binding_and_library():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dwcgan_hip.h")).read()
    lib = _lib_mod.load()
    for name in NEW_SYMBOLS:
        assert "batchnorm" not in name
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib_mod.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert lib.dwc_version() == 11 == _lib_mod.ABI_VERSION


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_new_entries_refuse_null_geometry_before_any_launch(prec):
    lib = _lib_mod.load()
    fn = lambda n: getattr(lib, PREFIX[prec] + "conv2d_" + n)
    assert fn("bwd_weight_zeropad")(None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None) == EINVAL
    assert fn("bwd_data_crop")(None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None) == EINVAL
    # a valid shape with NULL tensors is refused as well
    assert fn("bwd_weight_zeropad")(None, None, None, 1, 8, 8, 8, 8, 3, 3, 1, 1, 8, 8, None, 0, None) == EINVAL
    assert fn("bwd_data_crop")(None, None, None, 1, 8, 8, 8, 8, 3, 3, 1, 1, None, 0, None) == EINVAL
    assert fn("bwd_data_crop_ws_bytes")(0, 0, 0, 0, 0, 0, 0, 0, 0) == 0
    # stride 2 is the 4x4 pad-1 layer on an even image, as for the reflect data gradient
    assert fn("bwd_data_crop_ws_bytes")(1, 7, 8, 8, 8, 4, 4, 2, 1) == 0
    halo = [0] * 8 + [None, 0, None]
    if prec == "fp32":
        assert lib.dwc_x3_conv2d_wgrad_zeropad(None, None, None, *halo) == EINVAL
        assert lib.dwc_h2_conv2d_wgrad_zeropad(None, None, 0, None, None, 0, None, *halo) == EINVAL
        assert lib.dwc_x3_conv2d_wgrad_zeropad(None, None, None, 1, 8, 16, 64, 64, 3, 64, 64, None, 0, None) == EINVAL
        assert lib.dwc_x3_conv2d_s2_ws_zeropad(None, None, None, None, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None) == EINVAL
        assert lib.dwc_h2_conv2d_s2_ws_zeropad(None, None, 0, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None, 0, None, None) == EINVAL
        assert lib.dwc_x3_conv2d_s2_ws_zeropad(None, None, None, None, 1, 32, 32, 64, 64, 64, 0, None, 0, None, None) == EINVAL
    else:
        assert lib.dwc_bf16_conv2d_wgrad_halo_zeropad(None, None, None, *halo) == EINVAL
        assert lib.dwc_bf16_conv2d_wgrad_halo_zeropad(None, None, None, 1, 8, 16, 64, 128, 3, 64, 128, None, 0, None) == EINVAL
        assert lib.dwc_bf16_conv2d_s2_halo_zeropad(None, None, None, None, 0, 0, 0, 0, 0, 0, None) == EINVAL
        assert lib.dwc_bf16_conv2d_s2_halo_zeropad(None, None, None, None, 1, 32, 32, 64, 64, 0, None) == EINVAL


def test_pad_mode_other_than_reflect_or_zero_is_a_value_error():
    x, w = torch.zeros(1, 8, 4, 4), torch.zeros(8, 8, 3, 3)
    with pytest.raises(ValueError):
        ops.conv2d(x, w, None, 1, 1, pad_mode="replicate")
    with pytest.raises(ValueError):
        ops.conv2d_padded(x, w, None, 1, 1, pad_mode="circular")
    with pytest.raises(ValueError):
        ops.conv2d_heads(x, w, None, pad_mode="replicate")


def test_conv_block_zero_constructs_at_stride_2_and_replicate_still_raises(monkeypatch):
    """The first construction fails before the strided convolutions took the zero rule."""
    import networks.networks as nets
    blk = nets.Conv2dBlock(8, 8, 4, 2, 1, pad_type="zero")
    assert blk.pad_type == "zero" and blk.stride == 2
    with pytest.raises(NotImplementedError):
        nets.Conv2dBlock(8, 8, 4, 2, 1, pad_type="replicate")
    nets.Conv2dBlock(8, 8, 3, 1, 1, pad_type="replicate")
    monkeypatch.setattr(ops, "ZERO_PAD_HIP", 0)              # the A/B partner: F.pad at stride 1, nothing at stride 2
    nets.Conv2dBlock(8, 8, 3, 1, 1, pad_type="zero")
    with pytest.raises(NotImplementedError):
        nets.Conv2dBlock(8, 8, 4, 2, 1, pad_type="zero")


# =====================================================================================================================================
# helpers
# =====================================================================================================================================
def _rnd(prec):
    return (lambda t: t.to(torch.bfloat16).float()) if prec == "bf16" else (lambda t: t)


def _reference(prec, B, ci, co, H, W, k, s, p, seed, bias=False):
    """(x, w, b, gy, float64 y, dx, dw, db) of the zero-padded convolution; x, gy and (for the reference) w rounded for bf16."""
    rnd = _rnd(prec)
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(B, ci, H, W, generator=g))
    w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (ci * k * k) ** 0.5)
    b = torch.randn(co, generator=g) * 0.5 if bias else None
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gy = rnd(torch.randn(B, co, Ho, Wo, generator=g))
    xr = x.double().requires_grad_(True)
    wr = rnd(w).double().requires_grad_(True)
    br = None if b is None else b.double().requires_grad_(True)
    y = F.conv2d(xr, wr, br, stride=s, padding=p)
    (y * gy.double()).sum().backward()
    return x, w, b, gy, y.detach(), xr.grad, wr.grad, (None if br is None else br.grad)


def _check(tag, got, ref, tol, atol=0.0):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()          # (NaN -- an element the kernel left unwritten -- fails the comparison below)
    print("ZERO-PAD %s err/scale=%.3e tol=%.1e" % (tag, err / scale if scale else float("nan"), tol))
    assert scale > 0 and err <= tol * scale + atol, "%s: max err %.3e of scale, tolerance %.1e" % (tag, err / scale, tol)


def _cl(t, dt):
    return t.to(DEV).to(dt).contiguous(memory_format=torch.channels_last)


class _precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        ops.set_precision(self.prec)
        return ops.act_dtype()

    def __exit__(self, *exc):
        ops.set_precision("fp32")


def _scratch(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=DEV)


def _entry_forward(lib, prec, dt, x, w, geom):
    B, ci, co, H, W, k, s, p = geom
    xd = _cl(x, dt)
    wp = ops._prepped(w.to(DEV), "fwd", co, ci, 1, None, prec == "bf16")
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = ops.empty_cl(B, co, Ho, Wo, DEV, dt)
    y.fill_(float("nan"))
    fn = lambda n: ops._fn(lib, "conv2d_" + n, xd)
    nws = fn("fwd_ws_bytes")(B, H, W, ci, co, k, k, s, p)
    ws = _scratch(nws)
    _lib_mod.check(fn("fwd_zeropad")(xd.data_ptr(), wp.data_ptr(), None, y.data_ptr(), B, H, W, ci, co, k, k, s, p, 0,
                                     ws.data_ptr() if nws else None, nws, ops._stream()), "fwd_zeropad")
    return y


def _entry_wgrad(lib, prec, dt, x, gy, geom, alloc=None):
    B, ci, co, H, W, k, s, p = geom
    xd, gd = _cl(x, dt), _cl(gy, dt)
    fn = lambda n: ops._fn(lib, "conv2d_" + n, xd)
    nws = fn("bwd_weight_zeropad_ws_bytes")(B, H, W, ci, co, k, k, s, p)
    assert nws == fn("bwd_weight_ws_bytes")(B, H, W, ci, co, k, k, s, p) > 0
    if alloc is None:
        ws, dw = _scratch(nws), torch.full((co, ci, k, k), float("nan"), dtype=torch.float32, device=DEV)
    else:
        ws, dw = alloc.guarded((nws,), torch.uint8, DEV), alloc.guarded((co, ci, k, k), torch.float32, DEV)
    _lib_mod.check(fn("bwd_weight_zeropad")(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), B, H, W, ci, co, k, k, s, p, ci, co,
                                            ws.data_ptr(), nws, ops._stream()), "bwd_weight_zeropad")
    return dw


def _entry_dgrad(lib, prec, dt, w, gy, geom, alloc=None, want_split=None):
    B, ci, co, H, W, k, s, p = geom
    gd = _cl(gy, dt)
    wp = ops._prepped(w.to(DEV), "dgrad", co, ci, s, None, prec == "bf16")
    fn = lambda n: ops._fn(lib, "conv2d_" + n, gd)
    nws = fn("bwd_data_crop_ws_bytes")(B, H, W, ci, co, k, k, s, p)
    image = (B * (H + 2 * p) * (W + 2 * p) * ci * gd.element_size() + 255) // 256 * 256
    assert nws >= image
    if want_split is not None:
        assert (nws > image) == want_split, (geom, nws, image)
    if alloc is None:
        ws, dx = _scratch(nws), ops.empty_cl(B, ci, H, W, DEV, dt)
        dx.fill_(float("nan"))
    else:
        ws, dx = alloc.guarded((nws,), torch.uint8, DEV), alloc.guarded((B, ci, H, W), dt, DEV, channels_last=True)
    _lib_mod.check(fn("bwd_data_crop")(gd.data_ptr(), wp.data_ptr(), dx.data_ptr(), B, H, W, ci, co, k, k, s, p, ws.data_ptr(), nws,
                                       ops._stream()), "bwd_data_crop")
    if nws > 1:             # one byte less of scratch is refused before any launch
        assert fn("bwd_data_crop")(gd.data_ptr(), wp.data_ptr(), dx.data_ptr(), B, H, W, ci, co, k, k, s, p, ws.data_ptr(), nws - 1,
                                   ops._stream()) == -2
    return dx


# =====================================================================================================================================
# im2col entries
# =====================================================================================================================================
# (B, Cin, Cout, H, W, k, stride, pad), what is compared.  The gathered channel count is a power of two (Cin for y / dw, Cout for dx),
# the produced one a multiple of 8: 24 channels appear on the produced side only.
ENTRY_CASES = [
    ((1, 8, 16, 9, 7, 3, 1, 1), "y dw dx"),
    ((3, 16, 24, 9, 7, 3, 1, 1), "y dw"),
    ((3, 24, 8, 9, 7, 3, 1, 1), "dx"),
    ((3, 8, 8, 5, 5, 5, 1, 2), "y dw dx"),             # every pixel touches the border
    ((1, 16, 8, 8, 8, 7, 1, 3), "y dw dx"),
    ((3, 8, 16, 2, 2, 4, 2, 1), "y dw dx"),            # the style encoder's tail: every window has zero rows and columns
    ((1, 16, 8, 6, 10, 4, 2, 1), "y dw dx"),
    ((3, 8, 24, 6, 10, 4, 2, 1), "y dw"),
    ((3, 24, 16, 6, 10, 4, 2, 1), "dx"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ENTRY_CASES, ids=lambda c: "B%d-%dto%d-%dx%d-k%ds%dp%d" % c[0])
def test_im2col_zero_rule_entries(case, prec):
    geom, what = case
    B, ci, co, H, W, k, s, p = geom
    lib = _lib_mod.load()
    x, w, _, gy, y64, dx64, dw64, _ = _reference(prec, B, ci, co, H, W, k, s, p, seed=sum(geom))
    # the zero rule matters at this size: the reflect-padded result differs
    assert (F.conv2d(F.pad(x.double(), (p,) * 4, mode="reflect"), _rnd(prec)(w).double(), stride=s) - y64).abs().max() > 0.05 * y64.abs().max()
    tag = "%s %s" % (prec, geom)
    with _precision(prec) as dt:
        if "y" in what:
            _check(tag + " y", _entry_forward(lib, prec, dt, x, w, geom), y64, TOL[(prec, "y")])
        if "dw" in what:
            _check(tag + " dw", _entry_wgrad(lib, prec, dt, x, gy, geom), dw64, TOL[(prec, "dw")])
        if "dx" in what:
            _check(tag + " dx", _entry_dgrad(lib, prec, dt, w, gy, geom), dx64, TOL[(prec, "dx")])


# One shape per branch of dwc_conv2d_bwd_weight_plan: (B, Cin, Cout, H, W, k, s, p), branch
WGRAD_PLAN_CASES = [
    ((1, 8, 16, 9, 7, 3, 1, 1), "unsplit"),
    ((3, 16, 16, 32, 32, 3, 1, 1), "split"),           # 12 / 6 pixel ranges (fp32 / bf16), plain reduce
    ((2, 8, 8, 64, 64, 3, 1, 1), "wide"),              # 32 / 16 ranges of 576 elements: the wide reduce
    ((3, 8, 16, 48, 40, 4, 2, 1), "split"),            # stride 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", WGRAD_PLAN_CASES, ids=lambda c: "%s-k%ds%d" % (c[1], c[0][5], c[0][6]))
def test_weight_gradient_zero_rule_on_every_plan_branch(case, prec):
    geom, branch = case
    B, ci, co, H, W, k, s, p = geom
    lib = _lib_mod.load()
    bn, splits, chunk, wide = _lib_mod.plan(PREFIX[prec] + "conv2d_bwd_weight_plan", B, H, W, ci, co, k, k, s, p)
    assert {"unsplit": splits == 1 and not wide, "split": splits > 1 and not wide, "wide": splits >= 16 and wide == 1}[branch], \
        (geom, bn, splits, chunk, wide)
    x, w, _, gy, _, _, dw64, _ = _reference(prec, B, ci, co, H, W, k, s, p, seed=sum(geom) + 1)
    with _precision(prec) as dt:
        _check("%s %s %s dw" % (prec, geom, branch), _entry_wgrad(lib, prec, dt, x, gy, geom), dw64, TOL[(prec, "dw")])
        # native fp32 MFMA instantiation of the same rule (dwc_x3_gemm_mode bit 1 off)
        if prec == "fp32":
            old = lib.dwc_x3_gemm_mode(0)
            try:
                _check("fp32-native %s %s dw" % (geom, branch), _entry_wgrad(lib, prec, dt, x, gy, geom), dw64, TOL[(prec, "dw")])
            finally:
                lib.dwc_x3_gemm_mode(old)


# (B, Cin, Cout, H, W, k, s, p) per precision, split-K plan or not (the split plan reduces into the scratch image, a copy crops it)
CROP_PLAN_CASES = [
    ("unsplit-s1", {"fp32": (1, 8, 16, 9, 7, 3, 1, 1), "bf16": (1, 8, 16, 9, 7, 3, 1, 1)}, False),
    ("split-s1", {"fp32": (1, 8, 32, 8, 8, 3, 1, 1), "bf16": (1, 8, 64, 8, 8, 3, 1, 1)}, True),
    ("unsplit-s2", {"fp32": (3, 16, 8, 6, 10, 4, 2, 1), "bf16": (3, 16, 8, 6, 10, 4, 2, 1)}, False),
    ("split-s2", {"fp32": (1, 8, 256, 8, 8, 4, 2, 1), "bf16": (1, 8, 256, 8, 8, 4, 2, 1)}, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CROP_PLAN_CASES, ids=lambda c: c[0])
def test_guarded_output_and_scratch_of_the_new_entries(case, prec):
    """tests/guarded_alloc.py around dx / dw and the scratch of exactly *_ws_bytes, on a split and an unsplit plan of each entry:
    no byte outside is written, every element of the output is (NaN poison otherwise), and the values hold the entry tolerances.
    fp32 runs both the split-product and the native inner products."""
    import guarded_alloc
    name, geoms, split = case
    geom = geoms[prec]
    B, ci, co, H, W, k, s, p = geom
    lib = _lib_mod.load()
    alloc = guarded_alloc.GuardedAllocator()
    x, w, _, gy, _, dx64, dw64, _ = _reference(prec, B, ci, co, H, W, k, s, p, seed=sum(geom) + 2)
    with _precision(prec) as dt:
        for mode in ((None, 0) if prec == "fp32" else (None,)):
            old = lib.dwc_x3_gemm_mode(-1 if mode is None else mode)
            try:
                dx = _entry_dgrad(lib, prec, dt, w, gy, geom, alloc, want_split=split)
                alloc.verify()
                _check("%s %s dx mode %s" % (prec, name, mode), dx, dx64, TOL[(prec, "dx")])
                dw = _entry_wgrad(lib, prec, dt, x, gy, geom, alloc)
                alloc.verify()
                _check("%s %s dw mode %s" % (prec, name, mode), dw, dw64, TOL[(prec, "dw")])
            finally:
                lib.dwc_x3_gemm_mode(old)
        # the weight gradient on a split plan too (the wide-reduce shape), guarded
        wg = (2, 8, 8, 64, 64, 3, 1, 1)
        assert _lib_mod.plan(PREFIX[prec] + "conv2d_bwd_weight_plan", wg[0], wg[3], wg[4], wg[1], wg[2], 3, 3, 1, 1)[1] > 1
        if name == "unsplit-s1":
            x2, _, _, gy2, _, _, dw2, _ = _reference(prec, *wg, seed=5)
            dw = _entry_wgrad(lib, prec, dt, x2, gy2, wg, alloc)
            alloc.verify()
            _check("%s split dw guarded" % prec, dw, dw2, TOL[(prec, "dw")])


# =====================================================================================================================================
# halo weight-gradient kernels, called through the C ABI (ops.py's size rules would send shapes this small elsewhere)
# =====================================================================================================================================
# (B, Cin, Cout, H, W, K): the smallest shapes the *_ws_bytes queries accept.  One unit per image (all four borders in one tile),
# 2 x 2 units (every tile a corner), 3 x 3 units (edge tiles and an interior tile); K = 4 is the stride-2 layer (units of the
# H/2 x W/2 grid).  Cout 64: the two-halves form of the split-product kernel; bf16 K = 5 at Cout 64 needs Cin 128.
HALO_WGRAD_CASES = {
    "fp32": [(1, 64, 64, 8, 16, 3), (2, 64, 128, 16, 32, 3), (1, 64, 64, 24, 48, 3), (1, 64, 128, 8, 16, 5), (1, 64, 64, 24, 48, 5),
             (1, 64, 64, 8, 32, 4), (2, 64, 128, 16, 64, 4), (1, 64, 64, 24, 96, 4)],
    "bf16": [(1, 64, 128, 8, 16, 3), (2, 64, 128, 16, 32, 3), (1, 64, 128, 24, 48, 3), (1, 128, 64, 8, 16, 5), (1, 64, 128, 24, 48, 5),
             (1, 64, 128, 16, 32, 4), (2, 64, 128, 32, 64, 4), (1, 64, 128, 48, 96, 4)],
}


def _halo_wgrad_splits(lib, form, case):
    """Pixel ranges of the halo weight-gradient plan, from the scratch the query asks for: one [K*K*Cin][Cout] fp32 slab per range
    (two per range in the two-halves form of the split-product kernel, Cout not a multiple of 128)."""
    B, ci, co, H, W, K = case
    nws = (lib.dwc_bf16_conv2d_wgrad_halo_ws_bytes if form == "bf16" else lib.dwc_x3_conv2d_wgrad_ws_bytes)(B, H, W, ci, co, K)
    halves = 2 if form != "bf16" and co % 128 else 1
    return nws // (K * K * ci * co * 4 * halves)


@pytest.mark.parametrize("form", ["h2", "bf16"])
def test_halo_weight_gradient_cases_cover_split_and_unsplit_plans(form):
    """Host code only: the cases below hold an unsplit and a split plan of each halo weight-gradient entry, per filter size."""
    lib = _lib_mod.load()
    cases = HALO_WGRAD_CASES["bf16" if form == "bf16" else "fp32"]
    for K in (3, 5, 4):
        splits = [_halo_wgrad_splits(lib, form, c) for c in cases if c[5] == K]
        assert min(splits) == 1 and max(splits) > 1, (form, K, splits)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["h2", "x3", "bf16"])
@pytest.mark.parametrize("idx", range(8))
def test_halo_weight_gradient_zero_rule(form, idx):
    """dwc_h2_ / dwc_x3_conv2d_wgrad_zeropad and dwc_bf16_conv2d_wgrad_halo_zeropad against the float64 weight gradient of the
    zero-padded convolution, output and scratch between guards.  fp32 forms: 2e-6 of the largest reference magnitude and twice the
    fp32 CPU autograd's own error (+2e-7), as tests/test_h2_parity.py / test_x3_parity.py hold the reflect forms; bf16: 3e-4."""
    import guarded_alloc
    prec = "bf16" if form == "bf16" else "fp32"
    B, ci, co, H, W, K = HALO_WGRAD_CASES[prec][idx]
    s, p = (2, 1) if K == 4 else (1, K // 2)
    lib = _lib_mod.load()
    x, w, _, gy, _, _, dw64, _ = _reference(prec, B, ci, co, H, W, K, s, p, seed=B + ci + co + H + W + K)
    x32, w32 = x.clone().requires_grad_(True), _rnd(prec)(w).clone().requires_grad_(True)
    (F.conv2d(x32, w32, None, stride=s, padding=p) * gy).sum().backward()
    err32 = (w32.grad.double() - dw64).abs().max().item() / dw64.abs().max().item()
    # the rule matters: the reflect-padded layer has another weight gradient
    wr = w.double().requires_grad_(True)
    (F.conv2d(F.pad(x.double(), (p,) * 4, mode="reflect"), wr, stride=s) * gy.double()).sum().backward()
    assert (wr.grad - dw64).abs().max() > 1e-3 * dw64.abs().max()
    alloc = guarded_alloc.GuardedAllocator()
    with _precision(prec) as dt:
        xd, gd = _cl(x, dt), _cl(gy, dt)
        nws = (lib.dwc_bf16_conv2d_wgrad_halo_ws_bytes if form == "bf16" else lib.dwc_x3_conv2d_wgrad_ws_bytes)(B, H, W, ci, co, K)
        assert nws > 0, "shape left the halo weight-gradient kernel"
        print("ZERO-PAD %s halo wgrad %s: %d pixel range(s)" % (form, (B, ci, co, H, W, K), _halo_wgrad_splits(lib, form, (B, ci, co, H, W, K))))
        ws, dw = alloc.guarded((nws,), torch.uint8, DEV), alloc.guarded((co, ci, K, K), torch.float32, DEV)
        tail = (dw.data_ptr(), B, H, W, ci, co, K, ci, co, ws.data_ptr(), nws, ops._stream())
        if form == "bf16":
            rc = lib.dwc_bf16_conv2d_wgrad_halo_zeropad(xd.data_ptr(), gd.data_ptr(), *tail)
        elif form == "x3":
            rc = lib.dwc_x3_conv2d_wgrad_zeropad(xd.data_ptr(), gd.data_ptr(), *tail)
        else:
            xa, ga = ops.amax_of(xd), ops.amax_of(gd)
            rc = lib.dwc_h2_conv2d_wgrad_zeropad(xd.data_ptr(), xa[0], xa[1], gd.data_ptr(), ga[0], ga[1], *tail)
            # the slots the launch scaled by hold max|x| and max|g| bit for bit, before and after it
            assert _amax_bits(xd) == int(xd.abs().max().view(torch.int32)) and _amax_bits(gd) == int(gd.abs().max().view(torch.int32))
        _lib_mod.check(rc, form + " wgrad zeropad")
        alloc.verify()
    _check("%s halo wgrad %s (fp32 CPU autograd: %.2e)" % (form, (B, ci, co, H, W, K), err32), dw, dw64, 3e-4 if form == "bf16" else 2e-6)
    if form != "bf16":
        err = (dw.double().cpu() - dw64).abs().max().item() / dw64.abs().max().item()
        assert err <= 2 * err32 + 2e-7, (err, err32)


# =====================================================================================================================================
# stride-2 halo forward, called through the C ABI
# =====================================================================================================================================
# (B, Cin, Cout, H, W): tiles of 32 x 32 input pixels (16 x 16 outputs).  One tile per image (all four borders in one tile), 2 x 2
# (even count per side: every tile a corner), 3 x 3 and 3 x 2 (odd count: edge tiles and an interior tile), Cout of two column tiles,
# and for the split-product forms the contraction-split plan (dwc_x3_conv2d_ksplit_ws_bytes non-zero).
S2_FWD_CASES = [(1, 64, 64, 32, 32), (2, 64, 64, 64, 64), (1, 64, 64, 96, 96), (1, 64, 128, 96, 64), (8, 256, 64, 32, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["h2", "x3", "bf16"])
@pytest.mark.parametrize("shape", S2_FWD_CASES, ids=lambda s: "B%d-%dto%d-%dx%d" % s)
def test_stride2_halo_forward_zero_rule(shape, form):
    """dwc_h2_ / dwc_x3_conv2d_s2_ws_zeropad and dwc_bf16_conv2d_s2_halo_zeropad (bias + lrelu epilogue) against the float64 zero-padded
    4x4 stride-2 convolution, y between guards and poisoned.  fp32 forms: 5e-6 of the largest reference magnitude, as
    tests/test_h2_parity.py / test_x3_parity.py hold the reflect forms; bf16: 6e-3.  The two-plane form raises y's absmax slot to
    max|y| bit for bit."""
    import guarded_alloc
    prec = "bf16" if form == "bf16" else "fp32"
    B, ci, co, H, W = shape
    lib = _lib_mod.load()
    x, w, b, _, y64, _, _, _ = _reference(prec, B, ci, co, H, W, 4, 2, 1, seed=sum(shape), bias=True)
    y64 = F.leaky_relu(y64, 0.1)
    yr = F.leaky_relu(F.conv2d(F.pad(x.double(), (1,) * 4, mode="reflect"), _rnd(prec)(w).double(), b.double(), stride=2), 0.1)
    assert (yr - y64).abs().max() > 0.05 * y64.abs().max()            # the rule matters
    alloc = guarded_alloc.GuardedAllocator()
    with _precision(prec) as dt:
        xd, wd, bd = _cl(x, dt), w.to(DEV), b.to(DEV)
        y = alloc.guarded((B, co, H // 2, W // 2), dt, DEV, channels_last=True)
        act, st = ops.ACT["lrelu"], ops._stream()
        if form == "bf16":
            assert lib.dwc_bf16_conv2d_s2_halo_ok(B, H, W, ci, co)
            wp = ops._prepped(wd, "fwd", co, ci, 2, None, True)
            rc = lib.dwc_bf16_conv2d_s2_halo_zeropad(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W, ci, co, act, st)
        else:
            assert lib.dwc_x3_conv2d_s2_ok(B, H, W, ci, co)
            need = lib.dwc_x3_conv2d_ksplit_ws_bytes(B, H, W, ci, co, 4, 2)
            assert need > 0 or B != 8, "the last case left the contraction-split plan"
            print("ZERO-PAD %s s2 forward %s: contraction split scratch %d bytes" % (form, shape, need))
            _, _, tickets = ops._x3_ksplit(lib, xd.device, B, H, W, ci, co, 4, 2)
            ws = alloc.guarded((max(int(need), 1),), torch.uint8, DEV)
            if form == "x3":
                wp = ops._prepped(wd, "x3_fwd", co, ci, 1, None)
                rc = lib.dwc_x3_conv2d_s2_ws_zeropad(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W, ci, co, co, act,
                                                     ws.data_ptr() if need else None, need, tickets, st)
            else:
                wp = ops._prepped(wd, "h2_fwd", co, ci, 1, None)
                xa = ops.amax_of(xd)
                ya, yep = ops.amax_slot(xd.device)
                rc = lib.dwc_h2_conv2d_s2_ws_zeropad(xd.data_ptr(), xa[0], xa[1], wp.data_ptr(), bd.data_ptr(), y.data_ptr(), ya, yep, B, H, W,
                                                     ci, co, co, act, ws.data_ptr() if need else None, need, tickets, st)
        _lib_mod.check(rc, form + " s2 forward zeropad")
        alloc.verify()
        if form == "h2":
            ops.set_amax(y, ya, yep)
            assert _amax_bits(y) == int(y.abs().max().view(torch.int32))
    _check("%s s2 halo forward %s" % (form, shape), y, y64, 6e-3 if form == "bf16" else 5e-6)


# =====================================================================================================================================
# ops.conv2d(pad_mode='zero') on the halo kernels that take the rule
# =====================================================================================================================================
class _routes:
    """Collects the launch kinds (first word of each span's detail) of the ops calls made inside."""

    def __enter__(self):
        self.old, ops.TIMER = ops.TIMER, ops.KernelTimer()
        self.timer = ops.TIMER
        return self

    def __exit__(self, *exc):
        ops.TIMER = self.old

    def kinds(self):
        return [d.split()[0] for d in self.timer.details if d]


# (B, C, H, W, k): one tile per image, 2 x 2 tiles (every tile a corner), an edge tile and an interior tile (3 x 3), and the
# contraction-split plan of the split-product kernel (dwc_x3_conv2d_ksplit_ws_bytes non-zero; bf16: the halo weight gradient)
HALO_S1_CASES = [(2, 64, 16, 16, 3), (1, 64, 32, 32, 3), (1, 64, 16, 16, 5), (1, 64, 48, 48, 3), (2, 256, 16, 16, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", HALO_S1_CASES, ids=lambda s: "B%d-C%d-%dx%d-k%d" % s)
def test_stride1_halo_routes_under_zero(shape, prec):
    """Forward and data gradient on the halo kernels with reflect = 0 (the residual-gradient token rides on the data gradient's
    epilogue), weight gradient on the halo kernel's zero-rule form (fp32 two-plane; bf16 where Cout % 128 == 0, else the im2col
    zero-rule entry); the absmax slot of y equals max|y| bit for bit (two-plane forward)."""
    B, C, H, W, k = shape
    p = k // 2
    lib = _lib_mod.load()
    x, w, b, gy, y64, dx64, dw64, db64 = _reference(prec, B, C, C, H, W, k, 1, p, seed=sum(shape), bias=True)
    g = torch.Generator().manual_seed(9)
    g_res = _rnd(prec)(torch.randn(B, C, H, W, generator=g))
    with _precision(prec) as dt:
        half = prec == "bf16"
        ok = lib.dwc_bf16_conv2d_same_halo_ok(B, H, W, C, C, k) if half else lib.dwc_x3_conv2d_same_ok(B, H, W, C, C, k)
        assert ok, "shape left the halo kernels"
        if C == 256 and not half:
            assert lib.dwc_x3_conv2d_ksplit_ws_bytes(B, H, W, C, C, k, 1) > 0, "shape left the contraction-split plan"
        xd = _cl(x, dt).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        token = ops.ResGradToken()
        with _routes() as r:
            y = ops.conv2d(xd, wd, bd, 1, p, "none", token=token, pad_mode="zero")
            if not half:                  # the two-plane forward raised y's slot to max|y|, bit for bit
                assert _amax_bits(y) == int(y.detach().abs().max().view(torch.int32))
            token.g = _cl(g_res, dt)
            (y.float() * gy.to(DEV)).sum().backward()
            kinds = r.kinds()
        assert kinds[0] == ("fwd-halo" if half else "fwd-h2"), kinds
        assert ("dgrad-halo" if half else "dgrad-h2") in kinds and not any("ring" in q for q in kinds), kinds
        # (fp32: the halo weight gradient under the zero rule; bf16: the same where Cout % 128 == 0, else the im2col entry)
        bf16_halo = half and lib.dwc_bf16_conv2d_wgrad_halo_ws_bytes(B, H, W, C, C, k) > 0
        assert bf16_halo == (half and C == 256)
        assert [q for q in kinds if q.startswith("wgrad")] == ([("wgrad-halo" if bf16_halo else "wgrad")] if half else ["wgrad-h2"]), kinds
        ty, tdx = (6e-3, 6e-3) if half else (5e-6, 2e-6)
        _check("%s halo y %s" % (prec, shape), y, y64, ty)
        _check("%s halo dx+res %s" % (prec, shape), xd.grad, dx64 + g_res.double(), tdx if not half else 6e-3)
        _check("%s halo dw %s" % (prec, shape), wd.grad, dw64, TOL[(prec, "dw")])
        _check("%s halo db %s" % (prec, shape), bd.grad, db64, TOL[(prec, "dw")])


def _amax_bits(t):
    """(epoch, magnitude bits) of the absmax slot attached to ``t`` (ops.amax_slot: epoch << 32 | fp32 bit pattern)."""
    c = ops.amax_live(t)
    assert c is not None, "no live absmax slot on the tensor"
    pool = ops._AMAX[t.device.index if t.device.index is not None else torch.cuda.current_device()][0]
    word = int(pool[(c[0] - pool.data_ptr()) // 8])
    assert (word >> 32) == c[1], "slot epoch %d, tag says %d" % (word >> 32, c[1])
    return word & 0xffffffff


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 64, 64, 32, 32), (2, 64, 128, 64, 32), (1, 64, 64, 64, 64), (1, 64, 64, 96, 96)],
                         ids=lambda s: "B%d-%dto%d-%dx%d" % s)
def test_stride2_routes_under_zero(shape, prec, monkeypatch):
    """4x4 stride-2 pad-1 under the zero rule at shapes the halo data gradient takes: the data gradient as the four parity classes of
    the halo kernel with no ring behind them, forward on the bf16 halo kernel (fp32 this small: the size rule keeps it on the im2col
    zero-rule GEMM; test_stride2_halo_forward_zero_rule calls the fp32 halo forms), the weight gradient by the size rules.
    One tile of 32 x 32 input pixels, 2 x 1, 2 x 2 (every tile a corner) and 3 x 3 (edge tiles and an interior tile)."""
    B, ci, co, H, W = shape
    monkeypatch.setattr(ops, "S2DGRAD_MIN_WGS", 0)       # the size rule keeps shapes this small on the im2col GEMM
    x, w, b, gy, y64, dx64, dw64, db64 = _reference(prec, B, ci, co, H, W, 4, 2, 1, seed=sum(shape), bias=True)
    with _precision(prec) as dt:
        half = prec == "bf16"
        xd = _cl(x, dt).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with _routes() as r:
            y = ops.conv2d(xd, wd, bd, 2, 1, "none", pad_mode="zero")
            (y.float() * gy.to(DEV)).sum().backward()
            kinds = r.kinds()
        assert kinds[0] == ("fwd-s2halo" if half else "fwd-g3"), kinds
        assert ("dgrad-s2halo" if half else "dgrad-h2s2") in kinds and not any("ring" in q for q in kinds), kinds
        _check("%s s2 y %s" % (prec, shape), y, y64, TOL[(prec, "y")])
        _check("%s s2 dx %s" % (prec, shape), xd.grad, dx64, 6e-3 if half else 2e-6)
        _check("%s s2 dw %s" % (prec, shape), wd.grad, dw64, TOL[(prec, "dw")])
        _check("%s s2 db %s" % (prec, shape), bd.grad, db64, TOL[(prec, "dw")])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 16), (1, 48, 40)], ids=lambda s: "B%d-%dx%d" % s)
def test_stem_forward_route_under_zero(shape, prec):
    """The 7x7 stem (image planes -> 64, pad 3) under zero: forward on the stem kernels with reflect = 0 (fp32: y's absmax slot equals
    max|y| bit for bit), weight and bias gradients on the im2col zero-rule entry.  y: fp32 2e-5 / bf16 6e-3, dw: 5e-5 / 3e-4."""
    B, H, W = shape
    lib = _lib_mod.load()
    with _precision(prec) as dt:
        half = prec == "bf16"
        P = ops.image_planes(dt)
        x, w, b, gy, y64, _, dw64, db64 = _reference(prec, B, P, 64, H, W, 7, 1, 3, seed=sum(shape) + P, bias=True)
        y64 = F.leaky_relu(y64, 0.1)
        yr = F.leaky_relu(F.conv2d(F.pad(x.double(), (3,) * 4, mode="reflect"), _rnd(prec)(w).double(), b.double()), 0.1)
        assert (yr - y64).abs().max() > 0.05 * y64.abs().max()            # the rule matters
        assert (lib.dwc_bf16_conv2d_stem_ok if half else lib.dwc_x3_conv2d_stem_ok)(B, H, W, H, W, 7, ops.ACT["lrelu"])
        xd = _cl(x, dt)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with _routes() as r:
            y = ops.conv2d(xd, wd, bd, 1, 3, "lrelu", pad_mode="zero")
            kinds = r.kinds()
        assert kinds == ["fwd-stem" if half else "fwd-stem-x3"], kinds
        if not half:
            assert _amax_bits(y) == int(y.detach().abs().max().view(torch.int32))
        _check("%s stem y %s" % (prec, shape), y, y64, TOL[(prec, "y")])
    # gradients of the linear layer (no activation): the im2col zero-rule weight gradient
    with _precision(prec) as dt:
        x, w, b, gy, _, _, dw64, db64 = _reference(prec, B, P, 64, H, W, 7, 1, 3, seed=sum(shape) + P, bias=True)
        xd = _cl(x, dt)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with _routes() as r:
            y = ops.conv2d(xd, wd, bd, 1, 3, "none", pad_mode="zero")
            (y.float() * gy.to(DEV)).sum().backward()
            kinds = r.kinds()
        assert kinds[0] == ("fwd-stem" if half else "fwd-stem-x3") and kinds[1] in ("wgrad", "wgrad-g3"), kinds
        _check("%s stem dw %s" % (prec, shape), wd.grad, dw64, TOL[(prec, "dw")])
        _check("%s stem db %s" % (prec, shape), bd.grad, db64, TOL[(prec, "dw")])


@pytest.mark.gpu
def test_absmax_slots_of_y_and_g_under_zero(monkeypatch):
    """fp32 two-plane route under zero with an activation: after the forward y's slot, and after the backward the slot of g (the
    gradient behind the activation, which the halo weight- and data-gradient launches scale by) equal max|.| bit for bit."""
    B, C, H, W, k = 2, 64, 16, 16, 3
    x, w, b, gy, _, _, _, _ = _reference("fp32", B, C, C, H, W, k, 1, 1, seed=77, bias=True)
    asked = []
    real = ops.amax_of

    def spy(t):
        out = real(t)
        asked.append(t)
        return out
    monkeypatch.setattr(ops, "amax_of", spy)
    with _precision("fp32") as dt:
        xd = _cl(x, dt).requires_grad_(True)
        wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        with _routes() as r:
            y = ops.conv2d(xd, wd, bd, 1, 1, "lrelu", pad_mode="zero")
            assert _amax_bits(y) == int(y.detach().abs().max().view(torch.int32))
            del asked[:]
            (y * gy.to(DEV)).sum().backward()
            kinds = r.kinds()
        assert kinds == ["fwd-h2", "wgrad-h2", "dgrad-h2"], kinds
        gs = [t for t in asked if t.data_ptr() != xd.data_ptr()]
        assert len(gs) == 2 and gs[0].data_ptr() == gs[1].data_ptr() and tuple(gs[0].shape) == (B, C, H, W), [tuple(t.shape) for t in asked]
        g = gs[0]
        want = gy.to(DEV) * torch.where(y.detach() > 0, 1.0, 0.1)
        assert torch.allclose(g, want, rtol=1e-6, atol=0.0)                   # g = dy * lrelu'(y)
        assert _amax_bits(g) == int(g.abs().max().view(torch.int32))


# =====================================================================================================================================
# modules
# =====================================================================================================================================
def _forbid_4d_pad(monkeypatch):
    real_pad = torch.nn.functional.pad

    def pad(t, *a, **k):
        if t.dim() == 4:
            raise AssertionError("torch.nn.functional.pad on a 4-D tensor: the zero rule is not inside the kernel")
        return real_pad(t, *a, **k)            # (1-D: a bias padded to the aligned channel count)
    monkeypatch.setattr(torch.nn.functional, "pad", pad)
    return real_pad


def _norm64(kind, y, gamma, beta, eps=1e-5):
    from oracle import dwcgan_oracle as orc
    if kind == "in":
        return orc.instance_norm(y)
    if kind == "ln":
        return orc.layer_norm_munit(y, gamma, beta)
    if kind == "bn":                                        # nn.BatchNorm2d in training mode: biased batch variance
        mu = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y - mu) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        return (y - mu) / torch.sqrt(var + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return y


BLOCK_GEOMS = [(2, 8, 16, 9, 7, 3, 1, 1), (2, 8, 8, 7, 9, 5, 1, 2), (3, 8, 16, 6, 10, 4, 2, 1), (1, 8, 8, 9, 8, 7, 1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["none", "in", "ln", "bn", "sn"])
@pytest.mark.parametrize("geom", BLOCK_GEOMS, ids=lambda g: "k%ds%d" % (g[5], g[6]))
def test_conv_block_zero_vs_float64(geom, norm, monkeypatch):
    """Conv2dBlock(pad_type='zero', activation='lrelu') forward / dx / dw / db (and the norm's parameters) against the float64
    zero-padded convolution composed with the oracle's norm expressions; no 4-D F.pad during the call."""
    import networks.networks as nets
    from oracle import dwcgan_oracle as orc
    B, ci, co, H, W, k, s, p = geom
    g = torch.Generator().manual_seed(sum(geom) + len(norm))
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (ci * k * k) ** 0.5)
    b = torch.randn(co, generator=g) * 0.5
    gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gy = torch.randn(B, co, Ho, Wo, generator=g)
    u0 = torch.randn(co, generator=g)
    u0 = u0 / u0.norm()

    # float64 reference
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    gr, betar = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    weff = wr
    if norm == "sn":                                       # one power iteration from u0, sigma = u . W v with u, v constants
        wm = wr.detach().reshape(co, -1)
        v = wm.t().mv(u0.double())
        v = v / (v.norm() + 1e-12)
        u = wm.mv(v)
        u = u / (u.norm() + 1e-12)
        weff = wr / torch.dot(u, wr.reshape(co, -1).mv(v))
    yr = orc.activation(_norm64(norm, F.conv2d(xr, weff, br, stride=s, padding=p), gr, betar), "lrelu")
    (yr * gy.double()).sum().backward()

    blk = nets.Conv2dBlock(ci, co, k, s, p, norm=norm, activation="lrelu", pad_type="zero").to(DEV)
    conv = blk.conv.module if norm == "sn" else blk.conv
    with torch.no_grad():
        (conv.weight_bar if norm == "sn" else conv.weight).copy_(w)
        conv.bias.copy_(b)
        if norm == "sn":
            conv.weight_u.copy_(u0)
        if norm == "ln":
            blk.norm.gamma.copy_(gamma)
            blk.norm.beta.copy_(beta)
        if norm == "bn":
            blk.norm.weight.copy_(gamma)
            blk.norm.bias.copy_(beta)
    xd = x.to(DEV).requires_grad_(True)
    _forbid_4d_pad(monkeypatch)
    import guarded_alloc
    alloc = guarded_alloc.GuardedAllocator()           # scratch and channels-last outputs of the ops between guards
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    y = blk(xd)
    (y * gy.to(DEV)).sum().backward()
    monkeypatch.undo()
    alloc.verify()
    tag = "block %s %s" % (norm, geom)
    _check(tag + " y", y, yr.detach(), 5e-5, 2e-6)
    _check(tag + " dx", xd.grad, xr.grad, 3e-4, 2e-6)
    _check(tag + " dw", (conv.weight_bar if norm == "sn" else conv.weight).grad, wr.grad, 3e-4, 2e-6)
    if norm in ("none", "ln", "sn"):
        _check(tag + " db", conv.bias.grad, br.grad, 3e-4, 2e-6)
    else:                                                  # the mean subtraction removes the bias: no gradient, or exact zeros
        assert conv.bias.grad is None or not conv.bias.grad.any()
    if norm == "ln":
        _check(tag + " dgamma", blk.norm.gamma.grad, gr.grad, 3e-4, 2e-6)
        _check(tag + " dbeta", blk.norm.beta.grad, betar.grad, 3e-4, 2e-6)
    if norm == "bn":
        _check(tag + " dgamma", blk.norm.weight.grad, gr.grad, 3e-4, 2e-6)
        _check(tag + " dbeta", blk.norm.bias.grad, betar.grad, 3e-4, 2e-6)


@pytest.mark.gpu
def test_zero_pad_hip_0_is_the_f_pad_route(monkeypatch):
    """ops.ZERO_PAD_HIP = 0 (the A/B partner) pads on the device and gives the same block output."""
    import networks.networks as nets
    torch.manual_seed(3)
    blk = nets.Conv2dBlock(8, 16, 3, 1, 1, norm="none", activation="relu", pad_type="zero").to(DEV)
    x = torch.randn(2, 8, 9, 7, device=DEV)
    with torch.no_grad():
        y1 = blk(x)
        monkeypatch.setattr(ops, "ZERO_PAD_HIP", 0)
        calls = []
        real_pad = torch.nn.functional.pad
        monkeypatch.setattr(torch.nn.functional, "pad", lambda t, *a, **k: (calls.append(t.dim()), real_pad(t, *a, **k))[1])
        y0 = blk(x)
    assert 4 in calls
    _check("ZERO_PAD_HIP 0 against 1", y1, y0.double().cpu(), 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_heads_under_zero(prec, monkeypatch):
    """Decoder.forward_nhwc4 with pad_type='zero': planes 0-2 tanh, plane 3 sigmoid of the float64 zero-padded 7x7 convolutions, and
    the gradients of both heads and of the feature map (tolerances of the im2col entries, the bf16 dx / dw behind an activation
    1.5e-2 / 1e-2 as in tests/test_bf16_parity.py)."""
    import networks.networks as nets
    B, C, H, W = 2, 16, 16, 16
    g = torch.Generator().manual_seed(21)
    rnd = _rnd(prec)
    feat = rnd(torch.randn(B, C, H, W, generator=g))
    wc, wa = torch.randn(3, C, 7, 7, generator=g) * 0.03, torch.randn(1, C, 7, 7, generator=g) * 0.03
    bc, ba = torch.randn(3, generator=g) * 0.1, torch.randn(1, generator=g) * 0.1
    gy = rnd(torch.randn(B, 4, H, W, generator=g))
    fr = feat.double().requires_grad_(True)
    wcr, war = rnd(wc).double().requires_grad_(True), rnd(wa).double().requires_grad_(True)
    yr = torch.cat([torch.tanh(F.conv2d(fr, wcr, bc.double(), padding=3)), torch.sigmoid(F.conv2d(fr, war, ba.double(), padding=3))], 1)
    (yr * gy.double()).sum().backward()
    with _precision(prec) as dt:
        half = prec == "bf16"
        dec = nets.Decoder(0, 0, C, 3, pad_type="zero", use_attention=True).to(DEV)
        with torch.no_grad():
            dec.image_content.conv.weight.copy_(wc)
            dec.image_content.conv.bias.copy_(bc)
            dec.image_attention.conv.weight.copy_(wa)
            dec.image_attention.conv.bias.copy_(ba)
        fd = _cl(feat, dt).requires_grad_(True)
        _forbid_4d_pad(monkeypatch)
        heads = dec.forward_nhwc4(fd)
        (heads[:, :4].float() * gy.to(DEV)).sum().backward()
        monkeypatch.undo()
        _check("%s heads y" % prec, heads[:, :4], yr.detach(), TOL[(prec, "y")])
        _check("%s heads dfeat" % prec, fd.grad, fr.grad, 1.5e-2 if half else 3e-4)
        _check("%s heads dw content" % prec, dec.image_content.conv.weight.grad, wcr.grad, 1e-2 if half else 3e-4)
        _check("%s heads dw attention" % prec, dec.image_attention.conv.weight.grad, war.grad, 1e-2 if half else 3e-4)


@pytest.mark.gpu
def test_res_block_grouped_equals_concatenated_under_zero(monkeypatch):
    """ResBlock._forward_groups takes 'zero' as it takes 'reflect': the first convolution runs once at batch B.  Shape, data and bounds
    of tests/test_lrelu_fused.py::test_res_block_lrelu_grouped_equals_concatenated: y 2e-6, gradients 2e-5 of the tensor's largest
    magnitude (+1e-6)."""
    import networks.networks as nets
    torch.manual_seed(11)
    B, C, H = 2, 16, 12
    blk = nets.ResBlock(dim=C, norm="adain", activation="lrelu", pad_type="zero").to(DEV)
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn(B, C, H, H, generator=g)
    params = [(torch.randn(3 * B * C, generator=g) * 0.5 + 1, torch.randn(3 * B * C, generator=g)) for _ in range(2)]
    gy = torch.randn(3 * B, C, H, H, generator=g).to(DEV)
    calls = []
    real_conv = ops.conv2d

    def spy(x, *a, **k):
        calls.append((x.shape[0], k.get("pad_mode")))
        return real_conv(x, *a, **k)
    monkeypatch.setattr(ops, "conv2d", spy)
    _forbid_4d_pad(monkeypatch)
    dev = lambda t: t.detach().clone().to(DEV).requires_grad_(True)
    outs = []
    for grouped in (True, False):
        del calls[:]
        blk.zero_grad(set_to_none=True)
        x = dev(x0)
        leaves = []
        for m, (wt, bs) in zip((blk.model[0].norm, blk.model[1].norm), params):
            m.weight, m.bias = dev(wt), dev(bs)
            leaves += [m.weight, m.bias]
        y = blk(x, groups=3) if grouped else blk(torch.cat([x] * 3))
        (y * gy).sum().backward()
        assert calls == [(B if grouped else 3 * B, "zero"), (3 * B, "zero")], calls
        outs.append([y.detach(), x.grad.detach(), blk.model[0].conv.weight.grad.detach().clone(),
                     blk.model[1].conv.weight.grad.detach().clone()] + [t.grad.detach() for t in leaves])
    names = ("y", "dx", "dw (first conv)", "dw (second conv)", "dgamma0", "dbeta0", "dgamma1", "dbeta1")
    for a, b, name in zip(outs[0], outs[1], names):
        _check("grouped vs concatenated: " + name, a, b.double().cpu(), 2e-6 if name == "y" else 2e-5, 1e-6)
