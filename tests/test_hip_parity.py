"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and against the
vectors recorded from the reference.  Run on the MI355X box with ``pytest -m gpu``.

Tolerances (fp32 end to end): single ops are compared on the tensor's own scale,
max|hip - ref| <= 2e-5 * max|ref| (+1e-6); whole-network gradients at kaiming init 5e-3 of scale
(a handful of ReLU/IN near-ties flip between any two implementations, the CPU oracle vs the
CPU reference show the same spread); scalar losses 2e-4 relative.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hipdwc import host, ops, synth          # noqa: E402
from oracle import dwcgan_oracle as orc      # noqa: E402

T = torch.from_numpy
DEV = "cuda:0"


from hipdwc import _lib as _lib_mod  # noqa: E402


def close(a, b, rel=2e-5, atol=1e-6, msg=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs().max().item()
    lim = rel * b.abs().max().item() + atol
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


def dev(t, grad=False):
    return t.detach().clone().to(DEV).requires_grad_(grad)


# (B, Cin, Cout, H, k, stride, pad, act)
CONV_SHAPES = [
    (2, 4, 64, 32, 7, 1, 3, "relu"),        # stem on an NHWC4 image (dx through the 8-pixels-wide image dgrad)
    (1, 4, 64, 21, 7, 1, 3, "none"),        # same, odd size: padded width 27 -> pitch 32
    (3, 4, 32, 16, 5, 1, 2, "lrelu"),       # same, 5x5 / 32 gathered channels
    (2, 64, 128, 32, 4, 2, 1, "relu"),      # downsample
    (2, 128, 256, 64, 4, 2, 1, "lrelu"),    # downsample, several blocks per image (split-product forward, stride-2 form)
    (2, 256, 256, 16, 3, 1, 1, "none"),     # ResBlock conv (below the halo kernel's 16x16 block: im2col kernels + ring strips)
    (3, 64, 128, 12, 3, 1, 1, "relu"),      # rectangular channel counts, non power-of-two size
    (2, 64, 64, 10, 3, 1, 1, "none"),       # size not a multiple of 4: F(2x2,3x3)
    (1, 256, 128, 16, 5, 1, 2, "none"),     # upsample-block conv
    (2, 128, 64, 24, 5, 1, 2, "none"),      # BN=64 path, non power-of-two spatial size
    (2, 64, 4, 32, 7, 1, 3, "heads"),       # fused tanh/sigmoid heads, BN=32 path
    (3, 4, 64, 16, 4, 2, 1, "lrelu"),       # D stem
    (3, 512, 512, 2, 4, 2, 1, "lrelu"),     # D tail on a 2x2 map (reflect pad on tiny maps)
    (3, 512, 8, 4, 4, 1, 0, "none"),        # cls head: 'valid' full-extent conv
    (3, 512, 4, 4, 1, 1, 0, "none"),        # src head 1x1 (Cout 1 padded to 4)
    (5, 64, 256, 1, 1, 1, 0, "relu"),       # Linear as 1x1 conv, M = 5 rows
    (2, 8, 16, 12, 3, 1, 1, "sigmoid"),     # small channel counts (tiny config)
    (1, 16, 32, 6, 4, 2, 1, "tanh"),
]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_forward_backward(shape):
    B, ci, co, H, k, s, p, act = shape
    g = torch.Generator().manual_seed(sum(v for v in shape if isinstance(v, int)))
    x = torch.randn(B, ci, H, H, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (ci * k * k) ** 0.5)
    b = torch.randn(co, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    if act == "heads":
        pre = orc.conv_block(xr, wr, br, s, p)
        yr = torch.cat([torch.tanh(pre[:, :3]), torch.sigmoid(pre[:, 3:4])], 1)
    else:
        yr = orc.conv_block(xr, wr, br, s, p, act=act)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, wd, bd = dev(x, True), dev(w, True), dev(b, True)
    yd = ops.conv2d(xd, wd, bd, s, p, act)
    close(yd, yr, msg="y")
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=5e-5, msg="dx")
    close(wd.grad, wr.grad, rel=5e-5, msg="dw")
    close(bd.grad, br.grad, rel=5e-5, msg="db")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,ci,co,H,W", [(3, 64, 128, 32, 32), (2, 128, 256, 64, 32), (1, 64, 64, 32, 96), (2, 256, 512, 32, 32)])
def test_stride2_data_gradient_halo_form(B, ci, co, H, W, prec, monkeypatch):
    """Data gradient of the 4x4 stride-2 reflect-pad-1 layers (reference networks.py:90,94,437, networks_v2.py:107-111) in halo
    form (r04): interior as four output-parity classes of 2x2-tap convolutions over dY (split products in fp32, bf16 MFMA on the
    bf16 path), border ring of the padded image as eight GEMM strips + band fold -- since r06 inside the same launch (pre-summed patch
    rows / columns, virtual block rows; DWC_RING_FUSED=0 brings the strips back).  Against the float64 gradient of the
    reflect-padded convolution -- every pixel, with the image border (where the ring folds) checked separately --, for square
    and rectangular images, one and several tiles per image."""
    monkeypatch.setattr(ops, "S2DGRAD_MIN_WGS", 0)
    g = torch.Generator().manual_seed(B + ci + co + H + W)
    rnd = (lambda t: t.to(torch.bfloat16).float()) if prec == "bf16" else (lambda t: t)
    x = rnd(torch.randn(B, ci, H, W, generator=g))
    w = rnd(torch.randn(co, ci, 4, 4, generator=g) * (1.0 / (ci * 16) ** 0.5))
    gy = rnd(torch.randn(B, co, H // 2, W // 2, generator=g))
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.conv2d(torch.nn.functional.pad(xr, (1, 1, 1, 1), mode="reflect"), w.double(), None, stride=2)
    (yr * gy.double()).sum().backward()
    ops.set_precision(prec)
    try:
        calls = []
        lib = _lib_mod.load()
        name = "dwc_bf16_conv2d_s2_halo_bwd_data" if prec == "bf16" else (
            "dwc_h2_conv2d_s2_bwd_data" if ops.X3_PLANES == 2 else "dwc_x3_conv2d_s2_bwd_data")
        if ops.RING_FUSED and (prec == "bf16" or ops.X3_PLANES == 2):
            name += "_fused"          # (r06: the border ring inside the same launch, tests/test_ring_fused.py)
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a: (calls.append(1), real(*a))[1])
        xd = x.to(DEV).to(ops.act_dtype()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wd = w.to(DEV).requires_grad_(True)
        yd = ops.conv2d(xd, wd, None, 2, 1, "none")
        (yd.float() * gy.to(DEV)).sum().backward()
        assert calls, "the halo-form data gradient was not taken"
        ref = xr.grad.float()
        got = xd.grad.float().cpu()
        scale = ref.abs().max().item()
        tol = 2e-5 if prec == "fp32" else 8e-3
        err = (got - ref).abs()
        assert err.max().item() <= tol * scale, ("all pixels", err.max().item() / scale)
        border = torch.zeros(H, W, dtype=torch.bool)
        border[[0, 1, 2, H - 3, H - 2, H - 1], :] = True
        border[:, [0, 1, 2, W - 3, W - 2, W - 1]] = True
        assert err[:, :, border].max().item() <= tol * scale, ("border band", err[:, :, border].max().item() / scale)
        # the same gradient through the im2col path
        monkeypatch.setattr(ops, "S2DGRAD", 0)
        xd2 = xd.detach().clone().requires_grad_(True)
        y2 = ops.conv2d(xd2, wd, None, 2, 1, "none")
        (y2.float() * gy.to(DEV)).sum().backward()
        close(xd.grad.float(), xd2.grad.float().cpu(), rel=(5e-6 if prec == "fp32" else 1.6e-2), msg="halo form vs im2col form")
    finally:
        ops.set_precision("fp32")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("switch", ["DGRAD_FOLD", "RES_FUSE", "X3_S2", "S2HALO", "S2DGRAD"])
def test_alternative_paths_agree(prec, switch):
    """Every default path that replaced a simpler one this round keeps a switch back to it (DWC_DGRAD_FOLD: reflect-pad adjoint fused
    into the data-gradient GEMM vs a pass of its own; DWC_RES_FUSE: identity-branch gradient of a ResBlock in the convolution's
    epilogue vs autograd's add; DWC_X3_S2 / DWC_BF16_S2_HALO: stride-2 layers on the split-product / halo kernels vs the im2col
    GEMM).  Both settings must give the same gradients up to summation order (fp32) / one bf16 rounding."""
    from networks.networks import ResBlock, Conv2dBlock
    ops.set_precision(prec)
    try:
        torch.manual_seed(7)
        blk = torch.nn.Sequential(Conv2dBlock(64, 128, 4, 2, 1, norm="in", activation="relu", pad_type="reflect"),
                                  ResBlock(128, norm="in", activation="relu", pad_type="reflect")).to(DEV)
        x0 = torch.randn(20, 64, 64, 64, device=DEV)         # (20 images: enough workgroups for the split-product stride-2 forward)
        gy = torch.randn(20, 128, 32, 32, device=DEV)
        res = {}
        old = getattr(ops, switch)
        for val in (1, 0):
            setattr(ops, switch, val)
            x = x0.to(ops.act_dtype()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            for p_ in blk.parameters():
                p_.grad = None
            y = blk(x)
            (y.float() * gy).sum().backward()
            res[val] = [y.detach().float(), x.grad.detach().float()] + [p_.grad.detach().float().clone() for p_ in blk.parameters()
                                                                        if p_.grad is not None]
        setattr(ops, switch, old)
        # (the two paths of a switch round differently -- 2.5e-6 of the scale in fp32 --, and behind a ReLU a value they round to
        # different sides of 0 flips a derivative, which the instance norm's backward then spreads over that (sample, channel) plane
        # at ~1e-4 of the scale: measured 0.25 % of the elements beyond 2e-5, largest 6e-3.  So: the FRACTION of elements beyond a
        # tolerance that such a flip cannot reach, and a cap on the largest difference)
        tol, cap = (2e-3, 5e-2) if prec == "fp32" else (1.6e-2, 2.5e-1)
        for a, b in zip(res[1], res[0]):
            scale = b.abs().max().item() + 1e-12
            d = (a - b).abs()
            bad = (d > tol * scale).float().mean().item()
            # (r05: the norms' backward rebuilds the ReLU mask with the forward's own expression and rounding -- r04's form could
            # disagree with the forward output within an ulp of zero and the bound had been relaxed to 3e-3 for it; back at 1e-3)
            assert bad <= 1e-3 and d.max().item() <= cap * scale, (switch, prec, bad, d.max().item() / scale)
        # the block's output itself (no derivative in between) agrees to rounding
        y1, y0 = res[1][0], res[0][0]
        assert (y1 - y0).abs().max().item() <= (1e-4 if prec == "fp32" else 3.2e-2) * (y0.abs().max().item() + 1e-12)
    finally:
        ops.set_precision("fp32")


# (Cin, Cout, H, k, stride, pad): generic GEMM (stride 2), split-product 3x3 and 5x5; bf16: halo 3x3, generic
NONFINITE_SHAPES = [(64, 64, 16, 4, 2, 1), (256, 256, 16, 3, 1, 1), (128, 64, 16, 5, 1, 2)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_nonfinite_values_propagate(shape, act, prec):
    """torch semantics for non-finite values in every conv epilogue: a NaN in the input stays a NaN on exactly
    the outputs whose receptive field holds it -- through none / ReLU / LeakyReLU (a max/min formulation would turn it into
    0) --, ReLU(-inf) is 0 and LeakyReLU(-inf) is -inf (a -inf bias: added in the epilogue on every kernel path), and a NaN
    in the upstream gradient reaches dx and dw.  A diverged run must not report finite losses."""
    ci, co, H, k, st, p = shape
    B = 2
    ops.set_precision(prec)
    try:
        g = torch.Generator().manual_seed(ci + co + k)
        rnd = (lambda t: t.to(torch.bfloat16).float()) if prec == "bf16" else (lambda t: t)
        x = rnd(torch.randn(B, ci, H, H, generator=g))
        w = torch.randn(co, ci, k, k, generator=g) * (1.0 / (ci * k * k) ** 0.5)
        b = torch.randn(co, generator=g) * 0.1
        x[1, 5, 7, 9] = float("nan")
        b[3] = float("-inf")
        yr = orc.conv_block(x, rnd(w), b, st, p, act=act)

        def prep(t):
            t = t.to(DEV)
            return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last) if prec == "bf16" else t
        xd, wd, bd = prep(x).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        yd = ops.conv2d(xd, wd, bd, st, p, act)
        yh = yd.detach().float().cpu()
        # the reference's NaN footprint must be covered; a transform-domain kernel (Winograd: 4x4 input tile -> 2x2 outputs)
        # may spread the NaN over its tile, never beyond 4x the footprint, and nothing finite may replace a NaN
        nan_h, nan_r = torch.isnan(yh), torch.isnan(yr)
        assert nan_h[nan_r].all(), "a NaN was lost"
        assert nan_h.sum() <= 4 * nan_r.sum(), "NaN spread over more than the transform tile"
        both = ~nan_h
        assert torch.equal(torch.isinf(yh)[both], torch.isinf(yr)[both]), "inf footprint differs"
        assert torch.equal(torch.sign(yh[both & torch.isinf(yr)]), torch.sign(yr[both & torch.isinf(yr)]))
        fin = torch.isfinite(yr) & both
        assert nan_r.any() and fin.sum() > 0 and (torch.isinf(yr).any() or act == "relu")
        tol = 6e-3 if prec == "bf16" else 2e-5
        assert ((yh[fin] - yr[fin]).abs().max() <= tol * yr[fin].abs().max() + 1e-6)
        # backward: a NaN in dy must reach dx (its footprint) and dw (every tap that sees the pixel)
        x2 = rnd(torch.randn(B, ci, H, H, generator=g))
        b2 = torch.randn(co, generator=g) * 0.1
        xr, wr = x2.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y2 = orc.conv_block(xr, rnd(wr.detach()) + (wr - wr.detach()), b2, st, p, act="none")
        gy = rnd(torch.randn(y2.shape, generator=g))
        gy[0, 2, 3, 4] = float("nan")
        (y2 * gy).sum().backward()
        xd2, wd2 = prep(x2).requires_grad_(True), w.to(DEV).requires_grad_(True)
        yd2 = ops.conv2d(xd2, wd2, b2.to(DEV), st, p, "none")
        yd2.backward(prep(gy))
        dxh, dwh = xd2.grad.float().cpu(), wd2.grad.float().cpu()
        # (transform-domain kernels may spread a NaN over the whole transform tile: the reference's footprint must be covered,
        # nothing finite may replace a NaN)
        assert torch.isnan(dxh)[torch.isnan(xr.grad)].all(), "dx lost a NaN"
        assert torch.isnan(dwh)[torch.isnan(wr.grad)].all(), "dw lost a NaN"
        assert torch.isnan(xr.grad).any() and torch.isnan(wr.grad).any()
    finally:
        ops.set_precision("fp32")


@pytest.mark.parametrize("B,C,H,W", [(2, 64, 16, 32), (1, 16, 9, 24), (2, 8, 6, 12), (3, 64, 21, 72), (1, 64, 128, 128)])
def test_fused_image_heads(B, C, H, W):
    """tanh x3 + sigmoid heads as one conv; W % 8 == 0 takes the 'wide' 32-column formulation -- with 64 input channels on the
    dedicated split-product kernel (csrc/conv_narrow_x3.hip; 21 rows / 9 pixel groups: blocks hanging over both image edges)."""
    g = torch.Generator().manual_seed(B + C + H + W)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(4, C, 7, 7, generator=g) * (1.0 / (C * 49) ** 0.5)
    b = torch.randn(4, generator=g) * 0.1
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = orc.conv_block(xr, wr, br, 1, 3)
    yr = torch.cat([torch.tanh(pre[:, :3]), torch.sigmoid(pre[:, 3:4])], 1)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, wd, bd = dev(x, True), dev(w, True), dev(b, True)
    yd = ops.conv2d_heads(xd, wd, bd)
    close(yd, yr, msg="y")
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=5e-5, msg="dx")
    close(wd.grad, wr.grad, rel=5e-5, msg="dw")
    close(bd.grad, br.grad, rel=5e-5, msg="db")


def test_conv_no_bias_and_cout_not_multiple_of_4():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 16, 9, 9, generator=g), torch.randn(3, 16, 3, 3, generator=g) * 0.1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yr = orc.conv_block(xr, wr, None, 1, 1)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, wd = dev(x, True), dev(w, True)
    yd = ops.conv2d(xd, wd, None, 1, 1)
    assert yd.shape == yr.shape
    close(yd, yr)
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=5e-5)
    close(wd.grad, wr.grad, rel=5e-5)


@pytest.mark.parametrize("T,B,I,H,lens", [
    (7, 3, 12, 16, [7, 4, 1]),                        # tiny configuration, one sample of length 1
    (40, 16, 364, 300, None),                         # the shipped text encoder, layer 0
    (12, 20, 600, 300, None),                         # layer 1 input width, two 16-row tiles
    (6, 70, 12, 20, None),                            # more than 64 sequences (row chunks), H not a multiple of 16
])
@pytest.mark.parametrize("seq", [1, 0], ids=["persistent", "per-step"])
@pytest.mark.parametrize("hip_gemm", [1, 0], ids=["hip-gemm", "torch-gemm"])
def test_lstm_bidir_matches_packed_nn_lstm(T, B, I, H, lens, seq, hip_gemm, monkeypatch):
    """One bidirectional layer on padded input + lengths against torch's nn.LSTM on the PackedSequence (what the
    reference runs, networks_v2.py:226-233): outputs, final states, and every gradient -- with the forward recurrence as ONE
    persistent launch (workgroups hand h_t to each other inside the launch) and as one launch per time step; the layer's dense
    products (input projection, its input / weight gradients, the recurrent weight gradient) on the HIP GEMM kernels
    (ops._gemm_nt / _gemm_nn / _gemm_tn: widths 364, 600, 1200 -- no powers of two) and through torch."""
    monkeypatch.setattr(ops, "LSTM_SEQ", seq)
    if hip_gemm and not (ops.gemm_ok(I, 4 * H) and ops.gemm_ok(H, 4 * H)):
        pytest.skip("widths the HIP GEMM path does not take (ops falls back to torch by itself)")
    g = torch.Generator().manual_seed(T * 1000 + B + H)
    if lens is None:
        lens = sorted((int(v) for v in torch.randint(1, T + 1, (B,), generator=g)), reverse=True)
        lens[0] = T
    x = torch.randn(T, B, I, generator=g)
    ref = torch.nn.LSTM(I, H, 1, bidirectional=True)
    with torch.no_grad():
        for prm in ref.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * (1.0 / H ** 0.5))
    xr = x.clone().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xr, lens)
    outs, (hn, cn) = ref(packed)
    mem, _ = torch.nn.utils.rnn.pad_packed_sequence(outs, total_length=T)
    g1, g2, g3 = torch.randn(mem.shape, generator=g), torch.randn(hn.shape, generator=g), torch.randn(cn.shape, generator=g)
    ((mem * g1).sum() + (hn * g2).sum() + (cn * g3).sum()).backward()

    xd = dev(x, True)
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    par = {n: [dev(getattr(ref, n + "_l0" + suf), True) for suf in ("", "_reverse")] for n in names}
    lens_t = torch.tensor(lens)
    out, cell = ops.lstm_bidir(xd, lens_t.to(torch.int32).to(DEV), *[torch.stack(par[n]) for n in names],
                               owners=tuple(par["weight_ih"]) if hip_gemm else None)
    if seq:                      # the persistent launch's sticky status word (caller-owned, outside the scratch arena): no rendez-vous missed
        ops.lstm_status_poll(torch.device(DEV))
        ops.lstm_status_poll(torch.device(DEV), wait=True)
        assert int(ops._lstm_status(torch.device(DEV))[0].item()) == 0
    last, cols = (lens_t - 1).to(DEV), torch.arange(B, device=DEV)
    mem_d = torch.cat([out[0], out[1]], -1)
    hn_d = torch.stack([out[0][last, cols], out[1][0]])
    cn_d = torch.stack([cell[0][last, cols], cell[1][0]])
    close(mem_d, mem, rel=2e-5, msg="outputs")
    close(hn_d, hn, rel=2e-5, msg="h_n")
    close(cn_d, cn, rel=2e-5, msg="c_n")
    ((mem_d * g1.to(DEV)).sum() + (hn_d * g2.to(DEV)).sum() + (cn_d * g3.to(DEV)).sum()).backward()
    close(xd.grad, xr.grad, rel=1e-4, msg="dx")
    for n in names:
        for k, suf in enumerate(("", "_reverse")):
            close(par[n][k].grad, getattr(ref, n + "_l0" + suf).grad, rel=1e-4, msg=n + suf)


@pytest.mark.parametrize("M,K,N", [(16, 2400, 128), (640, 364, 1200), (37, 600, 1200), (5, 12, 8), (3000, 1200, 364)])
def test_linear_any_matches_float64(M, K, N):
    """nn.Linear with widths that are no powers of two on the im2col GEMM kernels (a K-wide row read as K/c pixels of c channels;
    ops.linear_any: the 2 x num_class text heads, reference networks_v2.py:204-205, and the LSTM's dense products): y, dx, dw, db
    against float64 at fp32 accuracy."""
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * (1.0 / K ** 0.5), torch.randn(N, generator=g)
    gy = torch.randn(M, N, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yr = torch.nn.functional.linear(xr, wr, br)
    (yr * gy.double()).sum().backward()
    xd, wd, bd = dev(x, True), dev(w, True), dev(b, True)
    y = ops.linear_any(xd, wd, bd)
    (y * gy.to(DEV)).sum().backward()
    for name, got, ref in (("y", y, yr), ("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad), ("db", bd.grad, br.grad)):
        scale = ref.abs().max().item()
        err = (got.detach().double().cpu() - ref.detach()).abs().max().item() / scale
        assert err <= 2e-5, "%s: %.3e of scale" % (name, err)
    # the prepared layouts follow the parameter: an in-place update must not be served from the cache
    with torch.no_grad():
        wd.mul_(2.0)
    y2 = ops.linear_any(xd.detach(), wd, bd)
    ref2 = torch.nn.functional.linear(x.double(), 2.0 * w.double(), b.double())
    assert (y2.detach().double().cpu() - ref2).abs().max().item() / ref2.abs().max().item() <= 2e-5


def test_lstm_persistent_launch_refuses_grids_that_cannot_be_resident(monkeypatch):
    """The hand-off inside dwc_lstm_seq_* needs every workgroup of the launch resident.  The launcher derives the capacity from
    the device (CU count x occupancy) and an optional caller cap: a grid above it is refused with DWC_EINVAL BEFORE anything is
    launched (ops then runs the per-step kernels, same results), and a failed hand-off is reported through the sticky status
    word, not through scratch memory."""
    from hipdwc import _lib
    lib = _lib.load()
    T, B, H = 5, 16, 300
    d = torch.device(DEV)
    xproj = torch.randn(2, T, B, 4 * H, device=d)
    w_hh = torch.randn(2, 4 * H, H, device=d) * 0.05
    lens = torch.full((B,), T, dtype=torch.int32, device=d)
    out, c, gates = (torch.empty(2, T, B, n, device=d) for n in (H, H, 4 * H))
    nws = lib.dwc_lstm_seq_ws_bytes(B, 2)
    assert nws % 16 == 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=d)          # EXACTLY the size the library asks for
    status = torch.zeros(1, dtype=torch.int32, device=d)
    st = torch.cuda.current_stream().cuda_stream
    args = (xproj.data_ptr(), w_hh.data_ptr(), lens.data_ptr(), out.data_ptr(), c.data_ptr(), gates.data_ptr(), T, B, H, 2,
            ws.data_ptr(), nws, status.data_ptr())
    assert lib.dwc_lstm_seq_fwd(*args, 37, st) == _lib.EINVAL     # 19 groups x 2 directions = 38 workgroups > cap 37
    assert lib.dwc_lstm_seq_fwd(*args, 38, st) == 0
    ref_out = torch.empty_like(out)
    _lib.check(lib.dwc_lstm_fwd(xproj.data_ptr(), w_hh.data_ptr(), lens.data_ptr(), ref_out.data_ptr(), c.data_ptr(), gates.data_ptr(),
                                T, B, H, 2, st), "lstm_fwd")
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.isfinite(out).all()
    close(out, ref_out.cpu(), rel=1e-5)
    # through ops: a cap below the grid silently takes the per-step kernels
    monkeypatch.setattr(ops, "LSTM_SEQ_MAX_WORKGROUPS", 1)        # 1 group x 2 directions = 2 workgroups > 1
    x = torch.randn(T, B, 12, device=d)
    par = [torch.randn(2, 4 * 16, 12, device=d), torch.randn(2, 4 * 16, 16, device=d), torch.randn(2, 64, device=d), torch.randn(2, 64, device=d)]
    a, _ = ops.lstm_bidir(x, lens, *par)
    monkeypatch.setattr(ops, "LSTM_SEQ_MAX_WORKGROUPS", 0)
    b, _ = ops.lstm_bidir(x, lens, *par)
    close(a, b.cpu(), rel=1e-5)


def test_instance_norm_last_arriver_two_streams_stress():
    """Two streams run norm forward + backward launches of different shapes concurrently, 200 rounds: every result must equal, BIT FOR
    BIT, what the same launches give when run alone on one stream (per-stream scratch, fixed summation order, no library-global
    state).  (Rounds 3-4 finalised the statistics in the last-arriving workgroup of a sample through caller-owned
    ticket rows, which is what the test's name refers to; r05 removed that mechanism -- csrc/norm.hip -- and the test keeps guarding the
    concurrency of what replaced it: partial + parallel finalise launches, and the resident-plane kernels.)  Shapes on both kinds of
    kernels: 32x32 / 16x16 planes are resident, 8x8 and 64x64 go through the multi-pass kernels."""
    d = torch.device(DEV)
    shapes = [(16, 256, 32), (48, 64, 16), (5, 128, 8), (8, 128, 64)]
    g = torch.Generator().manual_seed(5)
    data = []
    for (B, C, H) in shapes:
        x = (torch.randn(B, C, H, H, generator=g) * 1.5 + 0.3).to(d).contiguous(memory_format=torch.channels_last)
        ga, be = (torch.randn(B * C, generator=g) * 0.5 + 1).to(d), torch.randn(B * C, generator=g).to(d)
        gy = torch.randn(B, C, H, H, generator=g).to(d).contiguous(memory_format=torch.channels_last)
        data.append((x, ga, be, gy))

    def run(x, ga, be, gy):
        xr = x.detach().clone().requires_grad_(True)
        gr, br = ga.detach().clone().requires_grad_(True), be.detach().clone().requires_grad_(True)
        y = ops.instance_norm(xr, gr, br, relu=True)
        (y * gy).sum().backward()
        return [y.detach(), xr.grad, gr.grad, br.grad]

    want = [run(*t) for t in data]                              # alone on the default stream
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = {}
    for rnd in range(200):
        for si, st in enumerate(streams):
            with torch.cuda.stream(st):
                k = (rnd + 2 * si) % len(data)
                got[(si, k)] = run(*data[k])
    torch.cuda.synchronize()
    for (si, k), res in got.items():
        for a, b, name in zip(res, want[k], ("y", "dx", "dgamma", "dbeta")):
            assert torch.equal(a, b), (si, k, name, (a - b).abs().max().item())


@pytest.mark.parametrize("B,C,H", [(2, 256, 16), (3, 64, 32), (1, 128, 8), (2, 8, 6), (2, 512, 2), (5, 256, 32)])
@pytest.mark.parametrize("mode", ["in", "in_relu", "adain_relu", "adain_res"])
def test_instance_norm(B, C, H, mode):
    g = torch.Generator().manual_seed(B * 1000 + C + H)
    x = torch.randn(B, C, H, H, generator=g) * 2 + 0.7
    res = torch.randn(B, C, H, H, generator=g) if mode.endswith("res") else None
    ga = (torch.randn(B * C, generator=g) * 0.5 + 1) if mode.startswith("adain") else None
    be = torch.randn(B * C, generator=g) if mode.startswith("adain") else None
    relu = mode.endswith("relu")
    leaves = [t.clone().requires_grad_(True) for t in (x, res, ga, be) if t is not None]
    it = iter(leaves)
    xr = next(it)
    rr = next(it) if res is not None else None
    gr, br = (next(it), next(it)) if ga is not None else (None, None)
    yr = orc.adain(xr, gr, br) if ga is not None else orc.instance_norm(xr)
    if relu:
        yr = torch.clamp_min(yr, 0)
    if rr is not None:
        yr = yr + rr
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd = dev(x, True)
    rd = dev(res, True) if res is not None else None
    gd, bd = (dev(ga, True), dev(be, True)) if ga is not None else (None, None)
    yd = ops.instance_norm(xd, gd, bd, residual=rd, relu=relu)
    close(yd, yr, rel=3e-5, msg="y")
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=2e-4, msg="dx")
    if rd is not None:
        close(rd.grad, rr.grad, msg="dres")
    if gd is not None:
        close(gd.grad, gr.grad, rel=1e-4, msg="dgamma")
        close(bd.grad, br.grad, rel=1e-4, msg="dbeta")


@pytest.mark.parametrize("B,C,H", [(3, 128, 16), (1, 64, 32), (2, 8, 10)])
@pytest.mark.parametrize("relu", [False, True])
def test_layer_norm(B, C, H, relu):
    g = torch.Generator().manual_seed(B + C + H)
    x = torch.randn(B, C, H, H, generator=g) * 1.5 - 0.3
    ga, be = torch.rand(C, generator=g), torch.randn(C, generator=g) * 0.1
    xr, gr, br = [t.clone().requires_grad_(True) for t in (x, ga, be)]
    yr = orc.layer_norm_munit(xr, gr, br)
    if relu:
        yr = torch.clamp_min(yr, 0)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd, gd, bd = dev(x, True), dev(ga, True), dev(be, True)
    yd = ops.layer_norm_munit(xd, gd, bd, relu=relu)
    close(yd, yr, rel=3e-5, msg="y")
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=2e-4, msg="dx")
    close(gd.grad, gr.grad, rel=1e-4, msg="dgamma")
    close(bd.grad, br.grad, rel=1e-4, msg="dbeta")


def test_resample_and_golden(golden_dir):
    gold = np.load(os.path.join(golden_dir, "ops_golden.npz"))
    g = torch.Generator().manual_seed(3)
    # (the kernels walk 8 input rows per thread: 19 = two full row blocks + a partial one)
    for (B, C, H, W) in [(2, 4, 5, 6), (1, 64, 16, 16), (2, 8, 1, 3), (1, 8, 19, 7)]:
        x = torch.randn(B, C, H, W, generator=g)
        xr = x.clone().requires_grad_(True)
        yr = orc.upsample_bilinear2x(xr)
        gy = torch.randn(yr.shape, generator=g)
        (yr * gy).sum().backward()
        xd = dev(x, True)
        yd = ops.upsample2x(xd)
        close(yd, yr, rel=1e-6)
        (yd * gy.to(DEV)).sum().backward()
        close(xd.grad, xr.grad, rel=1e-6)
    xd = dev(T(gold["up2/x"]), True)
    yd = ops.upsample2x(xd)
    close(yd, T(gold["up2/y"]), rel=1e-6, msg="golden up2")
    (yd * T(gold["up2/gy"]).to(DEV)).sum().backward()
    close(xd.grad, T(gold["up2/dx"]), rel=1e-6, msg="golden up2 dx")
    for (B, C, H, W) in [(2, 4, 8, 12), (1, 64, 16, 16)]:
        x = torch.randn(B, C, H, W, generator=g)
        xr = x.clone().requires_grad_(True)
        yr = orc.downsample_half(xr)
        gy = torch.randn(yr.shape, generator=g)
        (yr * gy).sum().backward()
        xd = dev(x, True)
        yd = ops.downsample_half(xd)
        close(yd, yr, rel=1e-6)
        (yd * gy.to(DEV)).sum().backward()
        close(xd.grad, xr.grad, rel=1e-6)


def test_pack_blend_l1():
    g = torch.Generator().manual_seed(11)
    x3 = torch.randn(2, 3, 8, 8, generator=g)
    xd = dev(x3, True)
    x4 = ops.pack_image(xd)
    assert x4.shape == (2, 4, 8, 8) and x4.is_contiguous(memory_format=torch.channels_last)
    close(x4[:, :3], x3, rel=0, atol=0)
    assert float(x4[:, 3].abs().max()) == 0.0
    gy = torch.randn(2, 4, 8, 8, generator=g)
    (x4 * gy.to(DEV)).sum().backward()
    close(xd.grad, gy[:, :3], rel=0, atol=0)
    # blend
    heads = torch.cat([torch.tanh(torch.randn(2, 3, 8, 8, generator=g)), torch.sigmoid(torch.randn(2, 1, 8, 8, generator=g))], 1)
    real = torch.cat([x3, torch.zeros(2, 1, 8, 8)], 1)
    hr = heads.clone().requires_grad_(True)
    outr = hr[:, :3] * hr[:, 3:4] + real[:, :3] * (1 - hr[:, 3:4])
    go = torch.randn(outr.shape, generator=g)
    (outr * go).sum().backward()
    hd = dev(heads, True)
    outd = ops.attention_blend(hd, dev(real))
    close(outd[:, :3], outr, rel=1e-6)
    (outd[:, :3] * go.to(DEV)).sum().backward()
    close(hd.grad, hr.grad, rel=1e-5)
    # l1, plain and image flavour, odd sizes
    for shape, image in [((2, 256, 8, 8), False), ((3, 4, 9, 7), True), ((5, 64), False)]:
        a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        lr_ = (ar[:, :3] - br[:, :3]).abs().mean() if image else (ar - br).abs().mean()
        (lr_ * 3.0).backward()
        ad, bd = dev(a, True), dev(b, True)
        ld = ops.l1_mean(ad, bd, image=image)
        assert abs(float(ld) - float(lr_)) <= 1e-6 * max(1.0, abs(float(lr_)))
        (ld * 3.0).backward()
        close(ad.grad, ar.grad, rel=1e-6)
        close(bd.grad, br.grad, rel=1e-6)


def test_fused_adam_and_ema_match_torch():
    """Multi-tensor HIP Adam/EMA against torch.optim.Adam (CPU, single-tensor path) and torch.lerp:
    odd sizes across the 8192-element chunking, a parameter that never gets a gradient (must be
    skipped: no weight decay, no step count), another that gets one only on some steps."""
    from hipdwc.optim import FusedAdam, FusedEMA
    g = torch.Generator().manual_seed(0)
    shapes = [(7,), (8192,), (8193,), (3, 5, 7, 7), (20000,), (64, 33), (11,)]
    ref = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    hip = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref]
    kw = dict(lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-4)
    o_ref, o_hip = torch.optim.Adam(ref, foreach=False, **kw), FusedAdam(hip, **kw)
    for step in range(5):
        for i, (a, b) in enumerate(zip(ref, hip)):
            if i == 6 or (i == 2 and step % 2 == 1):       # no gradient at all / only on even steps
                a.grad, b.grad = None, None
                continue
            gr = torch.randn(a.shape, generator=g)
            a.grad, b.grad = gr.clone(), gr.to(DEV)
        o_ref.step()
        ver = [b._version for b in hip]
        o_hip.step()
        # the raw-pointer update must still bump autograd's version counters (the prepared-weight
        # cache in hipdwc.ops keys on them): exactly the tensors that were updated
        for i, b in enumerate(hip):
            assert (b._version > ver[i]) == (b.grad is not None), i
    for i, (a, b) in enumerate(zip(ref, hip)):
        close(b, a, rel=2e-6, atol=1e-7, msg="param %d" % i)
        if i != 6:
            close(o_hip.state[b]["exp_avg"], o_ref.state[a]["exp_avg"], rel=2e-6, msg="m %d" % i)
            close(o_hip.state[b]["exp_avg_sq"], o_ref.state[a]["exp_avg_sq"], rel=2e-6, msg="v %d" % i)
            assert float(o_hip.state[b]["step"]) == float(o_ref.state[a]["step"])
    assert torch.equal(hip[6].cpu(), ref[6].detach())       # untouched
    assert set(o_hip.state_dict()["state"][0].keys()) == set(o_ref.state_dict()["state"][0].keys())
    src, dst = torch.nn.ParameterList(hip), torch.nn.ParameterList([torch.nn.Parameter(torch.randn_like(p)) for p in hip])
    want = [torch.lerp(a.detach().cpu(), b.detach().cpu(), 0.999) for a, b in zip(src, dst)]
    FusedEMA(src, dst).step(0.999)
    for w, b in zip(want, dst):
        close(b, w, rel=1e-6, atol=1e-7, msg="ema")


def test_golden_conv_blocks(golden_dir):
    """The reference's own Conv2dBlock vectors (conv + norm + activation, forward and backward)."""
    import networks.networks as nets
    gold = np.load(os.path.join(golden_dir, "ops_golden.npz"))
    cases = {"stem7_relu": ("none", "relu"), "down4_in_relu": ("in", "relu"), "res3_in_none": ("in", "none"),
             "res3_adain_relu": ("adain", "relu"), "up5_ln_relu": ("ln", "relu"), "up5_ln_relu_b1": ("ln", "relu"),
             "head7_tanh": ("none", "tanh"), "head7_sigmoid": ("none", "sigmoid"), "dis4_lrelu": ("none", "lrelu"),
             "dis4_lrelu_2x2": ("none", "lrelu")}
    for name, (norm, act) in cases.items():
        gg = lambda k: T(gold["conv/%s/%s" % (name, k)])
        B, ci, co, H, k, s, p = [int(v) for v in gold["conv/%s/meta" % name]]
        blk = nets.Conv2dBlock(ci, co, k, s, p, norm=norm, activation=act, pad_type="reflect").to(DEV)
        with torch.no_grad():
            blk.conv.weight.copy_(gg("w"))
            blk.conv.bias.copy_(gg("b"))
            if norm == "ln":
                blk.norm.gamma.copy_(gg("gamma"))
                blk.norm.beta.copy_(gg("beta"))
        x = dev(gg("x"), True)
        if norm == "adain":
            blk.norm.weight, blk.norm.bias = dev(gg("aw"), True), dev(gg("ab"), True)
        y = blk(x)
        close(y, gg("y"), rel=5e-5, atol=2e-6, msg=name + " y")
        (y * gg("gy").to(DEV)).sum().backward()
        close(x.grad, gg("dx"), rel=3e-4, atol=2e-6, msg=name + " dx")
        close(blk.conv.weight.grad, gg("dw"), rel=3e-4, atol=2e-6, msg=name + " dw")
        if norm == "none":
            close(blk.conv.bias.grad, gg("db"), rel=3e-4, atol=2e-6, msg=name + " db")
        if norm == "ln":
            close(blk.norm.gamma.grad, gg("dgamma"), rel=3e-4, msg=name + " dgamma")
            close(blk.norm.beta.grad, gg("dbeta"), rel=3e-4, msg=name + " dbeta")
        if norm == "adain":
            close(blk.norm.weight.grad, gg("daw"), rel=3e-4, msg=name + " daw")
            close(blk.norm.bias.grad, gg("dab"), rel=3e-4, msg=name + " dab")


REACH_CASES = [  # (name, B, Cin, Cout, H, k, s, p, norm, act, pad_type) -- tests/golden/make_golden.py REACH_CASES
    ("zero3_bn_prelu", 3, 8, 16, 10, 3, 1, 1, "bn", "prelu", "zero"),
    ("rep5_none_selu", 2, 8, 8, 12, 5, 1, 2, "none", "selu", "replicate"),
    ("zero3_in_lrelu", 2, 8, 16, 12, 3, 1, 1, "in", "lrelu", "zero"),
    ("rep3_ln_prelu", 2, 16, 8, 8, 3, 1, 1, "ln", "prelu", "replicate"),
    ("zero3_none_relu", 2, 8, 8, 9, 3, 1, 1, "none", "relu", "zero"),
]


@pytest.mark.parametrize("case", REACH_CASES, ids=lambda c: c[0])
def test_conv_block_beyond_shipped_configs_vs_reference(golden_dir, case):
    """The part of the reference's Conv2dBlock signature no shipped configuration uses (networks.py:530-567): zero / replicate
    padding, BatchNorm, PReLU / SELU and a norm followed by a non-ReLU activation -- reachable since r05 through device torch ops
    around the HIP convolution.  Forward, dx, dw, db and the norm / activation parameters' gradients against vectors recorded
    from the imported reference (tests/golden/make_golden.py reach), BatchNorm's running statistics included."""
    import networks.networks as nets
    gold = np.load(os.path.join(golden_dir, "conv_reach.npz"))
    name, B, ci, co, H, k, s_, p, norm, act, pad = case
    gg = lambda key: T(gold["%s/%s" % (name, key)])
    blk = nets.Conv2dBlock(ci, co, k, s_, p, norm=norm, activation=act, pad_type=pad).to(DEV)
    with torch.no_grad():
        blk.conv.weight.copy_(gg("w"))
        blk.conv.bias.copy_(gg("b"))
        if norm == "ln":
            blk.norm.gamma.copy_(gg("gamma"))
            blk.norm.beta.copy_(gg("beta"))
        if norm == "bn":
            blk.norm.weight.copy_(gg("bn_w"))
            blk.norm.bias.copy_(gg("bn_b"))
        if act == "prelu":
            blk.activation.weight.fill_(0.3)
    x = dev(gg("x"), True)
    y = blk(x)
    close(y, gg("y"), rel=5e-5, atol=2e-6, msg=name + " y")
    (y * gg("gy").to(DEV)).sum().backward()
    close(x.grad, gg("dx"), rel=3e-4, atol=2e-6, msg=name + " dx")
    close(blk.conv.weight.grad, gg("dw"), rel=3e-4, atol=2e-6, msg=name + " dw")
    if norm == "none":
        close(blk.conv.bias.grad, gg("db"), rel=3e-4, atol=2e-6, msg=name + " db")
    if norm == "ln":
        close(blk.norm.gamma.grad, gg("dgamma"), rel=3e-4, msg=name + " dgamma")
        close(blk.norm.beta.grad, gg("dbeta"), rel=3e-4, msg=name + " dbeta")
    if norm == "bn":
        close(blk.norm.weight.grad, gg("dbn_w"), rel=3e-4, msg=name + " dbn_w")
        close(blk.norm.bias.grad, gg("dbn_b"), rel=3e-4, msg=name + " dbn_b")
        close(blk.norm.running_mean, gg("running_mean"), rel=1e-5, msg=name + " running_mean")
        close(blk.norm.running_var, gg("running_var"), rel=1e-5, msg=name + " running_var")
    if act == "prelu":
        close(blk.activation.weight.grad, gg("dprelu"), rel=3e-4, msg=name + " dprelu")


# ----------------------------------------------------------------------------------------
# whole modules / solver on the tiny config, against the reference's recorded run
# ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    return np.load(os.path.join(golden_dir, "tiny_step.npz"))


def _tiny_solver(tiny):
    from solver import Solver
    cfg = synth.make_config(image_size=32, tiny=True)
    torch.manual_seed(1234)
    s = Solver(cfg, torch.device(DEV), None).to(DEV)
    s.copy_nets()
    assert torch.equal(torch.get_rng_state(), T(tiny["rng_state_after_init"]))
    batch = {k[len("batch/"):]: T(tiny[k]) for k in tiny.files if k.startswith("batch/")}
    return s, cfg, {k: v.to(DEV) for k, v in batch.items()}


def test_tiny_modules_vs_reference(tiny):
    s, cfg, batch = _tiny_solver(tiny)
    s.eval()
    with torch.no_grad():
        content, mus, lvs = s.gen.encode(batch["x_real"])
        close(content, T(tiny["mod/content"]), rel=1e-4, msg="content")
        close(torch.stack(mus), T(tiny["mod/style_mu"]), rel=1e-4, msg="style mu")
        close(torch.stack(lvs), T(tiny["mod/style_logvar"]), rel=1e-4, msg="style logvar")
        style = torch.cat(mus, 1)
        tmu, tlv = s.gen.encode_txt(style, batch["txt"], batch["txt_lens"])
        close(torch.stack(tmu), T(tiny["mod/txt_mu"]), rel=1e-4, msg="txt mu")
        close(torch.stack(tlv), T(tiny["mod/txt_logvar"]), rel=1e-4, msg="txt logvar")
        img, att = s.gen.decode(content, style)
        close(img, T(tiny["mod/dec_img"]), rel=1e-4, msg="image")
        close(att, T(tiny["mod/dec_att"]), rel=1e-4, msg="attention")
        for i, (src, cls) in enumerate(s.dis(batch["x_real"])):
            close(src, T(tiny["mod/dis%d_src" % i]), rel=1e-4, msg="dis src")
            close(cls, T(tiny["mod/dis%d_cls" % i]), rel=1e-4, msg="dis cls")


@pytest.mark.parametrize("size", ["tiny", "full"])
def test_grouped_decode_equals_concatenated_decode(tiny, size):
    """r05: the solver decodes ONE content code with two / three styles in one pass (reference solver.py:171-190 calls gen.decode
    three times on c_real); the decoder's first convolution sees the same input in every group, so it runs once at batch B and its
    output is repeated in front of the AdaIN (networks.ResBlock._forward_groups).  Same result as decoding torch.cat([content] * 3):
    image heads within 2e-6 of their scale, gradients w.r.t. the content code, the first and the second convolution's weights and the
    style within 2e-5 (fp32 summation order: the groups' gradients meet before the convolution instead of inside its batch)."""
    from solver import Solver
    if size == "tiny":
        s, cfg, batch = _tiny_solver(tiny)
        x = batch["x_real"]
    else:
        cfg = synth.make_config(image_size=64)
        torch.manual_seed(7)
        s = Solver(cfg, torch.device(DEV), None).to(DEV)
        x = synth.make_batch(2, 64, seed=3)["x_real"].to(DEV)
    gen = s.gen
    B = x.shape[0]
    with torch.no_grad():
        content0, mus, _ = gen.encode(ops.pack_image(x))
        width = torch.cat(list(mus), 1).shape[1]
    g = torch.Generator().manual_seed(21)
    style0 = torch.randn(3 * B, width, generator=g).to(DEV)
    w1 = gen.dec.model[0].model[0].model[0].conv.weight
    w2 = gen.dec.model[0].model[0].model[1].conv.weight
    gy = None
    outs = []
    for grouped in (True, False):
        content = content0.detach().clone().requires_grad_(True)
        style = style0.detach().clone().requires_grad_(True)
        gen.zero_grad(set_to_none=True)
        heads = gen.decode_nhwc4(content, style, groups=3) if grouped else gen.decode_nhwc4(torch.cat([content] * 3), style)
        if gy is None:
            gy = torch.randn(heads.shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
        (heads * gy).sum().backward()
        outs.append([heads.detach(), content.grad.detach(), w1.grad.detach().clone(), w2.grad.detach().clone(), style.grad.detach()])
    for a, b, name in zip(outs[0], outs[1], ("heads", "d content", "d w (first conv)", "d w (second conv)", "d style")):
        close(a, b, rel=2e-6 if name == "heads" else 2e-5, msg="grouped vs concatenated decode: " + name)


def test_tiny_three_iterations_vs_reference(tiny):
    """Same seed, same random stream (HostNoise), three full iterations: every loss scalar the
    reference printed, its G gradients and its post-Adam weights after iteration 0."""
    want = json.loads(bytes(tiny["losses_json"]).decode())
    host.set_noise(host.HostNoise())
    try:
        s, cfg, batch = _tiny_solver(tiny)
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg)
        for it in range(3):
            s.dis_update(*a, it)
            s.gen_update(*a, it)
            if it == 0:
                # (convolution biases in front of an instance norm carry `_dwc_zero_grad` since r06: autograd hands them no gradient
                # tensor, FusedAdam steps them with zeros -- the identically-zero gradient the reference computes as rounding noise)
                grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
                         for k, p in s.gen.named_parameters() if p.grad is not None or getattr(p, "_dwc_zero_grad", False)}
                assert any(getattr(p, "_dwc_zero_grad", False) and p.grad is None for p in s.gen.parameters())
            if it == 1:
                # attention is off from iteration 1: the head must get NO gradient (Adam then skips it,
                # SURVEY section 7 quirk viii) rather than a zero one
                assert s.gen.dec.image_attention.conv.weight.grad is None
                assert s.gen.dec.image_attention.conv.bias.grad is None
            s.smooth_moving()
            s.update_learning_rate()
            s.update_attention_status(it)
            # iteration 0 sees the reference's own weights (2e-4).  From iteration 1 on every parameter has
            # taken an Adam sign-descent step of +-lr, and entries whose true gradient is ~0 go either way
            # under ANY change of summation order: the reference drifts from itself by 1e-4 / 5e-3 (relative,
            # loss_gen_total) at iterations 1 / 2 when only its thread count changes (tests/test_trajectory.py).
            tol = (2e-4, 5e-3, 2e-2)[it]
            for k, v in want[it].items():
                got = float(torch.as_tensor(getattr(s, k)).detach())
                assert abs(got - v) <= tol * max(1.0, abs(v)), (it, k, got, v)
            if it == 0:
                ref_g ={k[len("grad_it0/gen/"):]: T(tiny[k]) for k in tiny.files if k.startswith("grad_it0/gen/")}
                assert set(grads.keys()) == set(ref_g.keys())
                for k, gref in ref_g.items():
                    close(grads[k], gref, rel=5e-3, msg=k)
                lr, off, total = cfg["lr"], 0, 0
                for prefix, mod in (("after_it0/gen/", s.gen), ("after_it0/dis/", s.dis)):
                    sd = mod.state_dict()
                    for k in tiny.files:
                        if k.startswith(prefix) and "running_" not in k:
                            d = (sd[k[len(prefix):]].cpu() - T(tiny[k])).abs()
                            assert d.max().item() <= 2.05 * lr, k
                            off += int((d > 1e-6).sum())
                            total += d.numel()
                assert off <= 0.02 * total
        assert abs(s.init_ds_w - float(tiny["init_ds_w"])) < 1e-12
    finally:
        host.set_noise(host.DeviceNoise())


FULL_SAMPLE = 8192


def full_sample_idx(n):
    """Element numbers a full-size fixture keeps of a flattened n-element gradient (tests/golden/make_golden.py sample_idx)."""
    if n <= FULL_SAMPLE:
        return torch.arange(n)
    return (torch.arange(FULL_SAMPLE, dtype=torch.int64) * n) // FULL_SAMPLE


def check_full_grads(fx, prefix, params, rel):
    """Sampled gradient entries of the imported reference (<= 8192 evenly spread per tensor) + the tensor's sum of squares."""
    names = sorted({k.split("/")[1] for k in fx.files if k.startswith(prefix + "/")})
    assert names
    for name in names:
        g = params[name].grad
        assert g is not None, name
        flat = g.detach().float().reshape(-1).cpu()
        want = torch.from_numpy(fx["%s/%s/sample" % (prefix, name)])
        amax, _, sumsq = (float(v) for v in fx["%s/%s/stats" % (prefix, name)])
        err = (flat[full_sample_idx(flat.numel())] - want).abs().max().item()
        assert err <= rel * amax + 1e-6, "%s: sampled max err %.3e > %.3e" % (name, err, rel * amax + 1e-6)
        got_sq = float(flat.double().pow(2).sum())
        assert abs(got_sq - sumsq) <= 4 * rel * sumsq, (name, got_sq, sumsq)


@pytest.mark.parametrize("S,B,what", [(128, 2, "all"), (256, 1, "all"), (128, 64, "dis"), (256, 8, "dis"),
                                      (128, 64, "all"), (256, 8, "all")])
def test_full_size_iteration_vs_oracle(S, B, what, golden_dir):
    """The shipped network sizes (dim 64, 4 ResBlocks, 5-layer 2-scale D) at 128x128 and at the 256x256 of
    BASELINE configs[4]: one full iteration against the IMPORTED REFERENCE itself, run once in the build container from the same
    seeded initialisation, batch and random stream (tests/golden/make_golden.py full*: reference solver.py:151-240,317-353; the
    batch-64 run parks autograd's saved tensors on disk) -- every loss scalar, sampled gradient entries and the sum of squares of
    representative tensors.  (Rounds 1-4 ran the CPU oracle here, ~1 min and ~60 GB of host memory per batch-64 iteration on the
    GPU box; tests/test_oracle_golden.py now holds the oracle to the same fixtures on the CPU.)  Exercises the real layer shapes
    (128x128 tiles, split-K tails, wide heads) that the tiny configuration cannot.  (128, 64) and (256, 8) are the PER-GPU
    shapes of BASELINE configs[3] (global batch 512 on 8 GPUs) and configs[4] (global batch 64 on 8 GPUs): the D step alone
    ("dis") and the WHOLE iteration incl. the G step ("all": all 16 scalars + generator gradients)."""
    from solver import Solver
    fx = np.load(os.path.join(golden_dir, "full_s%d_b%d.npz" % (S, B)))
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
        for k in ("loss_dis", "loss_dis_all"):
            got, want = float(getattr(s, k)), float(fx[k])
            assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (k, got, want)
        check_full_grads(fx, "dgrad", dict(s.dis.named_parameters()), 1e-2)
        if what == "dis":
            return
        s.gen_update(*a)
        losses = json.loads(bytes(fx["losses_json"]).decode())
        for k, want in losses.items():
            got = float(torch.as_tensor(getattr(s, k)).detach())
            assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (k, got, want)
        # gradients of representative tensors (stem, ResBlocks, 5x5, heads, style MLP, style encoder, LSTM): whole-network gradient
        check_full_grads(fx, "ggrad", dict(s.gen.named_parameters()), 1e-2)
    finally:
        host.set_noise(host.DeviceNoise())


def test_em_distance_iteration_vs_oracle():
    """dist_mode != 'kls': the generator objective with gmm_earth_mover_distance_sp (reference gmm.py:33-41, solver.py:210-213)
    in place of the KL terms — unreachable under the shipped config, reachable through the API: two tiny iterations against
    the oracle, all scalars, plus the gradient that only this branch produces (d loss_kl_x / d style-encoder heads)."""
    from solver import Solver
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    cfg["dist_mode"] = "em"
    host.set_noise(host.HostNoise())
    try:
        torch.manual_seed(99)
        s = Solver(cfg, torch.device(DEV), None).to(DEV)
        s.copy_nets()
        rng = torch.get_rng_state()
        batch = synth.make_batch(3, 32, seed=12)
        oracle = orc.OracleSolver(cfg, {k: v.cpu() for k, v in s.gen.state_dict().items()},
                                  {k: v.cpu() for k, v in s.dis.state_dict().items()})
        oracle.copy_nets()
        o_losses, o_grads = [], None
        for it in range(2):
            oracle.iteration(batch, it)
            o_losses.append(dict(oracle.losses))
            if it == 0:
                o_grads = {k: v.clone() for k, v in oracle.last_gen_grads.items() if v is not None}
        torch.set_rng_state(rng)
        db = {k: v.to(DEV) for k, v in batch.items()}
        for it in range(2):
            a = (db["x_real"], db["c_src"], db["c_trg"], db["txt"], db["txt_lens"], db["label_src"], db["label_trg"], cfg, it)
            s.dis_update(*a)
            grabbed = {}
            real_step = s.gen_opt.step

            def grab(*aa, **kk):
                grabbed.update({n: p.grad.detach().clone() for n, p in s.gen.named_parameters() if p.grad is not None})
                return real_step(*aa, **kk)
            s.gen_opt.step = grab
            s.gen_update(*a)
            s.gen_opt.step = real_step
            s.smooth_moving()
            s.update_learning_rate()
            s.update_attention_status(it)
            for k, want in o_losses[it].items():
                got = float(torch.as_tensor(getattr(s, k)).detach())
                assert abs(got - want) <= 2e-4 * max(1.0, abs(want)), (it, k, got, want)
            if it == 0:
                for name in ("enc_style.fcs.0.weight", "enc_style.fcs.7.bias", "enc_txt.fcs.3.weight"):
                    close(grabbed[name], o_grads[name], rel=5e-3, msg=name)
        assert abs(o_losses[0]["loss_kl_x"]) > 1e-3          # the EM term is live
    finally:
        host.set_noise(host.DeviceNoise())


def test_tiny_dis_gradients_vs_reference(tiny, golden_dir):
    ref = np.load(os.path.join(golden_dir, "tiny_dis_grads.npz"))
    host.set_noise(host.HostNoise())
    try:
        s, cfg, batch = _tiny_solver(tiny)
        grabbed = {}
        real_step = s.dis_opt.step

        def grab(*a, **k):
            grabbed.update({n: p.grad.detach().clone() for n, p in s.dis.named_parameters()})
            return real_step(*a, **k)
        s.dis_opt.step = grab
        s.dis_update(batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"],
                     batch["label_src"], batch["label_trg"], cfg, 0)
        assert abs(float(s.loss_dis_all) - float(ref["loss_dis"])) < 2e-4
        for k, g in grabbed.items():
            close(g, T(ref[k]), rel=2e-3, msg=k)
    finally:
        host.set_noise(host.DeviceNoise())


def test_tiny_dis_penalties_vs_reference(tiny, golden_dir):
    """Solver.dis_update with the gradient penalty and the R1 penalty on (reference solver.py:291-315,337-350; r06 -- rounds 1-5 raised
    NotImplementedError): the HIP D step plus the two double-backward side branches on torch device ops, against the imported reference
    (gp_w = 10, use_r1 = True, iteration 15): scalars and every D gradient."""
    ref = np.load(os.path.join(golden_dir, "tiny_penalties.npz"))
    host.set_noise(host.HostNoise())
    try:
        s, cfg, batch = _tiny_solver(tiny)
        cfg = dict(cfg, gp_w=10.0, use_r1=True)
        grabbed = {}
        real_step = s.dis_opt.step

        def grab(*a, **k):
            grabbed.update({n: p.grad.detach().clone() for n, p in s.dis.named_parameters()})
            return real_step(*a, **k)
        s.dis_opt.step = grab
        s.dis_update(batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"],
                     batch["label_src"], batch["label_trg"], cfg, 15)
        for k in ("loss_dis", "loss_dis_all", "loss_gp", "loss_r1"):
            got, want = float(getattr(s, k)), float(ref[k])
            assert abs(got - want) <= 2e-4 * max(abs(want), 1e-12) + (2e-4 if k != "loss_r1" else 0.0), (k, got, want)
        for k, g in grabbed.items():
            close(g, T(ref["grad/" + k]), rel=2e-3, msg=k)
    finally:
        host.set_noise(host.DeviceNoise())


# ---- VGG16 perceptual loss (reference networks.py:639-688, solver.py:242-247) ----------
@pytest.mark.parametrize("B,C,H", [(2, 64, 16), (1, 8, 6), (3, 4, 10)])
def test_max_pool2_and_zeropad_conv(B, C, H):
    g = torch.Generator().manual_seed(B + C + H)
    x = torch.randn(B, C, H, H, generator=g)
    x[:, :, :2, :2] = 0.0                                  # a tied (all-zero) window: gradient goes to its first element
    w, b = torch.randn(16, C, 3, 3, generator=g) * 0.2, torch.randn(16, generator=g) * 0.1
    xr = x.clone().requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(torch.relu(torch.nn.functional.conv2d(xr, w, b, padding=1)), 2, 2)
    gy = torch.randn(yr.shape, generator=g)
    (yr * gy).sum().backward()
    xd = dev(x, True)
    yd = ops.max_pool2(ops.conv2d_zeropad(xd, dev(w), dev(b), 1, "relu"))
    close(yd, yr, msg="y")
    (yd * gy.to(DEV)).sum().backward()
    close(xd.grad, xr.grad, rel=5e-5, msg="dx")
    p = torch.randn(B, C, H, H, generator=g)
    pr = p.clone().requires_grad_(True)
    qr = torch.nn.functional.max_pool2d(pr, 2, 2)
    gq = torch.randn(qr.shape, generator=g)
    (qr * gq).sum().backward()
    pd = dev(p, True)
    qd = ops.max_pool2(pd)
    assert torch.equal(qd.cpu(), qr.detach())
    (qd * gq.to(DEV)).sum().backward()
    assert torch.equal(pd.grad.cpu(), pr.grad)


@pytest.mark.parametrize("tag", ["s32", "s64"])
def test_vgg_perceptual_loss_vs_reference(golden_dir, tag):
    """Solver.compute_vgg_loss on the seeded random Vgg16 against the values recorded from the reference."""
    from networks.networks import Vgg16
    from solver import Solver
    z = np.load(os.path.join(golden_dir, "vgg_loss.npz"))
    torch.manual_seed(777)
    vgg = Vgg16().to(DEV).eval()
    for prm in vgg.parameters():
        prm.requires_grad = False
    img, target = dev(torch.from_numpy(z[tag + "_img"])), dev(torch.from_numpy(z[tag + "_target"]), True)
    with torch.no_grad():
        from hipdwc.host import vgg_preprocess
        fea = vgg(vgg_preprocess(img))
    close(fea, torch.from_numpy(z[tag + "_fea"]), rel=2e-5, msg="relu5_3")
    loss = Solver.compute_vgg_loss(None, vgg, img, target)
    assert float(loss.detach()) == pytest.approx(float(z[tag + "_loss"]), rel=2e-3)
    loss.backward()
    close(target.grad, torch.from_numpy(z[tag + "_dtarget"]), rel=5e-3, atol=1e-9, msg="d loss / d target")


def test_iteration_with_vgg_loss_vs_oracle(tmp_path):
    """vgg_w > 0 (the shipped config's default): Solver loads <vgg_model_path>/models/vgg16.weight like the reference
    (utils.py:180-193, minus the download) and adds the perceptual term; one tiny-configuration iteration against
    the oracle, loss scalars and a generator gradient."""
    from networks.networks import Vgg16
    from solver import Solver
    torch.manual_seed(777)
    vgg_sd = Vgg16().state_dict()
    os.makedirs(tmp_path / "models")
    torch.save(vgg_sd, tmp_path / "models" / "vgg16.weight")
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    cfg["vgg_w"], cfg["vgg_model_path"] = 0.1, str(tmp_path)
    host.set_noise(host.HostNoise())
    try:
        torch.manual_seed(4321)
        s = Solver(cfg, torch.device(DEV), None).to(DEV)
        s.copy_nets()
        rng = torch.get_rng_state()
        batch = synth.make_batch(3, 32, seed=5)
        oracle = orc.OracleSolver(cfg, {k: v.cpu() for k, v in s.gen.state_dict().items()},
                                  {k: v.cpu() for k, v in s.dis.state_dict().items()}, vgg_params=vgg_sd)
        oracle.copy_nets()
        oracle.iteration(batch, 0)
        torch.set_rng_state(rng)
        db = {k: v.to(DEV) for k, v in batch.items()}
        a = (db["x_real"], db["c_src"], db["c_trg"], db["txt"], db["txt_lens"], db["label_src"], db["label_trg"], cfg, 0)
        s.dis_update(*a)
        s.gen_update(*a)
        assert oracle.losses["loss_gen_vgg"] > 0
        for k, want in oracle.losses.items():
            got = float(torch.as_tensor(getattr(s, k)).detach())
            assert abs(got - want) <= (2e-3 if k == "loss_gen_vgg" else 2e-4) * max(1.0, abs(want)), (k, got, want)
        name = "dec.model.2.conv.weight"
        close(dict(s.gen.named_parameters())[name].grad, oracle.last_gen_grads[name], rel=1e-2, msg=name)
    finally:
        host.set_noise(host.DeviceNoise())


@pytest.mark.parametrize("att", [True, False], ids=["attention", "no_attention"])
def test_sample_vs_reference(tiny, golden_dir, att):
    """Solver.sample (reference solver.py:249-289) against the stacks recorded from the reference on the tiny configuration:
    reconstruction, text-driven translation, resampled-style translation and (attention on) the attention maps."""
    ref = np.load(os.path.join(golden_dir, "sample_tiny.npz"))
    tag = "att" if att else "noatt"
    host.set_noise(host.HostNoise())
    try:
        s, cfg, batch = _tiny_solver(tiny)
        s.use_attention = att
        torch.manual_seed(555)
        res = s.sample(batch["x_real"], batch["txt"], batch["txt_lens"])
        assert len(res) == int(ref[tag + "/n"]) and s.training
        for i, r in enumerate(res):
            close(r, T(ref["%s/%d" % (tag, i)]), rel=2e-4, msg="%s output %d" % (tag, i))
    finally:
        host.set_noise(host.DeviceNoise())


def test_sample_matches_manual_path():
    """Solver.sample (reference solver.py:249-289, the image grid train.py writes): per-image encode / text-encode /
    decode in eval mode.  Shapes, value ranges, train-mode restoration, and the reconstruction column against the same
    calls made by hand."""
    from solver import Solver
    cfg = synth.make_config(image_size=32, tiny=True)
    torch.manual_seed(11)
    s = Solver(cfg, torch.device(DEV), None).to(DEV)
    batch = {k: v.to(DEV) for k, v in synth.make_batch(3, 32, seed=2).items()}
    host.set_noise(host.DeviceNoise())
    torch.manual_seed(5)
    out = s.sample(batch["x_real"], batch["txt"], batch["txt_lens"])
    assert s.training
    assert len(out) == (5 if s.use_attention else 4)
    for t in out:
        assert t.shape == batch["x_real"].shape and bool(torch.isfinite(t).all())
    assert torch.equal(out[0], batch["x_real"])
    assert float(out[1].abs().max()) <= 1.0 + 1e-6            # tanh image blended with a [-1,1] input stays in range
    s.eval()
    with torch.no_grad():
        x4 = ops.pack_image(batch["x_real"][1:2])
        content, style_real, _ = s.gen.encode(x4)
        rec = s._decode(content, torch.cat(style_real, dim=1), x4)[:, :3]
    s.train()
    close(out[1][1:2], rec, rel=1e-5, msg="reconstruction column")


def test_weight_refresh_multi_matches_single_layout_kernels():
    """after an optimiser step every prepared weight layout is rebuilt by ONE dwc_weight_refresh_multi
    launch.  Its output must equal, bit for bit, what the single-layout entry points build from the same weights: fp32 and
    bf16 im2col rows (forward, data gradient, transposed-filter data gradient, the four stride-2 parity classes), the
    three-plane bf16 splits and the two-plane f16 splits with their scales (r05)."""
    g = torch.Generator().manual_seed(9)
    cases = [  # (Cout, Cin, k, [(kind, cout_pad, cin_pad, stride, half)])
        (128, 64, 4, [("fwd", 128, 64, 2, False), ("dgrad", 128, 64, 2, False), ("fwd", 128, 64, 2, True), ("dgrad", 128, 64, 2, True)]),
        (256, 256, 3, [("fwd", 256, 256, 1, True), ("dgrad", 256, 256, 1, True), ("dgrad_t", 256, 256, 1, True), ("dgrad", 256, 256, 1, False),
                       ("dgrad_t", 256, 256, 1, False),
                       ("x3_fwd", 256, 256, 1, False), ("x3_dgrad", 256, 256, 1, False), ("h2_fwd", 256, 256, 1, False),
                       ("h2_dgrad", 256, 256, 1, False)]),
        (128, 256, 5, [("x3_fwd", 128, 256, 1, False), ("x3_dgrad", 128, 256, 1, False), ("fwd", 128, 256, 1, True), ("dgrad_t", 128, 256, 1, True),
                       ("h2_fwd", 128, 256, 1, False), ("h2_dgrad", 128, 256, 1, False)]),
        (61, 20, 3, [("fwd", 64, 20, 1, False), ("dgrad", 64, 20, 1, False), ("fwd", 64, 24, 1, True)]),      # padded rows / channels
        (8, 512, 4, [("fwd", 8, 512, 1, False), ("dgrad", 8, 512, 1, False)]),
    ]
    params = []
    for co, ci, k, layouts in cases:
        w = (torch.randn(co, ci, k, k, generator=g) * 0.1).to(DEV).requires_grad_(True)
        params.append((w, layouts))
        for kind, cop, cip, st, half in layouts:
            ops._prepped(w, kind, cop, cip, st, None, half)
    before = ops.REFRESH_STATS["launches"]
    with torch.no_grad():
        for w, _ in params:
            w.add_(torch.randn(w.shape, generator=g).to(DEV) * 0.05)          # in-place: bumps the version like an optimiser step
    n = ops.refresh_prepared([w for w, _ in params])
    assert n == sum(len(l) for _, l in params) and ops.REFRESH_STATS["launches"] == before + 1
    for w, layouts in params:
        for kind, cop, cip, st, half in layouts:
            got = ops._prepped(w, kind, cop, cip, st, None, half)              # cache hit: the refreshed tensor
            assert ops.refresh_prepared([w]) == 0
            ref_w = w.detach().clone().requires_grad_(True)                    # a fresh tensor: the single-layout kernels
            want = ops._prepped(ref_w, kind, cop, cip, st, None, half)
            assert got.data_ptr() != want.data_ptr()
            if kind.startswith("h2"):        # two f16 planes + {s_w, 1 / s_w}; the last 8 bytes are the refresh's own absmax slot
                got, want = got.view(torch.int16)[:-4], want.view(torch.int16)[:-4]
            assert torch.equal(got.view(torch.int16) if half or kind.startswith("x3") else got,
                               want.view(torch.int16) if half or kind.startswith("x3") else want), (kind, cop, cip, st, half)


@pytest.mark.parametrize("B,hw,segs", [(4, 4, 3), (16, 2, 2), (3, 1, 1), (48, 4, 3)])
def test_adv_tail_and_weighted_sum_vs_oracle(B, hw, segs):
    """One-launch adversarial tail of a discriminator scale (LSGAN + BCE-with-logits, reference networks.py:116-170) and the
    one-launch loss_gen_total sum (solver.py:226-238) against the oracle's term-by-term algebra, values and gradients."""
    g = torch.Generator().manual_seed(B * 10 + hw + segs)
    src = torch.randn(segs * B, 1, hw, hw, generator=g)
    cls = torch.randn(segs * B, 8, generator=g) * 2
    labels = (torch.rand(B, 8, generator=g) > 0.5).float()
    targets, w_src, w_cls = (0.0, 0.0, 1.0)[:segs], (1.0, 0.7, 2.0)[:segs], (0.0, 0.3, 2.0)[:segs]
    sr, cr = src.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    want = 0
    for s in range(segs):
        want = want + w_src[s] * ((sr[s * B:(s + 1) * B] - targets[s]) ** 2).mean() \
            + w_cls[s] * orc.bce_with_logits_mean(cr[s * B:(s + 1) * B], labels)
    (want * 1.7).backward()
    sd, cd = dev(src, True), dev(cls, True)
    got = ops.adv_tail(sd, cd, labels.to(DEV), B, targets, w_src, w_cls)
    assert abs(float(got) - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
    (got * 1.7).backward()
    close(sd.grad, sr.grad, rel=1e-5, msg="dsrc")
    close(cd.grad, cr.grad, rel=1e-5, msg="dcls")
    # weighted sum
    ts = [torch.randn((), generator=g) for _ in range(5)]
    ws = [1.0, 10.0, 0.1, -0.99999, 0.0]
    tr = [t.clone().requires_grad_(True) for t in ts]
    ref = sum(w * t for w, t in zip(ws, tr)) + 0.5 * 3.0
    ref.backward()
    td = [dev(t, True) for t in ts]
    out = ops.weighted_sum(list(zip(ws, td)) + [(0.5, 3.0), (0.1, 0)])
    assert abs(float(out) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    out.backward()
    for a, b in zip(td, tr):
        assert abs(float(a.grad) - float(b.grad)) <= 1e-7
