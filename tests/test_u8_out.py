"""The device half of the output pipeline (csrc/image_out_u8.hip, hipdwc.u8image.grid_u8 / image_to_u8, utils.write_grid,
Solver.forward(internal=True)): image batches -> the uint8 grid the reference's image writers save.

Reference: what the reference's ``__write_images`` (utils.py:69-73) computes through torchvision's ``make_grid(nrow, padding=0,
normalize=True)`` and ``save_image``, restated in plain torch ops on the CPU (``yardstick`` below; torchvision itself is not
installed).  Every comparison is ``torch.equal`` on the bytes: the chain is a fixed sequence of fp32 operations, each rounded on its
own, and the kernel repeats that sequence, so there is nothing to tolerate.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from hipdwc import _lib, ops, u8image

import guarded_alloc                            # noqa: E402  (tests/ is on the path: conftest)

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(4, 4), (3, 5), (8, 12), (16, 16)]      # (3, 5): the byte path; the others: four pixels per thread
NROWS = (1, 2, 3, 8)
BATCHES = (1, 2, 3, 5)
RANGES = (None, (-1.0, 1.0), (0.0, 1.0))
LAYOUTS = ("nchw1", "nchw3", "nhwc4", "nhwc8")
JUNK = 1.0e4                                     # what the planes that must not enter hold
_sid = lambda hw: "%dx%d" % hw


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def seen(x):
    """What the chain sees of a source: fp32 on the CPU, planes 0..2 of an internal image buffer."""
    return (x[:, :3] if ops.is_image(x) else x).float().cpu()


def yardstick(images, n, value_range=None, nrow=None):
    """The reference's chain on the CPU.  ``nrow`` apart from ``n`` only for image_to_u8 (all images, one column)."""
    nrow = n if nrow is None else nrow
    t = torch.cat([seen(x).expand(-1, 3, -1, -1)[:n] for x in images]).clone()
    lo, hi = (float(t.min()), float(t.max())) if value_range is None else value_range
    t.clamp_(lo, hi).sub_(lo).div_(max(hi - lo, 1e-5))
    N, _, H, W = t.shape
    cols = min(nrow, N)
    rows = int(math.ceil(N / cols))
    grid = torch.zeros(3, rows * H, cols * W)
    for j in range(N):
        r, c = j // cols, j % cols
        grid[:, r * H:(r + 1) * H, c * W:(c + 1) * W] = t[j]
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)


def noise(B, hw, seed, scale=0.8):
    """Normal noise that leaves (-1, 1) and (0, 1) on both sides.  fp32 [B, 3, H, W] on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 31 * hw[0] + hw[1] + 7 * B)
    return torch.randn(B, 3, hw[0], hw[1], generator=g) * scale


def as_layout(base, layout, device=DEV):
    """``base`` (fp32 [B, 3, H, W], CPU) as a source of ``layout`` on ``device``.  The planes of an internal buffer that are not
    the image hold +-JUNK, far outside every image's values: whatever reads them moves the range."""
    B, _, H, W = base.shape
    if layout == "nchw3":
        return base.to(device)
    if layout == "nchw1":
        return base[:, :1].contiguous().to(device)
    planes, dtype = (4, torch.float32) if layout == "nhwc4" else (8, torch.bfloat16)
    junk = torch.full((B, planes - 3, H, W), JUNK)
    junk[:, :, ::2] = -JUNK
    buf = torch.cat([base, junk], 1).to(dtype).contiguous(memory_format=torch.channels_last).to(device)
    assert ops.is_image(buf)
    return buf


def check(images, n, value_range=None, what=""):
    got = u8image.grid_u8(images, n, value_range)
    want = yardstick(images, n, value_range)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    differing = int((got.cpu() != want).sum())
    assert differing == 0, "%s: %d of %d bytes differ" % (what, differing, want.numel())
    assert torch.equal(got.cpu(), want)
    return got


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("dwc_image_out_ws_bytes", "dwc_image_out_grid_u8")


def test_abi_declares_the_output_symbols_at_version_11():
    header = open(os.path.join(os.path.dirname(HERE), "include", "dwcgan_hip.h")).read()
    for name in NEW_SYMBOLS:
        protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert len(protos) == 1, name
        assert len(protos[0].split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+DWC_ABI_VERSION\s+11\b", header)
    assert _lib.ABI_VERSION == 11 and _lib.load().dwc_version() == 11
    assert int(re.search(r"#define\s+DWC_IMAGE_OUT_MAX_SOURCES\s+(\d+)", header).group(1)) == _lib.IMAGE_OUT_MAX_SOURCES >= 8
    for name, code in (("NCHW1", "nchw1"), ("NCHW3", "nchw3"), ("NHWC4", "nhwc4"), ("NHWC8_BF16", "nhwc8_bf16")):
        assert int(re.search(r"#define\s+DWC_IMAGE_OUT_%s\s+(\d+)" % name, header).group(1)) == _lib.IMAGE_OUT_LAYOUTS[code]
    assert not hasattr(ops, "grid_u8") and not hasattr(ops, "image_to_u8")     # one home: hipdwc.u8image


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_output_entry_points_refuse_before_any_launch():
    """No device is touched: the pointers are dummies, so every call must return from the host-side checks."""
    lib = _lib.load()
    p = 4096
    big = 1 << 30
    rng = (ctypes.c_double * 2)(-1.0, 1.0)
    EWORKSPACE = -2

    def call(layouts, batches, useds, H, W, nrow, K=None, src=p, out=p, value_range=rng, ws=p, nbytes=big, arrays=(True, True, True)):
        K = len(layouts) if K is None else K
        srcs = None if src is None else (ctypes.c_void_p * max(len(layouts), 1))(*([src] * len(layouts)))
        lay, bat, use = (_ints(*v) if keep else None for v, keep in zip((layouts, batches, useds), arrays))
        rc = lib.dwc_image_out_grid_u8(srcs, lay, bat, use, K, H, W, nrow, value_range, out, ws, nbytes, None)
        # every call of this test must fail a host-side check: one that passes them all would launch on the dummy pointers (where
        # there is no device that shows as DWC_ELAUNCH, -3; where there is one it is a wild access)
        assert rc in (_lib.EINVAL, EWORKSPACE), (rc, layouts, batches, useds, H, W, nrow, K)
        need = lib.dwc_image_out_ws_bytes(lay, bat, use, K, H, W, nrow, int(value_range is None))
        return rc, need

    good = ((1, 2), (4, 4), (3, 4), 8, 12, 3)
    refused = [
        ((), (), (), 8, 12, 3),                                              # K = 0
        ((1,) * 9, (2,) * 9, (2,) * 9, 8, 12, 3),                            # more sources than the table holds
        ((1, 2), (4, 4), (0, 4), 8, 12, 3), ((1, 2), (4, 4), (3, -1), 8, 12, 3),      # a non-positive count
        ((1, 2), (0, 4), (3, 4), 8, 12, 3), ((1, 2), (4, -2), (3, 4), 8, 12, 3),      # a non-positive batch
        ((1, 2), (4, 4), (3, 4), 0, 12, 3), ((1, 2), (4, 4), (3, 4), 8, -3, 3),       # a non-positive size
        ((1, 2), (4, 4), (3, 4), 8, 12, 0), ((1, 2), (4, 4), (3, 4), 8, 12, -1),      # nrow
        ((1, 4), (4, 4), (3, 4), 8, 12, 3), ((-1, 2), (4, 4), (3, 4), 8, 12, 3),      # an unknown layout
        ((1, 2), (4, 4), (5, 4), 8, 12, 3),                                  # more images used than the buffer holds
        ((1, 2), (4, 4), (3, 4), 16385, 12, 3), ((1, 2), (4, 4), (3, 4), 8, 16385, 3),   # over-large extents
        ((1, 2), (65536, 4), (3, 4), 8, 12, 3),
    ]
    for shape in refused:
        for vr in (rng, None):
            assert call(*shape, value_range=vr) == (_lib.EINVAL, 0), shape
    assert call(*good, K=0)[0] == _lib.EINVAL and call(*good, K=-1) == (_lib.EINVAL, 0) and call(*good, K=9) == (_lib.EINVAL, 0)
    # a missing pointer: the table, one entry of it, the output, each descriptor array
    assert call(*good, src=None)[0] == _lib.EINVAL
    assert call(*good, src=0)[0] == _lib.EINVAL
    assert call(*good, out=None)[0] == _lib.EINVAL
    for k in range(3):
        assert call(*good, arrays=tuple(i != k for i in range(3))) == (_lib.EINVAL, 0), k
    # a pointer the loads cannot take: internal buffers move as 16-byte pixels, dense ones as floats
    assert call((2,), (4,), (4,), 8, 12, 3, src=p + 4)[0] == _lib.EINVAL
    assert call((3,), (4,), (4,), 8, 12, 3, src=p + 8)[0] == _lib.EINVAL
    assert call((1,), (4,), (4,), 8, 12, 3, src=p + 2)[0] == _lib.EINVAL
    # scratch: none with a value_range; without one, a (min, max) pair of floats per workgroup of the first launch
    assert lib.dwc_image_out_ws_bytes(_ints(*good[0]), _ints(*good[1]), _ints(*good[2]), 2, *good[3:], 0) == 0      # (the query alone)
    for shape in (good, ((0,), (1,), (1,), 1, 1, 1), ((1,) * 5, (8,) * 5, (8,) * 5, 128, 128, 8)):
        need = lib.dwc_image_out_ws_bytes(_ints(*shape[0]), _ints(*shape[1]), _ints(*shape[2]), len(shape[0]), *shape[3:], 1)
        assert 8 <= need <= 8 * 256 and need % 8 == 0, shape
        assert call(*shape, value_range=None, nbytes=need - 1) == (EWORKSPACE, need), shape
        assert call(*shape, value_range=None, ws=None, nbytes=need) == (EWORKSPACE, need), shape
    # the reference's grid fills the first launch: 5 x 8 x 3 x 128 x 128 floats are 480 workgroups' worth, capped
    assert lib.dwc_image_out_ws_bytes(_ints(*(1,) * 5), _ints(*(8,) * 5), _ints(*(8,) * 5), 5, 128, 128, 8, 1) == 8 * 256


def test_grid_u8_refuses_malformed_input():
    good = torch.zeros(2, 3, 8, 12)
    for fn in (lambda x: u8image.grid_u8(x, 2), lambda x: u8image.grid_u8([x], 2, (-1, 1)), u8image.image_to_u8):
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fn(good)
        with pytest.raises(RuntimeError, match="CPU tensor"):
            fn(torch.zeros(2, 4, 8, 12).contiguous(memory_format=torch.channels_last))     # an internal buffer, on the CPU
        with pytest.raises(TypeError):
            fn(good.double())
        with pytest.raises(TypeError):
            fn(good.to(torch.uint8))
        with pytest.raises(TypeError):
            fn(good.bfloat16())                                                # bf16 only as an internal buffer
        with pytest.raises(TypeError):
            fn(good.numpy())
        with pytest.raises(ValueError):
            fn(good[0])                                                        # rank 3
        with pytest.raises(ValueError):
            fn(good.unsqueeze(0))
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 2, 8, 12))
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 4, 8, 12))                                       # four planes, but not channels-last
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 5, 8, 12))
        with pytest.raises(ValueError):
            fn(torch.zeros(0, 3, 8, 12))
    with pytest.raises(ValueError, match="size"):
        u8image.grid_u8([good, torch.zeros(2, 3, 8, 8)], 2)
    with pytest.raises(ValueError, match="size"):
        u8image.grid_u8([good, torch.zeros(2, 1, 12, 8)], 2)
    for nrow in (0, -1):
        with pytest.raises(ValueError, match="nrow"):
            u8image.grid_u8([good], nrow)
    with pytest.raises(ValueError, match="sources"):
        u8image.grid_u8([good] * (_lib.IMAGE_OUT_MAX_SOURCES + 1), 2)
    with pytest.raises(ValueError, match="sources"):
        u8image.grid_u8([], 2)


def test_yardstick_tiles_as_make_grid_does():
    """The tiling rule of the yardstick itself, on values the conversion maps to themselves: image j of N lands in row j // cols,
    column j % cols with cols = min(nrow, N), and the cells past the last image are 0."""
    imgs = [torch.full((3, 3, 2, 2), float(10 * k)).add_(torch.arange(3.0).view(3, 1, 1, 1)) for k in range(1, 3)]     # 10 11 12, 20 21 22
    got = yardstick(imgs, 2, value_range=(0.0, 255.0))                          # two of each: 10 11 / 20 21
    assert tuple(got.shape) == (4, 4, 3) and got[:2, :2].eq(10).all() and got[:2, 2:].eq(11).all() and got[2:, :2].eq(20).all()
    got = yardstick(imgs, 3, value_range=(0.0, 255.0), nrow=4)                  # six images in rows of four: two empty cells
    assert tuple(got.shape) == (4, 8, 3) and got[2:, :2].eq(21).all() and got[2:, 2:4].eq(22).all() and not got[2:, 4:].any()


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def precision(request):
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision("fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SIZES, ids=_sid)
def test_grid_u8_is_byte_equal_to_the_yardstick(hw, layout):
    """Each layout alone: every nrow x batch (n < B, n == B, n > B) x value_range, on noise that leaves the fixed ranges."""
    for B in BATCHES:
        x = as_layout(noise(B, hw, seed=1), layout)
        for n in NROWS:
            for vr in RANGES:
                check([x], n, vr, "%s B %d n %d range %s" % (layout, B, n, vr))
    assert torch.equal(u8image.grid_u8(x, 2), u8image.grid_u8([x], 2))           # a bare tensor is a list of one
    if layout.startswith("nchw"):
        # dense memory that starts 4 bytes past a 16-byte boundary (a slice of a larger tensor): rows move float by float
        flat = torch.empty(x.numel() + 1, device=DEV)
        shifted = flat[1:].view(x.shape).copy_(x)
        assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
        for vr in RANGES:
            assert torch.equal(u8image.grid_u8([x, shifted], 3, vr), u8image.grid_u8([x, x], 3, vr))
            check([shifted], 5, vr, "%s, shifted" % layout)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(16, 16), (3, 5), (128, 128)], ids=_sid)
def test_grid_u8_on_the_reference_list(hw):
    """What Solver.sample returns with attention on: four 3-channel tensors and a one-channel map expanded to three."""
    B = 8
    outs = [noise(B, hw, seed=k).to(DEV) for k in range(4)]
    att = (torch.sigmoid(noise(B, hw, seed=9)[:, :1]).to(DEV).expand(-1, 3, -1, -1) - 0.5) / 0.5
    att_view = att[:, :1].expand(-1, 3, -1, -1)                                  # the same, as a stride-0 view
    assert not att_view.is_contiguous()
    for vr in RANGES:
        got = check(outs + [att], B, vr, "five dense, range %s" % (vr,))
        assert tuple(got.shape) == (5 * hw[0], B * hw[1], 3)
        assert torch.equal(u8image.grid_u8(outs + [att_view], B, vr), got)
    if hw[0] < 128:
        for n in (3, 11):
            check(outs + [att_view], n, None, "five, n %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("B,hw,n,vr", [(9, (512, 512), 3, None), (1, (725, 725), 1, (0.0, 1.0))], ids=["quads", "bytes"])
def test_grid_u8_beyond_one_pass_of_the_map_grid(B, hw, n, vr):
    """More work than the map launch's 2 048 workgroups of 256 threads take in one pass (524 288 quads or pixels): its grid-stride
    loop goes round again.  One-plane sources keep the case small; ``n < B`` leaves images unused behind the used ones."""
    x = as_layout(noise(B, hw, seed=8), "nchw1")
    srcs = [x, x, x] if vr is None else [x]
    assert len(srcs) * min(n, B) * hw[0] * hw[1] // (4 if hw[1] % 4 == 0 else 1) > 2048 * 256
    check(srcs, n, vr, "large")


@pytest.mark.gpu
@pytest.mark.parametrize("hw", SIZES, ids=_sid)
@pytest.mark.parametrize("precision", ["fp32", "bf16"], indirect=True)
def test_grid_u8_on_mixed_and_ragged_sources(precision, hw):
    """NCHW of both channel counts, NHWC4 and (whatever the active precision) NHWC8 in one list, with different batches: the last
    row has empty cells.  The internal buffer of the ACTIVE precision comes from ops.pack_image."""
    packed = ops.pack_image(noise(2, hw, seed=5).to(DEV))
    assert ops.is_image(packed) and packed.dtype == ops.act_dtype()
    packed[:, 3:] = JUNK                                                         # padding planes: must not enter
    srcs = [as_layout(noise(3, hw, seed=1), "nchw3"), as_layout(noise(2, hw, seed=2), "nhwc4"), packed,
            as_layout(noise(1, hw, seed=3), "nchw1"), as_layout(noise(5, hw, seed=4), "nhwc8")]
    for n in (1, 2, 3, 8):
        for vr in RANGES:
            got = check(srcs, n, vr, "mixed n %d range %s" % (n, vr))
    N = 3 + 2 + 2 + 1 + 5                                                        # n = 8 takes every image: 13 in rows of 8
    assert tuple(got.shape) == (2 * hw[0], 8 * hw[1], 3) and not got[hw[0]:, (N - 8) * hw[1]:].any()
    got = check(srcs[:3], 3, None, "ragged")                                     # 3 + 2 + 2 = 7 in rows of 3: two empty cells
    assert tuple(got.shape) == (3 * hw[0], 3 * hw[1], 3) and not got[2 * hw[0]:, hw[1]:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SIZES, ids=_sid)
def test_grid_u8_range_comes_from_exactly_what_enters(hw, layout):
    """value_range None.  A constant image (hi == lo: the 1e-5 divisor); the extremes in the very last used value and in the very
    first; larger extremes in an unused image (and, through as_layout, always in the planes that are not the image)."""
    B, n = 3, 2
    const = torch.full((B, 3, hw[0], hw[1]), 0.25)
    got = check([as_layout(const, layout)], n, None, "constant")
    assert not got.any()                                                         # (x - lo) / 1e-5 = 0 everywhere
    check([as_layout(const, layout)], n, (0.0, 1.0), "constant, fixed range")
    base = noise(B, hw, seed=3, scale=0.3)
    last = base.clone()
    last[n - 1, -1, -1, -1], last[n - 1, 0, -1, -1] = 50.0, -60.0                # the last used pixel of the last used image
    if layout == "nchw1":
        last[n - 1, 0, -1, -2] = 50.0                                            # (one plane: its last two values)
    first = base.clone()
    first[0, 0, 0, 0], first[0, -1, 0, 1 % hw[1]] = 40.0, -30.0
    unused = base.clone()
    unused[n:] = 1.0e3
    unused[n:, :, ::2] = -1.0e3
    for name, t in (("last", last), ("first", first), ("unused", unused)):
        x = as_layout(t, layout)
        got = check([as_layout(base, "nchw3"), x], n, None, name)                # as the last source, behind another one
        check([x], n, None, name + ", alone")
        if name != "unused":
            assert int(got.max()) == 255 and int(got.min()) == 0
    # the unused images moved nothing: the same bytes as without them
    assert torch.equal(u8image.grid_u8([as_layout(unused, layout)], n), u8image.grid_u8([as_layout(base[:n], layout)], n))


def boundary_ramp(hw):
    """fp32 [B, 3, H, W] holding, for every k < 255, the fp32 nearest (k + 0.5) / 255 and its two neighbours: under range (0, 1) a
    value on one side of the boundary becomes byte k, on the other k + 1, so the byte turns on the last bit of every intermediate
    result (stretched to a range whose width is no power of two, a multiplication by the reciprocal puts some on the wrong side)."""
    mid = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    mid = mid.astype(np.float32)
    vals = np.stack([np.nextafter(mid, np.float32(-1)), mid, np.nextafter(mid, np.float32(2))], 1).reshape(-1)
    per = 3 * hw[0] * hw[1]
    B = -(-vals.size // per)
    return torch.from_numpy(np.resize(vals, B * per).reshape(B, 3, hw[0], hw[1]).copy())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["nchw1", "nchw3", "nhwc4"])
@pytest.mark.parametrize("hw", [(16, 16), (3, 5)], ids=_sid)
def test_grid_u8_at_the_rounding_boundaries(hw, layout):
    ramp = boundary_ramp(hw)
    B = ramp.shape[0]
    for n in (B, 8):
        check([as_layout(ramp, layout)], n, (0.0, 1.0), "ramp")
    # the same values under a range whose width is no power of two: the division must be a true one.  (These values do tell: a
    # multiplication by the fp32 reciprocal of the width gives other bytes.)
    stretched = ramp * 2.2 - 0.9
    shifted = stretched.clone().clamp_(-0.9, 1.3).sub_(-0.9)
    width = torch.tensor(1.3 - -0.9, dtype=torch.float32)
    to_bytes = lambda v: v.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
    assert int((to_bytes(shifted / width) != to_bytes(shifted * (1.0 / width))).sum()) > 0
    check([as_layout(stretched, layout)], B, None, "stretched ramp")
    check([as_layout(stretched, layout)], B, (-0.9, 1.3), "stretched ramp, fixed range")


def _two_poisons(monkeypatch):
    """0xFF, then 0x00: an output byte that equals the yardstick under both was written."""
    yield guarded_alloc.POISON_BYTE
    monkeypatch.setattr(guarded_alloc, "POISON_BYTE", 0x00)
    yield 0x00


@pytest.mark.gpu
@pytest.mark.parametrize("ranged", [False, True], ids=["from-data", "fixed-range"])
@pytest.mark.parametrize("hw", [(3, 5), (8, 12)], ids=_sid)
@pytest.mark.parametrize("precision", ["fp32", "bf16"], indirect=True)
def test_grid_u8_under_guarded_buffers(precision, hw, ranged, monkeypatch):
    """Sources, output and scratch between guard zones, output and scratch poisoned: no guard byte changes, every output byte is
    written (the result equals the yardstick from an all-ones and from an all-zeros output), and a read past a source would bring
    a NaN into the range."""
    alloc = guarded_alloc.GuardedAllocator()
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(u8image, "torch", guarded_alloc.TorchProxy(alloc))
    vr = (-1.0, 1.0) if ranged else None
    internal = "nhwc8" if precision == "bf16" else "nhwc4"
    plain = [as_layout(noise(3, hw, seed=1), internal), as_layout(noise(2, hw, seed=2), internal if precision == "bf16" else "nchw3"),
             as_layout(noise(3, hw, seed=3), "nchw1" if precision == "fp32" else internal)]
    want = yardstick(plain, 3, vr)
    for poison in _two_poisons(monkeypatch):
        srcs = [alloc.guarded_input(x, DEV, channels_last=ops.is_image(x)) for x in plain]
        assert all(ops.is_image(s) == ops.is_image(x) and s.is_contiguous() == x.is_contiguous() for s, x in zip(srcs, plain))
        before = dict(alloc.handed)
        got = u8image.grid_u8(srcs, 3, vr)
        alloc.verify()
        assert alloc.handed.get("workspace", 0) == before.get("workspace", 0) + (0 if ranged else 1), poison
        assert alloc.handed.get("torch.empty", 0) == before.get("torch.empty", 0) + 1, poison
        assert torch.equal(got.cpu(), want), poison


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(3, 5), (8, 12)], ids=_sid)
def test_image_to_u8(hw, layout):
    for B in (1, 3):
        x = as_layout(noise(B, hw, seed=6), layout)
        got = u8image.image_to_u8(x)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (B, hw[0], hw[1], 3) and got.is_contiguous()
        want = yardstick([x], B, (-1.0, 1.0), nrow=1)
        assert torch.equal(got.cpu().reshape(want.shape), want)
        # the same kernel: a one-column grid of the images, one source each
        assert torch.equal(u8image.grid_u8([x[i:i + 1] for i in range(B)], 1, (-1.0, 1.0)).reshape(got.shape), got)
        # and per image the plain expression ((x + 1) / 2 * 255 + 0.5, truncated)
        per_image = seen(x).expand(-1, 3, -1, -1).clamp(-1, 1).sub(-1.0).div(2.0).mul(255).add(0.5).clamp(0, 255).permute(0, 2, 3, 1)
        assert torch.equal(got.cpu(), per_image.to(torch.uint8))
        assert torch.equal(u8image.image_to_u8(x, (0.0, 1.0)).cpu().reshape(-1, hw[1], 3), yardstick([x], B, (0.0, 1.0), nrow=1))
    one = as_layout(noise(1, hw, seed=6), layout)
    assert torch.equal(u8image.image_to_u8(one), u8image.grid_u8([one], 1, (-1, 1)).reshape(1, hw[0], hw[1], 3))


def _tiny_solver(image_size=32):
    from hipdwc import host, synth
    import tiny_solver
    cfg = synth.make_config(image_size=image_size, tiny=True, lstm_dropout=0.0)
    assert cfg["gen"]["use_attention"]
    host.set_noise(host.DeviceNoise())
    s = tiny_solver.build(cfg, DEV)
    batch = synth.make_batch(4, image_size, seed=7, device=DEV)
    return s, batch


@pytest.mark.gpu
def test_sample_grids_reach_files(tmp_path):
    import utils
    s, batch = _tiny_solver()
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    outputs = s.sample(batch["x_real"], batch["txt"], batch["txt_lens"])
    assert len(outputs) == 5 and all(tuple(o.shape) == (4, 3, 32, 32) for o in outputs)
    for n in (3, 4):
        path = str(tmp_path / ("g%d.png" % n))
        utils.write_grid(outputs, n, path)
        back = torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy())
        assert torch.equal(back, yardstick(outputs, n))
    n = 3
    utils.write_2images_single(outputs, n, str(tmp_path), "test_%08d" % 7)
    with Image.open(str(tmp_path / "gen_a2b_test_00000007.jpg")) as im:
        assert im.format == "JPEG" and im.size == (n * 32, 5 * 32)
    utils.write_2images(outputs[:4], n, str(tmp_path), "train_current")
    for side in ("a2b", "b2a"):
        with Image.open(str(tmp_path / ("gen_%s_train_current.jpg" % side))) as im:
            assert im.size == (n * 32, 2 * 32)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"], indirect=True)
def test_forward_internal_goes_to_bytes(precision):
    """uint8 -> image_from_u8 -> forward(txt_group=1, internal=True) -> image_to_u8 -> uint8, with no fp32 NCHW image in between."""
    s, batch = _tiny_solver()
    s.eval()
    g = torch.Generator().manual_seed(3)
    crops = torch.randint(0, 256, (4, 40, 40, 3), generator=g, dtype=torch.uint8).to(DEV)
    with torch.no_grad():
        x = u8image.image_from_u8(crops, 32)
        buf = s.forward(x, batch["txt"], batch["txt_lens"], txt_group=1, internal=True)
        assert ops.is_image(buf) and buf.dtype == ops.act_dtype() and tuple(buf.shape) == (4, ops.image_planes(), 32, 32)
        got = u8image.image_to_u8(buf)
        assert tuple(got.shape) == (4, 32, 32, 3)
        assert torch.equal(got.cpu().reshape(-1, 32, 3), yardstick([buf[:, :3].float()], 4, (-1.0, 1.0), nrow=1))
        plain = s.forward(x, batch["txt"], batch["txt_lens"], txt_group=1)
        assert plain.dtype == torch.float32 and tuple(plain.shape) == (4, 3, 32, 32) and not ops.is_image(plain)
        if precision == "fp32":
            assert torch.equal(got.cpu().reshape(-1, 32, 3), yardstick([plain], 4, (-1.0, 1.0), nrow=1))
