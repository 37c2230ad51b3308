"""The loader's resize / to-float / normalise steps on the device: uint8 HWC crops -> internal image buffer in one HIP launch
(csrc/image_u8.hip).  ``data_loader.get_loader(..., device_transform=True)`` delivers the crops.

The result is bit-equal to the CPU chain followed by ``ops.pack_image``: PIL's ``BILINEAR`` resize of an 8-bit image is integer
arithmetic on windows of 22-bit fixed-point coefficients (``resample_table`` builds them in float64 on the host, by the rule of
Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc``), and the normalised value of each of the 256 possible bytes is taken
from a table computed with ``ImageTransform``'s own expression.

The way out is here too: ``grid_u8`` and ``image_to_u8`` turn image batches (fp32 NCHW or internal buffers of either precision) into
the bytes of the reference's sample grids, in one or two HIP launches (csrc/image_out_u8.hip), byte-equal to
torchvision's ``make_grid(normalize=True)`` + ``save_image`` arithmetic on the CPU.  ``utils.write_grid`` writes them to a file.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, ops

PRECISION_BITS = 22          # Pillow's 32 - 8 - 2: coefficients are rounded to this many fractional bits


def resample_table(n_in, n_out):
    """Windows of PIL's antialiased bilinear resize from ``n_in`` to ``n_out`` samples along one axis:
    ``(start[int32, n_out], coef[int32, n_out, ksize])``; output sample i is
    ``clip(((1 << 21) + sum_k v[start[i] + k] * coef[i, k]) >> 22, 0, 255)``, taps past the end of the axis having coefficient 0."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resample_table needs positive sizes")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs                                                  # the triangle filter's support (1.0) times the filter scale
    ksize = 2 * int(math.ceil(support)) + 1
    start = np.zeros(n_out, dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - support + 0.5), 0)
        hi = min(int(c + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((x + lo - c + 0.5) / fs)) for x in range(hi - lo)]
        total = sum(w)                                            # (left to right, as Pillow accumulates it)
        start[i] = lo
        coef[i, :hi - lo] = [int(0.5 + (v / total if total != 0.0 else v) * (1 << PRECISION_BITS)) for v in w]
    return start, coef


def value_table():
    """fp32 value of every byte, by the very expression ``data_loader.ImageTransform`` applies to a decoded image."""
    return torch.arange(256, dtype=torch.uint8).float().div_(255.0).sub_(0.5).div_(0.5)


_TABLES = {}                 # (n_in, n_out, device) -> (start, coef) on the device
_VALUES = {}                 # device -> value_table() on the device


def _key(device):
    return (device.type, ops._dev_index(device))


def _device_table(n_in, n_out, device):
    key = (n_in, n_out) + _key(device)
    tab = _TABLES.get(key)
    if tab is None:
        start, coef = resample_table(n_in, n_out)
        if coef.shape[1] != _lib.load().dwc_image_u8_ksize(n_in, n_out):      # the kernel derives the row pitch from the sizes
            raise _lib.HipKernelError("resample_table(%d, %d): window width %d is not the library's" % (n_in, n_out, coef.shape[1]))
        tab = _TABLES[key] = (torch.from_numpy(start).to(device), torch.from_numpy(coef).to(device))
    return tab


def _device_values(device):
    key = _key(device)
    lut = _VALUES.get(key)
    if lut is None:
        lut = _VALUES[key] = value_table().to(device)
    return lut


def image_from_u8(u8, size):
    """``u8``: contiguous device uint8 ``[B, H, W, 3]`` (the flipped, centre-cropped images).  ``size``: int or ``(h, w)``.  Returns
    what ``ops.pack_image`` returns for the CPU chain's batch: the internal image buffer of the active precision, NHWC4 fp32 or
    NHWC8 bf16, channels-last, padding planes zero."""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8:
        raise TypeError("image_from_u8 takes a uint8 tensor")
    if u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError("image_from_u8 takes [B, H, W, 3] (HWC) images, got %s" % (tuple(u8.shape),))
    if not u8.is_contiguous():
        raise ValueError("image_from_u8 takes a contiguous [B, H, W, 3] tensor")
    ops._require_device(u8)
    hout, wout = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    B, H, W, C = u8.shape
    lib = _lib.load()
    half = ops.PRECISION == "bf16"
    name = "dwc_bf16_image_u8_to_nhwc8" if half else "dwc_image_u8_to_nhwc4"
    if hout < 1 or wout < 1 or lib.dwc_image_u8_ksize(H, hout) == 0 or lib.dwc_image_u8_ksize(W, wout) == 0:
        _lib.check(_lib.EINVAL, name)
    ystart, ycoef = _device_table(H, hout, u8.device)
    xstart, xcoef = _device_table(W, wout, u8.device)
    lut = _device_values(u8.device)
    y = ops.empty_cl(B, ops.image_planes(), hout, wout, u8.device, ops.act_dtype())
    ws = ops.workspace(lib.dwc_image_u8_ws_bytes(B, H, W, C, hout, wout), u8.device)
    _lib.check(getattr(lib, name)(u8.data_ptr(), xstart.data_ptr(), xcoef.data_ptr(), ystart.data_ptr(), ycoef.data_ptr(),
                                  lut.data_ptr(), y.data_ptr(), B, H, W, C, hout, wout, ws.data_ptr(), ws.numel(), ops._stream()), name)
    return y


# ---- the way out: image batches -> uint8 (csrc/image_out_u8.hip) ---------------------------------------------------------

def _source(x):
    """(tensor whose memory the kernel reads, layout code) of one entry of ``images``; no device is touched."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("grid_u8 takes tensors, got %s" % type(x).__name__)
    if x.dtype not in (torch.float32, ops.BF16):
        raise TypeError("grid_u8 takes fp32 images or internal image buffers (fp32 / bf16), got %s" % x.dtype)
    if x.dim() != 4:
        raise ValueError("grid_u8 takes [B, C, H, W] images, got %s" % (tuple(x.shape),))
    if min(x.shape) < 1:
        raise ValueError("grid_u8 takes non-empty images, got %s" % (tuple(x.shape),))
    if ops.is_image(x):
        return x, _lib.IMAGE_OUT_LAYOUTS["nhwc8_bf16" if x.dtype == ops.BF16 else "nhwc4"]
    if x.dtype != torch.float32:
        raise TypeError("a bf16 source of grid_u8 must be an internal image buffer (NHWC8)")
    if x.shape[1] not in (1, 3):
        raise ValueError("grid_u8 takes images of 1 or 3 channels (or internal image buffers), got %s" % (tuple(x.shape),))
    if x.shape[1] == 3 and x.stride(1) == 0:
        x = x[:, :1]                                              # a one-channel image expanded to three: read the one plane
    return x, _lib.IMAGE_OUT_LAYOUTS["nchw1" if x.shape[1] == 1 else "nchw3"]


def _grid_u8(images, count, nrow, value_range):
    """``grid_u8`` with the number of images taken from every source (``count``) apart from the number of columns."""
    if isinstance(images, torch.Tensor):
        images = [images]
    images = list(images)
    nrow = int(nrow)
    if nrow < 1 or count < 1:
        raise ValueError("grid_u8 needs nrow >= 1")
    if not images:
        raise ValueError("grid_u8 got no sources")
    if len(images) > _lib.IMAGE_OUT_MAX_SOURCES:
        raise ValueError("grid_u8 takes at most %d sources, got %d" % (_lib.IMAGE_OUT_MAX_SOURCES, len(images)))
    sources = [_source(x) for x in images]
    H, W = sources[0][0].shape[2:]
    for x, _ in sources:
        if tuple(x.shape[2:]) != (H, W):
            raise ValueError("grid_u8 sources differ in size: %s and %s" % ((H, W), tuple(x.shape[2:])))
    if value_range is not None:
        lo, hi = value_range
        value_range = (ctypes.c_double * 2)(float(lo), float(hi))
    for x, _ in sources:
        ops._require_device(x)
    device = sources[0][0].device
    if any(x.device != device for x, _ in sources):               # (the output, the scratch and the stream are one device's)
        raise ValueError("grid_u8 sources are on different devices: %s" % sorted({str(x.device) for x, _ in sources}))
    K = len(sources)
    used = [min(count, x.shape[0]) for x, _ in sources]
    # dense sources: the used images as dense fp32 memory (internal buffers are dense by what makes them one)
    held = [x.detach() if code >= _lib.IMAGE_OUT_LAYOUTS["nhwc4"] else x.detach()[:n].contiguous() for (x, code), n in zip(sources, used)]
    src = (_lib.c_fp * K)(*[x.data_ptr() for x in held])
    layout = (_lib.c_int * K)(*[code for _, code in sources])
    batch = (_lib.c_int * K)(*[x.shape[0] for x in held])
    used = (_lib.c_int * K)(*used)
    N = sum(used)
    cols = min(nrow, N)
    rows = -(-N // cols)
    lib = _lib.load()
    name = "dwc_image_out_grid_u8"
    need = lib.dwc_image_out_ws_bytes(layout, batch, used, K, H, W, nrow, int(value_range is None))
    out = torch.empty((rows * H, cols * W, 3), dtype=torch.uint8, device=device)
    ws = ops.workspace(need, device) if need else None
    _lib.check(lib.dwc_image_out_grid_u8(src, layout, batch, used, K, H, W, nrow, value_range, out.data_ptr(),
                                         None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), ops._stream()), name)
    return out


def grid_u8(images, nrow, value_range=None):
    """The reference's sample grid as bytes: what ``make_grid(cat([x.expand(-1, 3, -1, -1)[:nrow] for x in images]), nrow=nrow,
    padding=0, normalize=True)`` followed by ``save_image``'s ``mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)`` gives
    on the CPU, byte for byte: device uint8 ``[rows * H, cols * W, 3]`` with ``cols = min(nrow, N)``, ``rows = ceil(N / cols)`` over the
    N images taken; image j sits in row ``j // cols``, column ``j % cols``, cells without an image are 0.

    ``images``: a tensor or a list of at most 8.  Each is ``[B, 1 or 3, H, W]`` fp32 on the device (made dense when it is not, an
    ``expand``ed one-channel image read as its one plane) or an internal image buffer of either precision (``ops.is_image``: planes
    0..2 are the image, the others never enter); all of one H x W, mixed freely.  The first ``nrow`` images of each are taken.
    ``value_range``: ``(lo, hi)``, or None for the minimum and maximum over exactly the values taken, found on the device (two
    launches, no host synchronisation; with a ``value_range`` it is one launch).

    Finite inputs are the contract.  A NaN or an infinity moves no access, but its bytes -- and, with ``value_range=None``, the
    range and so every byte -- are unspecified."""
    return _grid_u8(images, int(nrow), nrow, value_range)


def image_to_u8(x, value_range=(-1.0, 1.0)):
    """``x``: ``[B, 1 or 3, H, W]`` fp32 or an internal image buffer -> device uint8 ``[B, H, W, 3]``, each image converted as
    ``grid_u8`` converts it (the one-column grid of all B images is the batch layout): what a translated test set is written from.
    Non-finite inputs as for ``grid_u8``."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("image_to_u8 takes one tensor, got %s" % type(x).__name__)
    count = x.shape[0] if x.dim() == 4 and x.shape[0] > 0 else 1   # (else: _source words the refusal)
    out = _grid_u8([x], count, 1, value_range)
    return out.view(count, out.shape[0] // count, out.shape[1], 3)
