"""The loader's resize / to-float / normalise steps on the device: uint8 HWC crops -> internal image buffer in one HIP launch
(csrc/image_u8.hip).  ``data_loader.get_loader(..., device_transform=True)`` delivers the crops.

The result is bit-equal to the CPU chain followed by ``ops.pack_image``: PIL's ``BILINEAR`` resize of an 8-bit image is integer
arithmetic on windows of 22-bit fixed-point coefficients (``resample_table`` builds them in float64 on the host, by the rule of
Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc``), and the normalised value of each of the 256 possible bytes is taken
from a table computed with ``ImageTransform``'s own expression.
"""
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
