"""Spectral normalisation, ``Conv2dBlock(norm='sn')`` (reference networks.py:754-816), on csrc/spectral_norm.hip.

The reference wraps the convolution in ``SpectralNorm``: every call of the module runs ONE power iteration (u, v written back in
place), sigma = u . W_bar v, and the convolution runs on W_bar / sigma.  Here the convolution runs on W_bar itself (the existing
kernels, prepared-weight cache and refresh included) and 1 / sigma is applied in a segmented epilogue: a batch of S equal segments,
segment s scaled by the sigma of the s-th of S consecutive iterations -- what S calls of the reference module on the S segments
compute.  ``sn_power_iteration`` runs the S iterations of every SN layer of a network in 2 S + 1 launches (W_bar does not change
within a forward).

Gradient.  With y_s = act(Z_s r_s + b), Z = conv(x, W_bar), r_s = 1 / sigma_s and u, v held constant:
    dW_bar = wgrad(x, g r) - (sum_s c_s r_s^2) u v^T,   c_s = <g_s, Z_s>,  g = dy * act'
(<wgrad(x_s, g_s), W_bar> = <g_s, Z_s>, so sigma's share needs no per-segment weight gradient).  u and v are the values the
parameters hold when the backward runs, not those of iteration s: the reference rebinds ``u.data`` / ``v.data`` on every call and
autograd's saved references read the rebound storage, so a backward after several calls uses the last pair for every call's term
(its forward values use each call's own sigma).  The epilogue's backward reads the parameters' storage at that moment likewise.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops

# struct dwc_sn_desc of include/dwcgan_hip.h (72 bytes)
_DESC_DT = np.dtype([("w", "<u8"), ("u", "<u8"), ("v", "<u8"), ("off_u", "<i8"), ("off_v", "<i8"), ("off_r", "<i8"), ("cout", "<i4"),
                     ("k", "<i4"), ("col_blk0", "<i4"), ("row_blk0", "<i4"), ("vec", "<i4"), ("reserved", "<i4")])
assert _DESC_DT.itemsize == 72
_TABLES = {}         # (S, per-layer pointers and shapes) -> (device descriptor table, column blocks, row blocks, floats, layout, host copy)


def _up4(n):
    return (n + 3) // 4 * 4


class SNRun:
    """One ``sn_power_iteration``: S and, per SN container, (U [S, Cout] = u_s rows, V [S, K] = v_s rows, R [S] = 1 / sigma_s) --
    views of one device buffer that the launches filled."""

    def __init__(self, S, views):
        self.S = S
        self._views = views

    def layer(self, module):
        return self._views[id(module)]


def sn_power_iteration(layers, S):
    """S power iterations for every SN container in ``layers`` (modules with ``weight_bar`` [Cout, ...], ``weight_u`` [Cout],
    ``weight_v`` [K]); the parameters u / v hold the last iteration's pair afterwards (version counters bumped).  No host
    synchronisation: the descriptor table is uploaded once per layer set."""
    layers = list(layers)
    S = int(S)
    if not layers or S < 1:
        raise ValueError("sn_power_iteration: at least one layer and S >= 1")
    lib = _lib.load()
    w0 = layers[0].weight_bar
    ops._require_device(w0)
    dev = w0.device
    key = (S,) + tuple((m.weight_bar.data_ptr(), m.weight_u.data_ptr(), m.weight_v.data_ptr(), tuple(m.weight_bar.shape)) for m in layers)
    ent = _TABLES.get(key)
    if ent is None:
        desc = np.zeros(len(layers), dtype=_DESC_DT)
        cb, rb = ctypes.c_int(), ctypes.c_int()
        off = col = row = 0
        layout = []
        for i, m in enumerate(layers):
            w, u, v = m.weight_bar, m.weight_u, m.weight_v
            cout, k = w.shape[0], w[0].numel()
            for t in (w, u, v):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError("sn_power_iteration: fp32 contiguous parameters on one device expected")
            if u.numel() != cout or v.numel() != k:
                raise ValueError("sn_power_iteration: weight_u / weight_v do not match weight_bar %s" % (tuple(w.shape),))
            _lib.check(lib.dwc_sn_power_blocks(cout, k, ctypes.byref(cb), ctypes.byref(rb)), "sn_power_blocks (Cout <= 1024, K <= 8192)")
            ou, ov, orr = off, off + _up4(S * cout), off + _up4(S * cout) + _up4(S * k)
            desc[i] = (w.data_ptr(), u.data_ptr(), v.data_ptr(), ou, ov, orr, cout, k, col, row, int(k % 4 == 0 and w.data_ptr() % 16 == 0), 0)
            layout.append((ou, ov, orr, cout, k))
            off += lib.dwc_sn_layer_saved_floats(S, cout, k)
            col += cb.value
            row += rb.value
        host = torch.from_numpy(desc.view(np.uint8).reshape(-1)).pin_memory()
        ent = (host.to(dev, non_blocking=True), col, row, off, layout, host)
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = ent
    table, col, row, total, layout = ent[:5]
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    elems = sum(c * k for _, _, _, c, k in layout)
    _lib.check(ops._timed("sn_power_kernel", 4.0 * S * elems, lambda: lib.dwc_sn_power_iteration(
        table.data_ptr(), len(layers), col, row, buf.data_ptr(), S, ops._stream()),
        detail="sn-power L%d S%d" % (len(layers), S)), "sn_power_iteration")
    ops._hbm("sn_power", 8 * S * elems)           # W_bar read twice per iteration
    torch.autograd.graph.increment_version([m.weight_u for m in layers] + [m.weight_v for m in layers])
    views = {}
    for m, (ou, ov, orr, cout, k) in zip(layers, layout):
        views[id(m)] = (buf[ou:ou + S * cout].view(S, cout), buf[ov:ov + S * k].view(S, k), buf[orr:orr + S])
    return SNRun(S, views)


class _SNEpilogue(torch.autograd.Function):
    """y = act(Z * r_s + b) over S equal batch segments (csrc/spectral_norm.hip).  Z: the convolution on W_bar, no bias / activation,
    [N, Cp, H, W] channels-last with Cp the kernels' padded channel count.  Backward: dZ and db in one pass, and the gradient through
    sigma into W_bar (module docstring) when W_bar needs one."""

    @staticmethod
    def forward(ctx, z, b, w_bar, u, v, r, S, act):
        ops._require_device(z)
        lib = _lib.load()
        z = ops.cl(z)
        N, cp, H, W = z.shape
        if N % S:
            raise ValueError("SN epilogue: batch %d is not %d equal segments" % (N, S))
        cout = w_bar.shape[0]
        bias = torch.zeros(cp, dtype=torch.float32, device=z.device) if b is None else \
            torch.nn.functional.pad(b.detach().float(), (0, cp - cout)).contiguous()
        y = ops.empty_cl(N, cp, H, W, z.device, z.dtype)
        rows = N * H * W
        st = ops._stream()
        detail = "sn-epi-fwd B%d %dx%d C%d S%d" % (N, H, W, cp, S)
        if z.dtype == ops.BF16:
            _lib.check(ops._timed("sn_epilogue_kernel", 0.0, lambda: lib.dwc_bf16_sn_epilogue_fwd(
                z.data_ptr(), r.data_ptr(), bias.data_ptr(), y.data_ptr(), rows, cp, S, act, st), detail=detail), "bf16_sn_epilogue_fwd")
        else:
            ya, yep = ops.out_amax(y)
            _lib.check(ops._timed("sn_epilogue_kernel", 0.0, lambda: lib.dwc_sn_epilogue_fwd(
                z.data_ptr(), r.data_ptr(), bias.data_ptr(), y.data_ptr(), rows, cp, S, act, ya, yep, st), detail=detail), "sn_epilogue_fwd")
            if ya is not None:
                ops.set_amax(y, ya, yep)
        ops._hbm("sn_epilogue", 2 * z.numel() * z.element_size())
        ctx.save_for_backward(z, bias, r)
        ctx.uv = (u, v)             # (the parameters themselves: their storage is read when the backward runs, module docstring)
        ctx.geom = (S, act, b is not None, cout, tuple(w_bar.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        z, bias, r = ctx.saved_tensors
        S, act, has_b, cout, wshape = ctx.geom
        dy = ops.cl(dy)
        N, cp, H, W = z.shape
        rows = N * H * W
        dev = z.device
        half = z.dtype == ops.BF16
        need_db = has_b and ctx.needs_input_grad[1]
        dz = ops.empty_cl(N, cp, H, W, dev, z.dtype)
        db = torch.empty(cp, dtype=torch.float32, device=dev) if need_db else None
        c = torch.empty(S, dtype=torch.float32, device=dev)
        nws = lib.dwc_sn_epilogue_bwd_ws_bytes(rows, cp, S, 8 if half else 4)
        ws = ops.workspace(nws, dev)
        st = ops._stream()
        detail = "sn-epi-bwd B%d %dx%d C%d S%d" % (N, H, W, cp, S)
        if half:
            _lib.check(ops._timed("sn_epilogue_kernel", 0.0, lambda: lib.dwc_bf16_sn_epilogue_bwd(
                dy.data_ptr(), z.data_ptr(), r.data_ptr(), bias.data_ptr(), dz.data_ptr(), ops._p(db), c.data_ptr(), rows, cp, S, act,
                ws.data_ptr(), ws.numel(), st), detail=detail), "bf16_sn_epilogue_bwd")
        else:
            ga, gep = ops.out_amax(dz)
            _lib.check(ops._timed("sn_epilogue_kernel", 0.0, lambda: lib.dwc_sn_epilogue_bwd(
                dy.data_ptr(), z.data_ptr(), r.data_ptr(), bias.data_ptr(), dz.data_ptr(), ops._p(db), c.data_ptr(), rows, cp, S, act,
                ws.data_ptr(), ws.numel(), ga, gep, st), detail=detail), "sn_epilogue_bwd")
            if ga is not None:
                ops.set_amax(dz, ga, gep)
        ops._hbm("sn_epilogue", 3 * z.numel() * z.element_size())
        dw = None
        if ctx.needs_input_grad[2]:
            u, v = ctx.uv
            dw = torch.empty(wshape, dtype=torch.float32, device=dev)
            k = dw[0].numel()
            _lib.check(ops._timed("sn_wgrad_kernel", 0.0, lambda: lib.dwc_sn_weight_grad(
                u.data_ptr(), 0, v.data_ptr(), 0, r.data_ptr(), c.data_ptr(), dw.data_ptr(), S, cout, k, 0, st),
                detail="sn-wgrad %dx%d S%d" % (cout, k, S)), "sn_weight_grad")
        return dz, (db[:cout] if db is not None else None), dw, None, None, None, None, None


def sn_conv2d(x, module, run, stride, pad, act="none", token=None, pad_mode="reflect"):
    """The reference's SpectralNorm(nn.Conv2d) call on the HIP kernels: reflect-padded (``pad_mode='zero'``: zero-padded, as
    ops.conv2d) convolution on ``module.weight_bar``, then the
    segmented epilogue with ``run``'s 1 / sigma_s (``run.S`` equal batch segments) + bias + activation.  Returns Cout channels (a
    channel slice of the padded buffer when Cout is not a multiple of 4 / 8)."""
    w_bar = module.weight_bar
    _, _, r = run.layer(module)
    z = ops._Conv2d.apply(x, w_bar, None, int(stride), int(pad), 0, True, None, token, not torch.is_grad_enabled(),
                          ops._pad_mode_zero(pad_mode))
    y = _SNEpilogue.apply(z, module.bias, w_bar, module.weight_u, module.weight_v, r, run.S, ops.ACT[act])
    return y if y.shape[1] == w_bar.shape[0] else y[:, :w_bar.shape[0]]


def sn_weight_torch(module):
    """W_bar / sigma as a torch expression, sigma = u . (W_bar v) with the pair the last power iteration left in the parameters -- for the callers that
    differentiate twice (gradient / R1 penalties).  u and v enter through ``.data`` aliases: autograd reads them when the backward
    runs, as the reference's rebound ``u.data`` / ``v.data``, and later in-place iterations do not trip its version check."""
    w_bar = module.weight_bar
    sigma = torch.dot(module.weight_u.data, w_bar.reshape(w_bar.shape[0], -1).mv(module.weight_v.data))
    return w_bar / sigma
