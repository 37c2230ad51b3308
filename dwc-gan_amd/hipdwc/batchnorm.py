"""Batch normalisation, ``Conv2dBlock(norm='bn')`` / dis.norm 'bn' (reference networks.py:547 nn.BatchNorm2d), over S equal batch
segments on csrc/norm.hip.

Batch norm is a cross-sample op: the reference's separate discriminator calls each normalise with their OWN batch statistics and
each step the running buffers once, so the solver's single pass over a concatenated batch is only the same computation when the
statistics are taken per segment.  ``batch_norm(x, ..., segments=S, order=...)``: x is S equal parts of the batch, part s is
normalised exactly as the module would normalise it in a call of its own, and the running buffers are stepped once per entry of
``order`` (segment indices, default 0 .. S-1; an index may repeat: the reference's D step calls the module on x_real twice), in that
sequence, on the device.  One statistics launch, one finalise launch (which also steps the buffers) and one apply launch with the
activation fused; backward likewise.  Statistics are fp32 and combined in a fixed order: bit-identical run to run, and a segment's
result does not depend on how many segments share the launch.

``DWC_BN_HIP=0`` (``BN_HIP``), and channel counts the kernels do not take (not a multiple of 4 fp32 / 8 bf16, more than 256 such
groups) or more than 8 segments / updates, run the same segmented semantics on stock device ops -- ``F.batch_norm`` per segment, in
``order``: the A/B partner of the kernels (benchmarks/bn_overhead.py) and the only fallback.

Under data parallel the statistics are per rank unless ``sync=`` is given: hipdwc.syncbn cuts the two kernel chains where
per-(segment, channel) numbers exist and exchanges those between the ranks.
"""
import ctypes
import os

import torch
import torch.nn.functional as F

from . import _lib, ops

BN_HIP = int(os.environ.get("DWC_BN_HIP", "1"))
ACTS = ("none", "relu", "lrelu")
MAX_SEGMENTS = _lib.BN_MAX_SEGMENTS


def supported(x, segments=1, n_order=None):
    """Whether csrc/norm.hip takes this tensor: a device fp32 / bf16 [B, C, H, W] with C a multiple of 4 / 8 and at most 256 such
    groups, up to 8 segments and running-statistics updates."""
    if not x.is_cuda or x.dim() != 4 or x.dtype not in (torch.float32, ops.BF16):
        return False
    v = 8 if x.dtype == ops.BF16 else 4
    c = x.shape[1]
    n_order = segments if n_order is None else n_order
    return c % v == 0 and c // v <= 256 and 1 <= segments <= MAX_SEGMENTS and n_order <= MAX_SEGMENTS and x.shape[0] <= 65535


def _stat(t, what):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise ValueError("batch_norm: %s must be a contiguous fp32 tensor" % what)
    return t


class _BatchNorm(torch.autograd.Function):
    """y = act((x - mean_s) * rstd_s * weight + bias) over S equal batch segments (csrc/norm.hip); steps running_mean / running_var in
    place through ``order`` when training.  Backward: dx with the coupling sums of the element's own segment, dweight / dbias summed
    over all segments (only for the parameters that require a gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, S, order, act, training, momentum, eps):
        ops._require_device(x)
        lib = _lib.load()
        x = ops.cl(x)
        B, C, H, W = x.shape
        Bs = B // S
        dev = x.device
        gamma = None if weight is None else weight.detach().float().contiguous()
        beta = None if bias is None else bias.detach().float().contiguous()
        _stat(running_mean, "running_mean")
        _stat(running_var, "running_var")
        y = ops.empty_cl(B, C, H, W, dev, x.dtype)
        mean = torch.empty(S * C, dtype=torch.float32, device=dev)
        rstd = torch.empty(S * C, dtype=torch.float32, device=dev)
        ws = ops.workspace(lib.dwc_batchnorm_ws_bytes(S, Bs, H * W, C), dev)
        desc = _lib.BnOrder(len(order), (ctypes.c_int * MAX_SEGMENTS)(*order))
        amax = ops._norm_call("batchnorm_fwd", x, y, (x.data_ptr(), ops._p(gamma), ops._p(beta), ops._p(running_mean), ops._p(running_var),
                                                      y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), S, Bs, H * W, C, eps, momentum, act,
                                                      int(training), desc, ws.data_ptr(), ws.numel()))
        if amax:
            ops.set_amax(y, *amax)
        ops._hbm("batchnorm_fwd", x.numel() * x.element_size() * (3 if training else 2))
        if training and running_mean is not None and len(order):
            torch.autograd.graph.increment_version([running_mean, running_var])      # (written through raw pointers)
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.geom = (S, act, int(training))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        S, act, training = ctx.geom
        dy = ops.cl(dy.to(x.dtype))
        B, C, H, W = x.shape
        Bs = B // S
        dev = x.device
        dx = ops.empty_cl(B, C, H, W, dev, x.dtype)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None and ctx.needs_input_grad[1] else None
        dbeta = torch.empty(C, dtype=torch.float32, device=dev) if beta is not None and ctx.needs_input_grad[2] else None
        ws = ops.workspace(lib.dwc_batchnorm_ws_bytes(S, Bs, H * W, C), dev)
        amax = ops._norm_call("batchnorm_bwd", x, dx, (dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ops._p(gamma), ops._p(beta),
                                                       dx.data_ptr(), ops._p(dgamma), ops._p(dbeta), S, Bs, H * W, C, act, training,
                                                       ws.data_ptr(), ws.numel()))
        if amax:
            ops.set_amax(dx, *amax)
        ops._hbm("batchnorm_bwd", x.numel() * x.element_size() * 5)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def _act_torch(y, act):
    if act == "relu":
        return torch.relu(y)
    if act == "lrelu":
        return F.leaky_relu(y, 0.1)
    return y


def _segmented_torch(x, weight, bias, running_mean, running_var, S, order, act, training, momentum, eps):
    """The same semantics on stock ops: ``F.batch_norm`` per segment; the call that produces a segment's output is the segment's first
    entry in ``order`` (it steps the buffers), a repeated entry steps them again from the same segment, a segment outside ``order``
    leaves them alone."""
    if not training:
        return _act_torch(F.batch_norm(x, running_mean, running_var, weight, bias, False, momentum, eps), act)
    parts = list(torch.chunk(x, S)) if S > 1 else [x]
    ys = [None] * S
    for s in order:
        if ys[s] is None:
            ys[s] = F.batch_norm(parts[s], running_mean, running_var, weight, bias, True, momentum, eps)
        elif running_mean is not None:
            with torch.no_grad():
                F.batch_norm(parts[s].detach(), running_mean, running_var, None, None, True, momentum, eps)
    for s in range(S):
        if ys[s] is None:
            ys[s] = F.batch_norm(parts[s], None, None, weight, bias, True, momentum, eps)
    return _act_torch(torch.cat(ys) if S > 1 else ys[0], act)


def batch_norm(x, weight, bias, running_mean, running_var, segments=1, order=None, act="none", training=True, momentum=0.1, eps=1e-5,
               sync=None):
    """nn.BatchNorm2d (+ none / relu / lrelu(0.1)) on a batch of ``segments`` equal parts, each normalised as in a call of its own;
    ``order``: the segments whose statistics step the running buffers, in sequence (default every segment once).  ``training=False``:
    the running buffers normalise the whole batch and are not written (segments / order do not matter).

    ``sync`` (data parallel, hipdwc.syncbn): an object with ``world``, ``rank`` and ``all_gather``; a segment is then the union of the
    ranks' parts of it and is normalised with the statistics of that union, identical bit for bit on every rank, as are the running
    buffers.  ``order`` means the same; eval mode exchanges nothing; ``None``, or one rank without ``sync.force``, is the path above."""
    if momentum is None:
        raise NotImplementedError("batch_norm: momentum=None (cumulative moving average) is not built")
    if act not in ACTS:
        raise ValueError("batch_norm: activation %r is not one of %s" % (act, ACTS))
    if x.dim() != 4:
        raise ValueError("batch_norm: expected a 4-D NCHW-shaped tensor")
    S = int(segments)
    B = x.shape[0]
    if S < 1 or B % S:
        raise ValueError("batch_norm: batch %d is not %d equal segments" % (B, S))
    order = tuple(range(S)) if order is None else tuple(int(i) for i in order)
    if any(i < 0 or i >= S for i in order):
        raise ValueError("batch_norm: order %s names a segment outside 0..%d" % (order, S - 1))
    if (running_mean is None) != (running_var is None):
        raise ValueError("batch_norm: running_mean and running_var come together")
    synced = False
    if training and sync is not None:
        from . import syncbn
        synced = syncbn.active(sync)
    if training:
        if not synced and (B // S) * x.shape[2] * x.shape[3] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s in %d segment(s)" % (
                list(x.shape), S))
    else:
        if running_mean is None:
            raise NotImplementedError("batch_norm: eval mode without running statistics")
        S, order = 1, ()
    if BN_HIP and not x.is_cuda:
        ops._require_device(x)
    if synced:
        return syncbn.sync_batch_norm(x, weight, bias, running_mean, running_var, S, order, act, momentum, eps, sync,
                                      bool(BN_HIP and supported(x, S, len(order))))
    if BN_HIP and supported(x, S, len(order)):
        return _BatchNorm.apply(x, weight, bias, running_mean, running_var, S, order, ops.ACT[act], bool(training), float(momentum),
                                float(eps))
    return _segmented_torch(x, weight, bias, running_mean, running_var, S, order, act, training, momentum, eps)
