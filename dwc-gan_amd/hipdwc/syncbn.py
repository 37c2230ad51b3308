"""Synchronised batch norm: ``batch_norm(..., sync=...)`` of hipdwc.batchnorm under data parallel (hipdwc.dp).

Each rank holds Bs samples of each of the S segments; a SEGMENT IS THE UNION OF THE RANKS' PARTS of it, and is normalised with the
statistics of that union -- what a single device computes on the global batch.  ``order`` and ``num_batches_tracked`` mean what they
mean without ``sync``; eval mode uses the buffers and exchanges nothing; ``world == 1`` without ``force`` takes the plain path.

The plain chain (statistics, finalise, apply; backward likewise) is cut at the two points where per-(segment, channel) numbers exist:

    forward    moments (count, mean, M2)[3][S][C]  -> all-gather ->  finalise (Chan merge in RANK order, buffers)  -> apply
    backward   sums (sum g, sum g xhat)[2][S][C], local dgamma / dbeta  -> all-gather ->  apply (adds the R entries in rank order)

(count, mean, M2) does not add, so the exchange is an all-gather and the merge is the kernels' own ``bn_merge``: the pivoted
statistics survive (a sum x / sum x^2 all-reduce would lose them), and the fixed order makes mean, rstd, dx and the running buffers
bit-identical on every rank and run to run -- the order of a library's reduction is not ours to fix.  dgamma / dbeta stay sums over
the rank's own samples: the gradient reducer averages them like any other parameter gradient.

``sync`` is any object with ``world``, ``rank`` and ``all_gather(t) -> [world, *t.shape]`` in rank order (``GroupSync`` is the one over
torch.distributed); optional attributes: ``force`` (take the phase path at world 1) and ``segment_batch`` (samples per segment over
all ranks, where the ranks' shards are not equal; default ``world * Bs`` -- equal shards are the contract of ``dp.shard_batch``).

Two forms, as in hipdwc.batchnorm: ``_SyncBatchNorm`` on the five phases of csrc/norm.hip (dwc_syncbn_*), and ``_SyncBatchNormTorch``,
the same semantics on stock ops (CPU tensors, ``DWC_BN_HIP=0``, shapes the kernels do not take): the A/B partner.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib, ops
from .batchnorm import MAX_SEGMENTS, _act_torch, _stat


class GroupSync:
    """``sync`` over a torch.distributed process group (None: the default group).  ``all_gather`` returns a persistent receive buffer
    per (shape, dtype, device): its contents hold until the next gather of that shape -- the phases consume it at once, in stream
    order.  ``calls`` / ``bytes`` count the collectives issued.  Copy-safe: a deep copy of a module that carries one (Solver.copy_nets)
    shares the handle instead of copying a live process group."""

    def __init__(self, group=None, force=False):
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.force = force
        self.stacked = dist.get_backend(group) == "nccl"        # gloo refuses a stacked output: it takes the list form
        self.calls = 0
        self.bytes = 0
        self._recv = {}

    def __deepcopy__(self, memo):
        return self

    def all_gather(self, t):
        t = t.contiguous()
        key = (tuple(t.shape), t.dtype, t.device)
        out = self._recv.get(key)
        if out is None:
            out = self._recv[key] = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        if self.stacked:
            dist.all_gather_into_tensor(out, t, group=self.group)
        else:
            dist.all_gather(list(out.unbind(0)), t, group=self.group)
        self.calls += 1
        self.bytes += out.numel() * out.element_size()
        return out


def active(sync):
    """Whether ``sync`` asks for the phase path: more than one rank, or forced."""
    return sync is not None and (sync.world > 1 or bool(getattr(sync, "force", False)))


def _segment_batch(sync, Bs):
    n = getattr(sync, "segment_batch", None)
    return int(sync.world) * Bs if n is None else int(n)


def _gathered(sync, t, what):
    out = sync.all_gather(t)
    if tuple(out.shape) != (sync.world,) + tuple(t.shape) or out.dtype != t.dtype or out.device != t.device:
        raise ValueError("batch_norm: sync.all_gather returned %s %s for the %s, expected %s" % (
            tuple(out.shape), out.dtype, what, (sync.world,) + tuple(t.shape)))
    return out.contiguous()


def sync_moments(x, S):
    """This rank's (count, mean, M2) of its part of each of the S segments of x: fp32 [3, S, C] (dwc_syncbn_moments)."""
    ops._require_device(x)
    lib = _lib.load()
    x = ops.cl(x)
    B, C, H, W = x.shape
    Bs = B // S
    moments = torch.empty((3, S, C), dtype=torch.float32, device=x.device)
    ws = ops.workspace(lib.dwc_syncbn_ws_bytes(S, Bs, H * W, C), x.device)
    _lib.check(ops._fn(lib, "syncbn_moments", x)(x.data_ptr(), moments.data_ptr(), S, Bs, H * W, C, ws.data_ptr(), ws.numel(),
                                                 ops._stream()), "syncbn_moments")
    return moments


def sync_finalise(moments_all, running_mean, running_var, order, momentum, eps):
    """(mean, rstd), fp32 [S * C] each, of the union of the R gathered moments [R, 3, S, C], merged in rank order; steps the running
    buffers (None: skipped) through ``order`` in place (dwc_syncbn_finalise)."""
    lib = _lib.load()
    R, _, S, C = moments_all.shape
    dev = moments_all.device
    mean = torch.empty(S * C, dtype=torch.float32, device=dev)
    rstd = torch.empty(S * C, dtype=torch.float32, device=dev)
    desc = _lib.BnOrder(len(order), (ctypes.c_int * MAX_SEGMENTS)(*order))
    _lib.check(lib.dwc_syncbn_finalise(moments_all.data_ptr(), R, mean.data_ptr(), rstd.data_ptr(), ops._p(running_mean),
                                       ops._p(running_var), S, C, eps, momentum, desc, ops._stream()), "syncbn_finalise")
    return mean, rstd


def sync_bwd_sums(dy, x, mean, rstd, weight, bias, S, act, need_dweight=True, need_dbias=True):
    """(sums, dweight, dbias): this rank's (sum g, sum g xhat) per segment, fp32 [2, S, C], and the parameter gradients over its own
    samples (None where there is no parameter or ``need_*`` is off), with the global ``mean`` / ``rstd`` of the forward
    (dwc_syncbn_bwd_sums).  ``act``: 'none' / 'relu' / 'lrelu' or its code."""
    ops._require_device(x)
    lib = _lib.load()
    act = ops.ACT[act] if isinstance(act, str) else act
    x = ops.cl(x)
    dy = ops.cl(dy.to(x.dtype))
    B, C, H, W = x.shape
    Bs = B // S
    dev = x.device
    gamma = None if weight is None else weight.detach().float().contiguous()
    beta = None if bias is None else bias.detach().float().contiguous()
    sums = torch.empty((2, S, C), dtype=torch.float32, device=dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None and need_dweight else None
    dbeta = torch.empty(C, dtype=torch.float32, device=dev) if beta is not None and need_dbias else None
    ws = ops.workspace(lib.dwc_syncbn_ws_bytes(S, Bs, H * W, C), dev)
    _lib.check(ops._fn(lib, "syncbn_bwd_sums", x)(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ops._p(gamma),
                                                  ops._p(beta), sums.data_ptr(), ops._p(dgamma), ops._p(dbeta), S, Bs, H * W, C, act,
                                                  ws.data_ptr(), ws.numel(), ops._stream()), "syncbn_bwd_sums")
    return sums, dgamma, dbeta


class _SyncBatchNorm(torch.autograd.Function):
    """``_BatchNorm`` of hipdwc.batchnorm in training mode with the statistics of the union over ``sync``'s ranks: forward moments,
    gather, finalise, apply; backward sums, gather, apply (module docstring).  Two collectives per call and pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, S, order, act, momentum, eps, sync):
        ops._require_device(x)
        x = ops.cl(x)
        B, C, H, W = x.shape
        Bs = B // S
        dev = x.device
        gamma = None if weight is None else weight.detach().float().contiguous()
        beta = None if bias is None else bias.detach().float().contiguous()
        _stat(running_mean, "running_mean")
        _stat(running_var, "running_var")
        moments_all = _gathered(sync, sync_moments(x, S), "moments")
        mean, rstd = sync_finalise(moments_all, running_mean, running_var, order, momentum, eps)
        y = ops.empty_cl(B, C, H, W, dev, x.dtype)
        amax = ops._norm_call("syncbn_apply", x, y, (x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ops._p(gamma), ops._p(beta),
                                                     y.data_ptr(), S, Bs, H * W, C, act))
        if amax:
            ops.set_amax(y, *amax)
        ops._hbm("syncbn_fwd", x.numel() * x.element_size() * 3)
        if running_mean is not None and len(order):
            torch.autograd.graph.increment_version([running_mean, running_var])      # (written through raw pointers)
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.geom = (S, act, _segment_batch(sync, Bs) * H * W)
        ctx.sync = sync
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        S, act, n_global = ctx.geom
        dy = ops.cl(dy.to(x.dtype))
        B, C, H, W = x.shape
        Bs = B // S
        sums, dgamma, dbeta = sync_bwd_sums(dy, x, mean, rstd, gamma, beta, S, act, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        sums_all = _gathered(ctx.sync, sums, "backward sums")
        dx = ops.empty_cl(B, C, H, W, x.device, x.dtype)
        amax = ops._norm_call("syncbn_bwd_apply", x, dx, (dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ops._p(gamma),
                                                          ops._p(beta), sums_all.data_ptr(), sums_all.shape[0], n_global, dx.data_ptr(),
                                                          S, Bs, H * W, C, act))
        if amax:
            ops.set_amax(dx, *amax)
        ops._hbm("syncbn_bwd", x.numel() * x.element_size() * 5)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def _act_grad(pre, g, act):
    if act == "relu":
        return torch.where(pre > 0, g, torch.zeros_like(g))
    if act == "lrelu":
        return torch.where(pre > 0, g, 0.1 * g)
    return g


class _SyncBatchNormTorch(torch.autograd.Function):
    """The same semantics on stock ops, in x's precision (statistics in fp32 for bf16): the partner of ``_segmented_torch``."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, S, order, act, momentum, eps, sync):
        B, C, H, W = x.shape
        Bs = B // S
        st = torch.float32 if x.dtype == ops.BF16 else x.dtype
        xs = x.detach().to(st).reshape(S, Bs, C, H, W)
        n = Bs * H * W
        mean_l = xs.mean((1, 3, 4))
        m2_l = ((xs - mean_l[:, None, :, None, None]) ** 2).sum((1, 3, 4))
        moments_all = _gathered(sync, torch.stack([torch.full_like(mean_l, float(n)), mean_l, m2_l]), "moments")
        cnt, mean, m2 = moments_all[0, 0].clone(), moments_all[0, 1].clone(), moments_all[0, 2].clone()
        for r in range(1, moments_all.shape[0]):            # Chan et al., rank order
            cb, mb, m2b = moments_all[r]
            tot, delta = cnt + cb, mb - mean
            mean = mean + delta * (cb / tot)
            m2 = m2 + m2b + delta * delta * (cnt * (cb / tot))
            cnt = tot
        rstd = 1.0 / torch.sqrt(m2 / cnt + eps)
        if running_mean is not None:
            uvar = m2 / (cnt - 1.0)
            for s in order:
                running_mean.mul_(1.0 - momentum).add_(momentum * mean[s].to(running_mean.dtype))
                running_var.mul_(1.0 - momentum).add_(momentum * uvar[s].to(running_var.dtype))
        w = None if weight is None else weight.detach().to(st)
        b = None if bias is None else bias.detach().to(st)
        xhat = (xs - mean[:, None, :, None, None]) * rstd[:, None, :, None, None]
        pre = xhat if w is None else xhat * w[None, None, :, None, None]
        if b is not None:
            pre = pre + b[None, None, :, None, None]
        ctx.save_for_backward(xhat, pre, rstd, w)
        ctx.geom = (act, cnt, x.dtype, b is not None)
        ctx.sync = sync
        return _act_torch(pre, act).reshape(B, C, H, W).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        xhat, pre, rstd, w = ctx.saved_tensors
        act, cnt, dtype, has_bias = ctx.geom
        g = _act_grad(pre, dy.to(xhat.dtype).reshape(xhat.shape), act)
        sums = torch.stack([g.sum((1, 3, 4)), (g * xhat).sum((1, 3, 4))])
        sums_all = _gathered(ctx.sync, sums, "backward sums")
        tot = sums_all[0].clone()
        for r in range(1, sums_all.shape[0]):
            tot = tot + sums_all[r]
        k1, k2 = tot[0] / cnt, tot[1] / cnt
        scale = rstd if w is None else rstd * w[None, :]
        dx = scale[:, None, :, None, None] * (g - k1[:, None, :, None, None] - xhat * k2[:, None, :, None, None])
        dw = sums[1].sum(0) if w is not None and ctx.needs_input_grad[1] else None
        db = sums[0].sum(0) if has_bias and ctx.needs_input_grad[2] else None
        return dx.reshape(dy.shape).to(dtype), dw, db, None, None, None, None, None, None, None, None


def sync_batch_norm(x, weight, bias, running_mean, running_var, S, order, act, momentum, eps, sync, hip):
    """Training-mode batch norm over S segments with the statistics of the union over ``sync``'s ranks; ``hip``: on the kernels."""
    n = _segment_batch(sync, x.shape[0] // S) * x.shape[2] * x.shape[3]
    if n < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s in %d segment(s) on %d rank(s)" % (
            list(x.shape), S, sync.world))
    fn = _SyncBatchNorm if hip else _SyncBatchNormTorch
    return fn.apply(x, weight, bias, running_mean, running_var, S, order, ops.ACT[act] if hip else act, float(momentum), float(eps), sync)
