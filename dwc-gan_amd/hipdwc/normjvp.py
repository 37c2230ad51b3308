"""Gradient and R1 penalties through a discriminator with ``dis.norm: in / ln`` on the HIP kernels.

The closed form of hipdwc.penalty rests on a piecewise-linear chain, whose second derivative vanishes.  A normalisation's does not.
What still holds: with P = phi(g), g = dy/dx and ghat = phi'(g) held constant,

    dP/dtheta = grad_theta <ghat, g(theta)> = grad_theta ydot,      ydot = the forward-mode derivative of y along ghat,

so the penalty needs only once-differentiable ops:

    primal        z_l = conv_l(reflect_pad(a_{l-1}); W_l) + b_l,  a_l = act(norm_l(z_l)),  a_0 = x   (layer 1 has no norm, as in _make_net)
    first order   g = grad(sum w_s a_L, x) through the existing backward;  (P, k) = dwc_grad_penalty_fwd(g);  ghat = k g
    tangent       t_0 = ghat;  zdot_l = conv_l(reflect_pad(t_{l-1}); W_l)  (no bias);  ndot_l = norm_tangent(z_l, zdot_l, gamma_l);
                  t_l = ndot_l * act'(a_l)  (the mask is a constant: act'' = 0 almost everywhere);  ydot = sum w_s t_L
    second order  dP/dtheta = autograd.grad(ydot, theta): W_l (through z_l and zdot_l), b_l, gamma_l, beta_l and w_s.

``norm_tangent`` is the one new op (csrc/norm_tangent.hip: forward and backward for both group kinds); ``_ActMask`` wraps
dwc_act_bwd_bias, whose backward is the same kernel.  Everything else is ``ops.conv2d`` / ``ops.instance_norm`` /
``ops.layer_norm_munit`` with the fused activation and the reductions of csrc/penalty.hip.

The primal forward runs TWICE: once with only x on the tape (for g), once with only the parameters on it (for the second-order
gradients).  One forward traversed twice (``retain_graph``) would be safe -- no residual tokens ride on this chain and every backward
takes its scratch afresh -- but a node decides at forward time which gradients it forms, so the first traversal would form every
weight gradient and the second every data gradient for nothing; L extra forward convolutions cost less than L extra weight gradients.

As in hipdwc.penalty the branch is fp32 whatever ``ops.PRECISION`` says, P is linear in its output gradient, the Function's forward
forms the unscaled gradients and its backward only multiplies them by ``dout``.
"""
import torch

from . import _lib, ops, penalty

KINDS = {"in": 0, "ln": 1}                # DWC_NORM_TANGENT_IN / DWC_NORM_TANGENT_LN


def supported_channels(c):
    """Whether csrc/norm_tangent.hip takes C = ``c`` (a power of two, 4 .. 1024): asked of the library, host only, no launch."""
    return _lib.load().dwc_norm_tangent_ws_bytes(KINDS["in"], 1, 4, int(c)) > 0


class _NormTangent(torch.autograd.Function):
    """ndot = d/ds norm(z + s zdot) at s = 0, without the norm's shift: gamma (r cd - lam A xh) in the notation of the kernel file."""

    @staticmethod
    def forward(ctx, z, zdot, gamma, kind, eps):
        ops._require_device(z)
        lib = _lib.load()
        z, zdot = ops.cl(z), ops.cl(zdot)
        if z.dtype != torch.float32 or zdot.dtype != torch.float32 or z.shape != zdot.shape:
            raise TypeError("norm_tangent: fp32 tensors of one shape")
        B, C, H, W = z.shape
        dev = z.device
        g = None if gamma is None else gamma.detach().float().contiguous()
        nws = lib.dwc_norm_tangent_ws_bytes(kind, B, H * W, C)
        if not nws:
            raise _lib.HipKernelError("norm_tangent: unsupported shape B%d C%d %dx%d (C a power of two, 4 .. 1024)" % (B, C, H, W))
        out = ops.empty_cl(B, C, H, W, dev)
        stats = torch.empty(lib.dwc_norm_tangent_stats_elems(kind, B, C), dtype=torch.float32, device=dev)
        ws = ops.workspace(nws, dev)
        _lib.check(lib.dwc_norm_tangent_fwd(z.data_ptr(), zdot.data_ptr(), ops._p(g), out.data_ptr(), stats.data_ptr(), kind, B, H * W, C,
                                            eps, ws.data_ptr(), ws.numel(), ops._stream()), "norm_tangent_fwd")
        ctx.save_for_backward(z, zdot, g, stats)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        z, zdot, g, stats = ctx.saved_tensors
        dout = ops.cl(dout)
        B, C, H, W = z.shape
        dev = z.device
        dz, dzdot = ops.empty_cl(B, C, H, W, dev), ops.empty_cl(B, C, H, W, dev)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if g is not None and ctx.needs_input_grad[2] else None
        ws = ops.workspace(lib.dwc_norm_tangent_ws_bytes(ctx.kind, B, H * W, C), dev)
        _lib.check(lib.dwc_norm_tangent_bwd(dout.data_ptr(), z.data_ptr(), zdot.data_ptr(), ops._p(g), stats.data_ptr(), dz.data_ptr(),
                                            dzdot.data_ptr(), ops._p(dgamma), ctx.kind, B, H * W, C, ws.data_ptr(), ws.numel(),
                                            ops._stream()), "norm_tangent_bwd")
        return dz, dzdot, dgamma, None, None


def norm_tangent(z, zdot, gamma=None, kind="in", eps=1e-5):
    """The tangent of ``ops.instance_norm(z)`` (kind "in"; no affine parameters) or ``ops.layer_norm_munit(z, gamma, beta)`` (kind
    "ln"; gamma [C] or None = 1) before the activation, along the input tangent ``zdot``.  fp32, differentiable once w.r.t. z, zdot
    and gamma."""
    if kind not in KINDS:
        raise ValueError("kind must be 'in' or 'ln'")
    if kind == "in" and gamma is not None:
        raise ValueError("kind 'in' is the plain instance norm: no gamma")
    return _NormTangent.apply(z, zdot, gamma, KINDS[kind], float(eps))


class _ActMask(torch.autograd.Function):
    """t * act'(a) for a piecewise-linear activation, the slope read off the activation OUTPUT a and treated as a constant."""

    @staticmethod
    def forward(ctx, t, a, act):
        a = ops.cl(a.detach())
        ctx.save_for_backward(a)
        ctx.act = act
        return penalty._act_bwd(ops.cl(t), a, act)[0]

    @staticmethod
    def backward(ctx, dy):
        a, = ctx.saved_tensors
        return penalty._act_bwd(ops.cl(dy), a, ctx.act)[0], None, None


def act_mask(t, a, act):
    return t if act == "none" else _ActMask.apply(t, a, act)


def _norm(z, kind, gamma, beta, eps, act):
    if kind == "ln":
        return ops.layer_norm_munit(z, gamma, beta, eps=eps, act=act)
    return ops.instance_norm(z, eps=eps, act=act)


def _primal(x, spec, Ws, bs, gammas, betas, owners):
    """a_1 .. a_L and z_1 .. z_L (None where the layer has no norm) of the chain on the current tape."""
    a, zs = [x], []
    for l, (act, kind, eps) in enumerate(spec):
        if kind == "none":
            zs.append(None)
            a.append(ops.conv2d(a[-1], Ws[l], bs[l], 2, 1, act, owner=owners[l]))
        else:
            # (IN subtracts the per-(n, c) mean: d/d bias == 0, returned as zeros)
            zs.append(ops.conv2d(a[-1], Ws[l], bs[l], 2, 1, "none", bias_grad=kind == "ln", owner=owners[l]))
            a.append(_norm(zs[-1], kind, gammas[l], betas[l], eps, act))
    return a, zs


class _SrcGradPenaltyNormed(torch.autograd.Function):
    """P(x; theta) as above.  x4: fp32 NHWC4 image; ``spec`` = (activation, norm kind, eps) per layer; ``params`` = W, b, gamma, beta
    per layer (None where the layer has none); 4x4 stride-2 convolutions under reflect padding."""

    @staticmethod
    def forward(ctx, x4, mode, spec, w_s, *params):
        ops._require_device(x4)
        L = len(spec)
        ctx.n_in = 4 + len(params)
        owners = params[0::4]
        det = [None if p is None else p.detach() for p in params]
        # ---- primal forward with x on the tape, first-order chain ---------------------------------------------------------------
        with torch.enable_grad():
            x = x4.detach().requires_grad_(True)
            a, _ = _primal(x, spec, det[0::4], det[1::4], det[2::4], det[3::4], owners)
        e = w_s.detach().reshape(1, -1, 1, 1).expand_as(a[L])
        g = ops.cl(torch.autograd.grad(a[L], x, grad_outputs=e)[0])
        del a, x
        out, k = penalty._penalty(g, mode)
        if not any(ctx.needs_input_grad[3:]):
            return out
        t = penalty._scale(g, k)
        # ---- primal forward with the parameters on the tape, tangent forward, second-order gradients ---------------------------------
        # (a bias in front of an instance norm stays off the tape: its gradient is identically zero, so it gets none)
        dead = {4 * l + 1 for l, (_, kind, _) in enumerate(spec) if kind == "in"}
        leaves = [w_s.detach().requires_grad_(True)] + [None if p is None else p.detach().requires_grad_(i not in dead)
                                                        for i, p in enumerate(params)]
        Ws, bs, gammas, betas = leaves[1::4], leaves[2::4], leaves[3::4], leaves[4::4]
        with torch.enable_grad():
            a, zs = _primal(x4.detach(), spec, Ws, bs, gammas, betas, owners)
            for l, (act, kind, eps) in enumerate(spec):
                zdot = ops.conv2d(t, Ws[l], None, 2, 1, "none", owner=owners[l])
                if kind != "none":
                    zdot = norm_tangent(zs[l], zdot, gammas[l], kind, eps)
                t = act_mask(zdot, a[l + 1], act)
            ydot = ops.conv2d(t, leaves[0], None, 1, 0, owner=w_s)
        idx = [i for i, p in enumerate(leaves) if p is not None and p.requires_grad and ctx.needs_input_grad[3 + i]]
        grads = torch.autograd.grad(ydot, [leaves[i] for i in idx], grad_outputs=torch.ones_like(ydot), allow_unused=True)
        ctx.slots = tuple(i for i, gr in zip(idx, grads) if gr is not None)
        ctx.save_for_backward(*[gr for gr in grads if gr is not None])
        return out

    @staticmethod
    def backward(ctx, dout):
        res = [None] * ctx.n_in
        for i, gr in zip(getattr(ctx, "slots", ()), ctx.saved_tensors):
            res[3 + i] = dout * gr
        return tuple(res)


def supported(dis):
    """Whether the first scale of the MsImageDis ``dis`` is a chain this route takes: dis.norm in / ln, reflect padding, an activation
    of penalty.ACTS, channel counts that the pointwise passes and the tangent kernels take."""
    blocks = list(dis.cnns_feat[0])
    if dis.norm not in KINDS or dis.pad_type != "reflect" or dis.activ not in penalty.ACTS:
        return False
    if not penalty.supported([blk.conv.weight for blk in blocks], [blk.act_kind for blk in blocks]):
        return False
    return all(blk.norm_kind == "none" or (blk.norm_kind == dis.norm and supported_channels(blk.conv.weight.shape[0])) for blk in blocks)


def src_grad_penalty(dis, x, mode):
    """``penalty.src_grad_penalty`` for a discriminator with ``dis.norm`` in / ln: differentiable w.r.t. the convolution weights and
    biases, the LayerNorm gamma / beta and the 'src' head's weight of scale 0."""
    if mode not in penalty.MODES:
        raise ValueError("mode must be 'gp' or 'r1'")
    if not supported(dis):
        raise NotImplementedError("HIP gradient penalties: discriminator norm %r / pad %r / activation %r / dim %r" % (
            dis.norm, dis.pad_type, dis.activ, dis.dim))
    ops._require_device(x)
    if not (x.dtype == torch.float32 and ops.is_image(x)):
        if x.shape[1] != 3:
            raise ValueError("expected a [B, 3, H, W] batch or an fp32 NHWC4 image buffer")
        x = ops._Pack4.apply(x.detach().float(), False)
    spec, params = [], []
    for blk in dis.cnns_feat[0]:
        ln = blk.norm_kind == "ln" and blk.norm.affine
        spec.append((blk.act_kind, blk.norm_kind, float(blk.norm.eps) if blk.norm is not None else 0.0))
        params += [blk.conv.weight, blk.conv.bias, blk.norm.gamma if ln else None, blk.norm.beta if ln else None]
    return _SrcGradPenaltyNormed.apply(x.detach(), mode, tuple(spec), dis.cnns_src[0].weight, *params)
