"""Gradient penalty and R1 penalty of the discriminator's first scale on the HIP kernels (reference solver.py:291-315, 337-350).

Both penalties differentiate the 'src' map of scale 0 w.r.t. its INPUT and then that gradient w.r.t. D's weights.  The HIP autograd
Functions are once-differentiable, and they stay so: with piecewise-linear activations (lrelu / relu / none) and ``norm: none`` the
second derivative has a closed form made of the convolutions ``ops.conv2d`` already dispatches:

    forward        a_l = act(conv_l(reflect_pad(a_{l-1}); W_l) + b_l),  a_0 = x
    first order    d_L = w_s * act'(a_L);  e_{l-1} = dgrad_l(d_l; W_l);  d_l = e_l * act'(a_l);  g = e_0
    penalty        q_n = |g_n|^2;  GP: P = mean (sqrt(q_n) - 1)^2,  R1: P = mean q_n^2;  ghat = dP/dg = k_n g_n
    second order   dhat_l = conv_l(reflect_pad(ehat_{l-1}); W_l)  (ehat_0 = ghat; no bias, no activation)
                   dP/dW_l = wgrad_l(input ehat_{l-1}, output gradient d_l);  ehat_l = dhat_l * act'(a_l)
                   dP/dw_s[c] = sum over samples and pixels of ehat_L;  the biases get no gradient (act'' = 0 almost everywhere)

Every convolution, data gradient and weight gradient above is a call of ``ops.conv2d`` / the backward of ``ops._Conv2d`` (under
``torch.enable_grad()``, through ``torch.autograd.grad`` with the activations as inputs), so kernel selection, prepared weight
layouts (cached on the parameters, shared with the D pass proper) and absmax slots keep their single home in hipdwc.ops.  The passes
that are not convolutions run on csrc/penalty.hip (dwc_grad_penalty_fwd / _scale, dwc_src_head_seed) and dwc_act_bwd_bias.

The branch is fp32 whatever ``ops.PRECISION`` says (the torch branch it replaces is fp32 too): it packs its own fp32 NHWC4 image.

P is linear in its own output gradient, so the Function's forward already forms the (unscaled) weight gradients and its backward
only multiplies them by ``dout``: no activation outlives the forward.  Under data parallelism these gradients reach the parameters
through autograd's ordinary accumulation, like those of the adversarial terms: the bucket reducer (hipdwc.dp) needs no change.
"""
import torch

from . import _lib, ops

MODES = {"gp": 0, "r1": 1}                # DWC_PENALTY_GP / DWC_PENALTY_R1
ACTS = ("lrelu", "relu", "none")
_ONE = {}                                  # device index -> fp32 [1] holding 1.0 (the forward's own `dout`)


def _one(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _ONE.get(key)
    if t is None:
        t = _ONE[key] = torch.ones(1, dtype=torch.float32, device=dev)
    return t


def _act_bwd(dy, y, act, want_g=True, want_db=False):
    """g = dy * act'(y) (channels-last like dy) and / or db[c] = sum over rows of g: dwc_act_bwd_bias."""
    lib = _lib.load()
    B, C, H, W = dy.shape
    rows = B * H * W
    g = ops.empty_cl(B, C, H, W, dy.device) if want_g else None
    db = torch.empty(C, dtype=torch.float32, device=dy.device) if want_db else None
    ws = ops.workspace(lib.dwc_act_bwd_bias_ws_bytes(rows, C), dy.device)
    _lib.check(lib.dwc_act_bwd_bias(dy.data_ptr(), y.data_ptr(), ops._p(g), ops._p(db), rows, C, ops.ACT[act], ws.data_ptr(), ws.numel(),
                                    ops._stream()), "act_bwd_bias")
    return g, db


def _seed(a, w_s, act):
    """d = w_s * act'(a) for the activation map a [B, C, h, w] (channels-last) under the 1x1 src head w_s [1, C, 1, 1]."""
    B, C, h, w = a.shape
    d = ops.empty_cl(B, C, h, w, a.device)
    ws = w_s.detach().reshape(-1).contiguous()
    _lib.check(_lib.load().dwc_src_head_seed(a.data_ptr(), ws.data_ptr(), d.data_ptr(), B * h * w, C, ops.ACT[act], ops._stream()),
               "src_head_seed")
    return d


def _penalty(g, mode):
    """(P, k) of the NHWC4 gradient image g [B, 4, H, W]: the penalty and the per-sample coefficient of dP/dg."""
    B, planes, H, W = g.shape
    q = torch.empty(B, dtype=torch.float32, device=g.device)
    k = torch.empty(B, dtype=torch.float32, device=g.device)
    out = torch.empty((), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().dwc_grad_penalty_fwd(g.data_ptr(), q.data_ptr(), k.data_ptr(), out.data_ptr(), B, H * W, planes, 3,
                                                MODES[mode], ops._stream()), "grad_penalty_fwd")
    return out, k


def _scale(g, k):
    """ghat = k_n * g on the three real planes, zero on the padding plane (the forward's own dout is 1)."""
    B, planes, H, W = g.shape
    ghat = ops.empty_cl(B, planes, H, W, g.device)
    _lib.check(_lib.load().dwc_grad_penalty_scale(g.data_ptr(), k.data_ptr(), _one(g.device).data_ptr(), ghat.data_ptr(), B, H * W, planes,
                                                  3, ops._stream()), "grad_penalty_scale")
    return ghat


def supported(weights, acts):
    """Whether the chain's channel counts suit the pointwise passes (dwc_act_bwd_bias: C / 4 divides 256 or is a multiple of it)."""
    for w in weights:
        c = w.shape[0]
        if c % 4 or (256 % (c // 4) if c // 4 < 256 else (c // 4) % 256):
            return False
    return all(a in ACTS for a in acts)


class _SrcGradPenalty(torch.autograd.Function):
    """P(x; W_1..W_L, w_s) as above.  x4: fp32 NHWC4 image; ``wb`` = W_1, b_1, ..., W_L, b_L (4x4, stride 2, reflect pad 1)."""

    @staticmethod
    def forward(ctx, x4, mode, acts, w_s, *wb):
        ops._require_device(x4)
        L = len(wb) // 2
        Ws, bs = wb[0::2], wb[1::2]
        ctx.L = L
        # ---- forward and first-order chain: one graph node per layer, the weights off the tape ------------------------------
        with torch.enable_grad():
            a = [x4.detach().requires_grad_(True)]
            for l in range(L):
                a.append(ops.conv2d(a[-1], Ws[l].detach(), bs[l].detach(), 2, 1, acts[l], owner=Ws[l]))
        d = [None] * (L + 1)
        d[L] = _seed(a[L], w_s, acts[L - 1])
        e = w_s.detach().reshape(1, -1, 1, 1).expand_as(a[L])
        for l in range(L, 0, -1):
            if l < L:                            # (the node's backward forms the same product on its way to the data gradient)
                d[l] = e if acts[l - 1] == "none" else _act_bwd(e, a[l], acts[l - 1])[0]
            e = torch.autograd.grad(a[l], a[l - 1], grad_outputs=e)[0]
        g = ops.cl(e)
        a[0] = None
        # ---- penalty and its gradient w.r.t. g --------------------------------------------------------------------------------------
        out, k = _penalty(g, mode)
        if not any(ctx.needs_input_grad[3:]):
            return out
        eh = _scale(g, k)
        # ---- second-order chain: forward convolution of ehat, weight gradient against d_l ------------------------------------------
        grads = []
        for l in range(1, L + 1):
            with torch.enable_grad():
                w = Ws[l - 1].detach().requires_grad_(True)
                dh = ops.conv2d(eh, w, None, 2, 1, "none", owner=Ws[l - 1])
            grads.append(torch.autograd.grad(dh, w, grad_outputs=d[l])[0])
            d[l] = None
            dh = dh.detach()
            if l < L:
                eh = dh if acts[l - 1] == "none" else _act_bwd(dh, a[l], acts[l - 1])[0]
            else:
                grads.append(_act_bwd(dh, a[l], acts[l - 1], want_g=False, want_db=True)[1])
            a[l] = None
        ctx.save_for_backward(*grads)
        return out

    @staticmethod
    def backward(ctx, dout):
        if not ctx.saved_tensors:
            return (None,) * (4 + 2 * ctx.L)
        *dws, dsrc = ctx.saved_tensors
        res = [None, None, None, (dout * dsrc).reshape(1, -1, 1, 1) if ctx.needs_input_grad[3] else None]
        for l in range(ctx.L):
            res += [dout * dws[l] if ctx.needs_input_grad[4 + 2 * l] else None, None]
        return tuple(res)


def src_grad_penalty(dis, x, mode):
    """``Solver.gradient_penalty`` (mode "gp": mean (|dy/dx|_2 - 1)^2) or ``Solver.r1_penalty`` (mode "r1": mean (|dy/dx|_2^2)^2) of
    y = sum of the first scale's 'src' map of the MsImageDis ``dis`` at x ([B, 3, H, W], or an fp32 NHWC4 image buffer), differentiable
    w.r.t. the convolution weights of that scale.  Raises NotImplementedError for a discriminator outside the closed form (see
    MsImageDis.penalty_hip_ok)."""
    if mode not in MODES:
        raise ValueError("mode must be 'gp' or 'r1'")
    if not dis.penalty_hip_ok():
        raise NotImplementedError("HIP gradient penalties: discriminator norm %r / pad %r / activation %r / dim %r" % (
            dis.norm, dis.pad_type, dis.activ, dis.dim))
    ops._require_device(x)
    if not (x.dtype == torch.float32 and ops.is_image(x)):
        if x.shape[1] != 3:
            raise ValueError("expected a [B, 3, H, W] batch or an fp32 NHWC4 image buffer")
        x = ops._Pack4.apply(x.detach().float(), False)
    blocks = list(dis.cnns_feat[0])
    wb = []
    for blk in blocks:
        wb += [blk.conv.weight, blk.conv.bias]
    return _SrcGradPenalty.apply(x.detach(), mode, tuple(blk.act_kind for blk in blocks), dis.cnns_src[0].weight, *wb)
