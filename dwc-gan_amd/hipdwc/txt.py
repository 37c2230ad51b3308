"""The text encoder's data movement on the kernels of csrc/txt_glue.hip (C ABI ``dwc_txt_*`` in include/dwcgan_hip.h).

``encode`` is what ``networks_v2.TxtEncoder.forward`` (and, on the caller's own word vectors, ``forward_embed``) runs when
``ops.TXT_FUSED`` is set: the same values, random draws and
gradients as its stock-tensor-op path, with ONE launch each for the layer-1 operand, the tensor between two layers and the final
states, and one each for their adjoints (the two sums of the backward -- style rows over t, table rows per token id -- stay
torch's reductions on the inputs they had, which keeps a run's bits).  The whole stack of layers is a single autograd node (``_TxtStack``): its backward calls
the layers' backward (``ops.lstm_layer_bwd``) itself, so every gradient tensor is written once, by the kernel that knows all of its
contributions, instead of being zero-filled, scattered into and summed by the autograd engine.

The thin wrappers (``operand_fwd`` ... ``states_bwd``) allocate their outputs as ordinary tensors; the kernels need no scratch.
"""
import torch

from . import _lib, host, ops
from .ops import _p, _stream

MAX_LAYERS = _lib.TXT_MAX_LAYERS


def _f32(t, shape=None):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "dense fp32 device tensor expected"
    assert shape is None or tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
    return t


def _i32(t, n):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n, "int32 [%d] device tensor expected" % n
    return t


def _layers(outs, cs):
    ly = _lib.TxtLayers()
    ly.n = len(outs)
    for l, (o, c) in enumerate(zip(outs, cs)):
        ly.out[l], ly.c[l] = _p(o), _p(c)
    return ly


def operand_fwd(table, tokens, order, mask, style, t_max):
    """X:[t_max,B,E+S] in length-sorted order.  tokens: int64 [B,seq_len] in caller order; mask: [>=t_max,B,E] sorted, or None."""
    B, seq_len = tokens.shape
    V, E = table.shape
    S = style.shape[1]
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and 1 <= t_max <= seq_len
    assert mask is None or (_f32(mask).shape[0] >= t_max and mask.shape[1:] == (B, E))
    x = torch.empty((t_max, B, E + S), dtype=torch.float32, device=table.device)
    _lib.check(_lib.load().dwc_txt_operand_fwd(_f32(table).data_ptr(), tokens.data_ptr(), _i32(order, B).data_ptr(), _p(mask),
                                               _f32(style, (B, S)).data_ptr(), x.data_ptr(), t_max, B, seq_len, E, S, V, _stream()),
               "txt_operand_fwd")
    return x


def operand_bwd(dxa, dxb, tokens, order, mask, E, vocab, padding_idx, need_style=True, need_table=True):
    """(d_style [B,S] in caller order, d_table [vocab,E]) from dX = dxa + dxb (dxb may be None), None where not needed.

    One launch lays dX out as the stock path's own intermediate gradients (``dwc_txt_operand_bwd``); the two sums are then the
    reductions that path runs, on the same values, shapes and strides -- the sum over t of the expanded style rows and
    ``embedding_dense_backward`` --, so that a training run has the bits it had without the kernels."""
    t_max, B, I = dxa.shape
    S = I - E
    seq_len = tokens.shape[1]
    _f32(dxa)
    assert dxb is None or _f32(dxb).shape == dxa.shape
    if not (need_style or need_table):
        return None, None
    dev = dxa.device
    d_cat = torch.empty((seq_len, B, I), dtype=torch.float32, device=dev) if need_style else None     # (columns E.. are written)
    d_emb = torch.empty((seq_len, B, E), dtype=torch.float32, device=dev) if need_table else None
    idx = torch.empty((seq_len, B), dtype=torch.int64, device=dev) if need_table else None
    _lib.check(_lib.load().dwc_txt_operand_bwd(dxa.data_ptr(), _p(dxb), tokens.data_ptr(), _i32(order, B).data_ptr(), _p(mask),
                                               _p(d_cat), _p(d_emb), _p(idx), t_max, B, seq_len, E, S, _stream()), "txt_operand_bwd")
    d_style = d_cat[:, :, E:].sum(0) if need_style else None
    d_table = None
    if need_table:
        d_table = torch.ops.aten.embedding_dense_backward(d_emb, idx, vocab, -1 if padding_idx is None else int(padding_idx), False)
    return d_style, d_table


def operand_embed_fwd(emb, order, lens, mask, style, t_max):
    """X:[t_max,B,E+S] in length-sorted order from the caller's embedded words.  emb: [B,seq_len,E] in caller order; lens: the sorted
    lengths; rows behind a sample's length are zeros whatever emb holds there (a select: NaN / Inf included)."""
    B, seq_len, E = _f32(emb).shape
    S = style.shape[1]
    assert 1 <= t_max <= seq_len
    assert mask is None or (_f32(mask).shape[0] >= t_max and mask.shape[1:] == (B, E))
    x = torch.empty((t_max, B, E + S), dtype=torch.float32, device=emb.device)
    _lib.check(_lib.load().dwc_txt_operand_embed_fwd(emb.data_ptr(), _i32(order, B).data_ptr(), _i32(lens, B).data_ptr(), _p(mask),
                                                     _f32(style, (B, S)).data_ptr(), x.data_ptr(), t_max, B, seq_len, E, S, _stream()),
               "txt_operand_embed_fwd")
    return x


def operand_embed_bwd(dxa, dxb, order, lens, mask, E, seq_len, need_style=True, need_emb=True):
    """(d_style [B,S] in caller order, d_emb [B,seq_len,E] in caller order) from dX = dxa + dxb (dxb may be None), None where not
    needed.  d_emb is written once, by the one launch (zeros behind each length and from t_max on); the style rows are summed by the
    reduction of ``operand_bwd``, on the tensor that launch lays out for it."""
    t_max, B, I = dxa.shape
    S = I - E
    _f32(dxa)
    assert dxb is None or _f32(dxb).shape == dxa.shape
    if not (need_style or need_emb):
        return None, None
    dev = dxa.device
    d_cat = torch.empty((seq_len, B, I), dtype=torch.float32, device=dev) if need_style else None     # (columns E.. are written)
    d_emb = torch.empty((B, seq_len, E), dtype=torch.float32, device=dev) if need_emb else None
    _lib.check(_lib.load().dwc_txt_operand_embed_bwd(dxa.data_ptr(), _p(dxb), _i32(order, B).data_ptr(), _i32(lens, B).data_ptr(),
                                                     _p(mask), _p(d_cat), _p(d_emb), t_max, B, seq_len, E, S, _stream()),
               "txt_operand_embed_bwd")
    return (d_cat[:, :, E:].sum(0) if need_style else None), d_emb


def _mask_args(mask, mask_row, T, B, H):
    if mask is None:
        return None, None
    if mask_row is None:
        _f32(mask, (T, B, 2 * H))
        return mask.data_ptr(), None
    assert _f32(mask).dim() == 2 and mask.shape[1] == 2 * H
    assert mask_row.is_cuda and mask_row.dtype == torch.int64 and mask_row.is_contiguous() and mask_row.numel() == T * B
    return mask.data_ptr(), mask_row.data_ptr()


def inter_fwd(out, mask=None, mask_row=None):
    """[T,B,2H] operand of the next layer from out:[2,T,B,H], times the inter-layer mask ([T,B,2H], or [rows,2H] with the int64 row
    of each (t, b) slot in ``mask_row``)."""
    _, T, B, H = _f32(out).shape
    m, r = _mask_args(mask, mask_row, T, B, H)
    data = torch.empty((T, B, 2 * H), dtype=torch.float32, device=out.device)
    _lib.check(_lib.load().dwc_txt_inter_fwd(out.data_ptr(), m, r, data.data_ptr(), T, B, H, _stream()), "txt_inter_fwd")
    return data


def inter_bwd(dxa, dxb, mask, mask_row, d_feat, order, last, layer, H):
    """d_out:[2,T,B,H] of ``layer`` (not the top one): the gradient from the next layer's operand plus its final-state rows of d_feat."""
    T, B, _ = _f32(dxa, (dxa.shape[0], dxa.shape[1], 2 * H)).shape
    assert dxb is None or _f32(dxb).shape == dxa.shape
    m, r = _mask_args(mask, mask_row, T, B, H)
    assert _f32(d_feat).numel() % (4 * B * H) == 0 and 0 <= layer < d_feat.numel() // (4 * B * H)
    d_out = torch.empty((2, T, B, H), dtype=torch.float32, device=dxa.device)
    _lib.check(_lib.load().dwc_txt_inter_bwd(dxa.data_ptr(), _p(dxb), m, r, d_feat.data_ptr(), _i32(order, B).data_ptr(),
                                             _i32(last, B).data_ptr(), layer, d_out.data_ptr(), T, B, H, _stream()), "txt_inter_bwd")
    return d_out


def states_fwd(outs, cs, last, unsort):
    """feat:[B, 4*L*H] from out / c ([2,T,B,H] each) of the L layers."""
    L = len(outs)
    assert 1 <= L <= MAX_LAYERS and len(cs) == L
    _, T, B, H = outs[0].shape
    for t in list(outs) + list(cs):
        _f32(t, (2, T, B, H))
    feat = torch.empty((B, 4 * L * H), dtype=torch.float32, device=outs[0].device)
    _lib.check(_lib.load().dwc_txt_states_fwd(_layers(outs, cs), _i32(last, B).data_ptr(), _i32(unsort, B).data_ptr(), feat.data_ptr(),
                                              T, B, H, _stream()), "txt_states_fwd")
    return feat


def states_bwd(d_feat, order, last, T, H, need_out):
    """(d_outs, d_cs): d_c of every layer and d_out of the layers ``need_out`` names (None for the others), [2,T,B,H] each."""
    B = d_feat.shape[0]
    L = d_feat.shape[1] // (4 * H)
    assert 1 <= L <= MAX_LAYERS and _f32(d_feat).shape[1] == 4 * L * H and len(need_out) == L
    new = lambda: torch.empty((2, T, B, H), dtype=torch.float32, device=d_feat.device)
    d_outs = [new() if need_out[l] else None for l in range(L)]
    d_cs = [new() for _ in range(L)]
    _lib.check(_lib.load().dwc_txt_states_bwd(d_feat.data_ptr(), _i32(order, B).data_ptr(), _i32(last, B).data_ptr(),
                                              _layers(d_outs, d_cs), T, B, H, _stream()), "txt_states_bwd")
    return d_outs, d_cs


def group_rows(layers, B, G):
    """Source flat row (of 2H floats) of every output row of ``regroup`` in groups of G: int64 [2*layers*B]."""
    L2 = 2 * layers
    o = torch.arange(L2 * B, dtype=torch.int64)
    g = o // L2 // G
    n = o - g * G * L2
    return (n // G) * B + g * G + n % G


def rank_rows(layers, W, Bl, rank):
    """(fwd, bwd): the row of the gathered [W][Bl][2*layers] rows that each output row of rank ``rank`` is, and the row of the gathered
    output gradients that each flat row of its own feat gradient is; int64 [2*layers*Bl] each."""
    L2, Bg = 2 * layers, W * Bl
    o = torch.arange(L2 * Bl, dtype=torch.int64)
    n = rank * Bl * L2 + o
    p, row = n // Bg, n % Bg
    s = row // Bl
    return s * Bl * L2 + p * Bl + row % Bl, (o // Bl) * Bg + rank * Bl + o % Bl


def _gathered(sync, t):
    out = sync.all_gather(t)
    if tuple(out.shape) != (sync.world,) + tuple(t.shape) or out.dtype != t.dtype or out.device != t.device:
        raise ValueError("regroup: sync.all_gather returned %s %s, expected %s" % (tuple(out.shape), out.dtype,
                                                                                   (sync.world,) + tuple(t.shape)))
    return out.contiguous()


class _Regroup(torch.autograd.Function):
    """feat [B, 4LH] -> the feature rows of the view taken per group of G samples (``sync`` None) or over the union of ``sync``'s
    ranks, on dwc_txt_regroup_*: one launch each way, and one all-gather each way in the rank form."""

    @staticmethod
    def forward(ctx, feat, L, G, sync):
        B, F = _f32(feat).shape
        H = F // (4 * L)
        ctx.geom, ctx.sync = (L, B, H, G), sync
        out = torch.empty((B, F), dtype=torch.float32, device=feat.device)
        lib = _lib.load()
        if sync is None:
            _lib.check(lib.dwc_txt_regroup_fwd(feat.data_ptr(), out.data_ptr(), L, B, H, G, _stream()), "txt_regroup_fwd")
        else:
            every = _gathered(sync, feat)
            _lib.check(lib.dwc_txt_regroup_rank_fwd(every.data_ptr(), out.data_ptr(), L, sync.world, B, H, sync.rank, _stream()),
                       "txt_regroup_rank_fwd")
        return out

    @staticmethod
    def backward(ctx, d_out):
        (L, B, H, G), sync = ctx.geom, ctx.sync
        d_out = _f32(d_out.contiguous())
        d_feat = torch.empty((B, 4 * L * H), dtype=torch.float32, device=d_out.device)
        lib = _lib.load()
        if sync is None:
            _lib.check(lib.dwc_txt_regroup_bwd(d_out.data_ptr(), d_feat.data_ptr(), L, B, H, G, _stream()), "txt_regroup_bwd")
        else:
            every = _gathered(sync, d_out)
            _lib.check(lib.dwc_txt_regroup_rank_bwd(every.data_ptr(), d_feat.data_ptr(), L, sync.world, B, H, sync.rank, _stream()),
                       "txt_regroup_rank_bwd")
        return d_feat, None, None, None


class _RegroupTorch(torch.autograd.Function):
    """The same permutation as stock indexing, in feat's precision and on its device: the A/B partner."""

    @staticmethod
    def forward(ctx, feat, L, G, sync):
        B, F = feat.shape
        ctx.shape, ctx.sync = (B, F, F // (2 * L)), sync
        if sync is None:
            fwd = group_rows(L, B, G)
            ctx.bwd = torch.sort(fwd)[1]                    # (the inverse permutation)
            src = feat
        else:
            fwd, ctx.bwd = rank_rows(L, sync.world, B, sync.rank)
            src = _gathered(sync, feat.contiguous())
        return src.reshape(-1, ctx.shape[2]).index_select(0, fwd.to(feat.device)).reshape(B, F)

    @staticmethod
    def backward(ctx, d_out):
        B, F, width = ctx.shape
        src = d_out if ctx.sync is None else _gathered(ctx.sync, d_out.contiguous())
        return src.reshape(-1, width).index_select(0, ctx.bwd.to(d_out.device)).reshape(B, F), None, None, None


def regroup(feat, group=None, sync=None, layers=None):
    """The heads' feature rows of ``feat`` [B, 4*layers*H] (``states_fwd``: the reference's view over the whole call) with the view
    taken over other sets of samples: per ``group`` consecutive samples -- 1: every row is the one of a batch-1 call --,
    or, with an active ``sync`` (``world``, ``rank``, ``all_gather``; hipdwc.syncbn.active), over the union of the ranks' batches in
    rank order, which gives this rank its rows of the single-device call on the concatenated batch.  ``group`` None or B without an
    active ``sync`` returns ``feat`` itself.  On the device with ``ops.TXT_FUSED`` the kernels move the rows; elsewhere stock indexing."""
    from .syncbn import active
    if feat.dim() != 2:
        raise ValueError("regroup: feat must be [batch, 4 * layers * hidden], got %s" % (list(feat.shape),))
    B, F = feat.shape
    on = active(sync)
    if group is not None and (int(group) < 1 or B % int(group)):
        raise ValueError("regroup: group %s does not divide the batch of %d" % (group, B))
    if group is not None and on:
        raise ValueError("regroup: group and an active sync exclude each other (the view is taken over the ranks' union)")
    if not on and (group is None or int(group) == B):
        return feat
    if layers is None or layers < 1 or F % (4 * layers):
        raise ValueError("regroup: %s layers do not divide a feature row of %d" % (layers, F))
    if feat.is_cuda and ops.TXT_FUSED:
        if layers > MAX_LAYERS:
            raise ValueError("the text encoder's kernels take up to %d LSTM layers (DWC_TXT_MAX_LAYERS), got %d" % (MAX_LAYERS, layers))
        return _Regroup.apply(feat.contiguous(), int(layers), 0 if on else int(group), sync if on else None)
    return _RegroupTorch.apply(feat, int(layers), 0 if on else int(group), sync if on else None)


class _Plan:
    """What one call of ``encode`` fixes outside the differentiable inputs: indices, masks, sizes, cache owners."""
    __slots__ = ("dense", "tokens", "order", "unsort", "lens", "last", "t_max", "mask_in", "masks", "mask_rows", "owners_ih", "owners_hh", "owners_b",
                 "padding_idx", "layers")


class _TxtStack(torch.autograd.Function):
    """(source of layer 1, style rows, stacked LSTM parameters of every layer) -> feat [B, 4*L*H].  The source is the embedding
    table, looked up at ``plan.tokens``, or -- ``plan.dense`` -- the caller's embedded words [B,seq_len,E] themselves; its gradient
    comes back in the same slot."""

    @staticmethod
    def forward(ctx, plan, table, style, *params):
        if plan.dense:
            data = operand_embed_fwd(table, plan.order, plan.lens, plan.mask_in, style.contiguous(), plan.t_max)
        else:
            data = operand_fwd(table, plan.tokens, plan.order, plan.mask_in, style.contiguous(), plan.t_max)
        outs, cs, saved = [], [], []
        for l in range(plan.layers):
            out, c, sv = ops.lstm_layer_fwd(data, plan.lens, *params[4 * l:4 * l + 4], owners=plan.owners_ih[l],
                                            owners_hh=plan.owners_hh[l], owners_b=plan.owners_b[l])
            outs.append(out)
            cs.append(c)
            saved.append(sv)
            if l + 1 < plan.layers:
                data = inter_fwd(out, plan.masks[l], plan.mask_rows[l])
        ctx.save_for_backward(*[t for sv in saved for t in sv.pop("tensors")])
        ctx.plan, ctx.saved = plan, saved
        ctx.table_shape = tuple(table.shape)
        return states_fwd(outs, cs, plan.last, plan.unsort)

    @staticmethod
    def backward(ctx, d_feat):
        plan, L = ctx.plan, ctx.plan.layers
        kept = ctx.saved_tensors
        saved = [dict(sv, tensors=kept[l * len(kept) // L:(l + 1) * len(kept) // L]) for l, sv in enumerate(ctx.saved)]
        T, _, _, H = saved[0]["shape"]
        need = ctx.needs_input_grad
        d_feat = d_feat.contiguous()
        d_outs, d_cs = states_bwd(d_feat, plan.order, plan.last, T, H, [l == L - 1 for l in range(L)])
        d_out = d_outs[L - 1]
        grads = [None] * (4 * L)
        d_style = d_table = None
        for l in reversed(range(L)):
            nw = need[3 + 4 * l:7 + 4 * l]
            need_x = l > 0 or need[1] or need[2]
            dx, dw_ih, dw_hh, db = ops.lstm_layer_bwd(saved[l], d_out, d_cs[l], need_x, nw[0], nw[1], nw[2] or nw[3], split_dx=True)
            grads[4 * l:4 * l + 4] = [dw_ih, dw_hh, db, db]
            if l > 0:
                d_out = inter_bwd(dx[0], dx[1], plan.masks[l - 1], plan.mask_rows[l - 1], d_feat, plan.order, plan.last, l - 1, H)
            elif need_x and plan.dense:
                d_style, d_table = operand_embed_bwd(dx[0], dx[1], plan.order, plan.lens, plan.mask_in, ctx.table_shape[2],
                                                     ctx.table_shape[1], need_style=need[2], need_emb=need[1])
            elif need_x:
                d_style, d_table = operand_bwd(dx[0], dx[1], plan.tokens, plan.order, plan.mask_in, ctx.table_shape[1],
                                               ctx.table_shape[0], plan.padding_idx, need_style=need[2], need_table=need[1])
        return (None, d_table, d_style) + tuple(grads)


def encode(enc, style_ord, src_tokens, src_lengths, packed_index, embeddings=None):
    """feat:[B, 4*L*H] of ``networks_v2.TxtEncoder`` ``enc`` for the caller's style rows, tokens [B,seq_len] and lengths [B].
    ``packed_index(lens_sorted, t_max, bsz, device)``: row of a PackedSequence's data that holds each (t, b) slot.
    ``embeddings`` (then ``src_tokens`` is None): the embedded words [B,seq_len,E] themselves, dense fp32 on the device, take the
    place of the table lookup (``TxtEncoder.forward_embed``); indices, draws and owners are the ones of the token path."""
    if enc.num_layers > MAX_LAYERS:
        raise ValueError("the text encoder's kernels take up to %d LSTM layers (DWC_TXT_MAX_LAYERS), got %d" % (MAX_LAYERS, enc.num_layers))
    noise = host.noise()
    dense = embeddings is not None
    dev = embeddings.device if dense else src_tokens.device
    bsz, seq_len = embeddings.shape[:2] if dense else src_tokens.shape
    lens_sorted, order_host = torch.sort(src_lengths.detach().to("cpu"), descending=True)     # on the host: no device sync per call
    # order, its inverse, the sorted lengths and the last-token index travel in ONE staging block (pinned: the copy does not make
    # the host wait for the stream), already in the int32 the kernels read
    stage = torch.empty(4, bsz, dtype=torch.int32)
    if ops.PINNED_STAGE:
        stage = stage.pin_memory()
    stage[0], stage[1], stage[2], stage[3] = order_host, torch.sort(order_host)[1], lens_sorted, lens_sorted - 1
    on_dev = stage.to(dev, non_blocking=True)
    lens_list = lens_sorted.tolist()
    training = enc.training
    H, E = enc.hidden_size, enc.embed_dim

    plan = _Plan()
    plan.dense = dense
    plan.tokens = None if dense else src_tokens.long().contiguous()   # (the kernels read int64; nn.Embedding also takes int32 ids)
    plan.order, plan.unsort, plan.lens, plan.last = on_dev[0], on_dev[1], on_dev[2], on_dev[3]
    plan.t_max, plan.layers, plan.padding_idx = int(lens_list[0]), enc.num_layers, enc.embed_tokens.padding_idx
    # The draws are those of the stock path, in its order and on its shapes: dropout_in on the embedded [seq_len,B,E] tokens, then per
    # layer boundary nn.LSTM's dropout -- in parity mode drawn in PACKED order and looked up per slot --, then parity mode's unused
    # draw on the padded memory (reference networks_v2.py:235-236).
    plan.mask_in = noise.dropout_mask((seq_len, bsz, E), enc.dropout_in, dev) if training and enc.dropout_in > 0 else None
    plan.masks, plan.mask_rows = [], []
    # (the masks between the layers are drawn while the stack runs in the stock path; nothing else draws in between, so drawing
    # them here, before the first launch, consumes the generators identically)
    for l in range(enc.num_layers - 1):
        mask = rows = None
        if training and enc.dropout_out > 0:
            if getattr(noise, "align_stream", False):
                mask = noise.dropout_mask((int(sum(lens_list)), 2 * H), enc.dropout_out, dev)
                rows = packed_index(lens_list, plan.t_max, bsz, dev)
            else:
                mask = noise.dropout_mask((plan.t_max, bsz, 2 * H), enc.dropout_out, dev)
        plan.masks.append(mask)
        plan.mask_rows.append(rows)
    if training and enc.dropout_out > 0 and getattr(noise, "align_stream", False):
        noise.dropout_mask((plan.t_max, bsz, 2 * H), enc.dropout_out, dev)
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    per_layer = [{n: tuple(getattr(enc.lstm, "%s_l%d%s" % (n, l, suf)) for suf in ("", "_reverse")) for n in names}
                 for l in range(enc.num_layers)]
    plan.owners_ih = [p["weight_ih"] for p in per_layer]
    plan.owners_hh = [p["weight_hh"] for p in per_layer]
    plan.owners_b = [p["bias_ih"] + p["bias_hh"] for p in per_layer]
    params = [ops.cat_params(p[n], stack=True) for p in per_layer for n in names]
    return _TxtStack.apply(plan, embeddings if dense else enc.embed_tokens.weight, style_ord, *params)
