"""GPU tests of the text encoder's fused data movement (csrc/txt_glue.hip, hipdwc/txt.py).

Two groups.  The first calls every ``dwc_txt_*`` export through the C ABI itself, into NaN-filled outputs, and compares with the
stock tensor expression it replaces (lines of ``networks_v2.TxtEncoder.forward``) with ``torch.equal``: every kernel is pure
movement, and the two sums of the backward (style rows, embedding table) are torch's reductions on what the kernels lay out.  The second runs ``TxtEncoder`` forward + backward on both paths
(``ops.TXT_FUSED`` 0 and 1) under one seed and compares what ``ops.lstm_layer_fwd`` / ``ops.lstm_layer_bwd`` and the heads were
handed on either path -- the layer-1 operand, the tensor between the layers, ``feat``, ``d_out``, ``d_c``, ``dX`` --, the outputs,
the generator states and the parameter gradients.

Shapes: E 12, S 8, H 16, seq_len 7; batch 3 with lengths [3, 5, 1] (unsorted, a length 1, t_max < seq_len) and batch 1; one and two
layers; token rows with a repeated id and padding ids, padding inside t < t_max included.

Bound of the summed gradients (style rows, embedding table, LSTM weights): twice the largest error the stock path itself shows
against a float64 evaluation of the same expression on the same inputs and masks (CPU ``nn.LSTM`` in double per layer), per tensor;
both errors are printed before the assertion.  After an in-place step of the weights the bound run is one that keeps no derived
tensor (``ops._lstm_derived`` replaced by a plain rebuild), since both paths share the per-step caches of the transposed ``w_hh`` and
the bias sum.  ``dropout_in`` and ``dropout_out`` are switched separately.
"""
import types

import pytest
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

pytestmark = pytest.mark.gpu

from hipdwc import host, ops, txt            # noqa: E402
from hipdwc import _lib as _lib_mod          # noqa: E402
from networks import networks_v2             # noqa: E402

DEV = "cuda:0"
E, S, H, SEQ, VOCAB, PAD = 12, 8, 16, 7, 11, 0
C_DIM, N_CLS = 2, 4                          # style width S = C_DIM * N_CLS
BATCHES = {
    # lengths, token rows [B, SEQ]: id 4 twice in row 0, ids 2 and 4 shared between rows, padding from each length on
    "b3": ([3, 5, 1], [[4, 7, 4, 0, 0, 0, 0], [2, 4, 9, 2, 10, 0, 0], [7, 0, 0, 0, 0, 0, 0]]),
    "b1": ([4], [[5, 5, 3, 8, 0, 0, 0]]),
}


def _dev(t):
    return t.to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _indices(lens):
    """order, unsort, sorted lengths, last as the encoder stages them: int32 on the device, plus the int64 forms for torch indexing."""
    lens_sorted, order = torch.sort(torch.tensor(lens), descending=True)
    unsort = torch.sort(order)[1]
    i32 = lambda t: _dev(t.to(torch.int32))
    return types.SimpleNamespace(order=i32(order), unsort=i32(unsort), lens=i32(lens_sorted), last=i32(lens_sorted - 1),
                                 order64=_dev(order), unsort64=_dev(unsort), last64=_dev(lens_sorted - 1),
                                 lens_list=lens_sorted.tolist(), t_max=int(lens_sorted[0]))


def _keep_mask(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return _dev((torch.rand(shape, generator=g) > 0.3).float() / 0.7)


def _stock_feat(outs, cs, ix, bsz):
    """networks_v2.TxtEncoder.forward: final states -> feat, as stock tensor ops."""
    cols = torch.arange(bsz, device=DEV)
    hs, cc = [], []
    for out, cell in zip(outs, cs):
        hs += [out[0][ix.last64, cols], out[1][0]]
        cc += [cell[0][ix.last64, cols], cell[1][0]]
    L = len(outs)
    h_n, c_n = torch.stack(hs), torch.stack(cc)
    h_n = h_n.view(L, 2, bsz, -1).transpose(1, 2).reshape(L, bsz, -1).index_select(1, ix.unsort64)
    c_n = c_n.view(L, 2, bsz, -1).transpose(1, 2).reshape(L, bsz, -1).index_select(1, ix.unsort64)
    return torch.cat([h_n, c_n], dim=1).view(bsz, -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the exports, one by one, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_operand_exports(batch, masked):
    lib = _lib_mod.load()
    lens, rows = BATCHES[batch]
    B, ix = len(lens), _indices(lens)
    g = torch.Generator().manual_seed(3)
    table, style = _dev(torch.randn(VOCAB, E, generator=g)), _dev(torch.randn(B, S, generator=g))
    tokens = _dev(torch.tensor(rows))
    mask = _keep_mask((SEQ, B, E), 5) if masked else None
    x = _nan(ix.t_max, B, E + S)
    rc = lib.dwc_txt_operand_fwd(table.data_ptr(), tokens.data_ptr(), ix.order.data_ptr(), ops._p(mask), style.data_ptr(), x.data_ptr(),
                                 ix.t_max, B, SEQ, E, S, VOCAB, ops._stream())
    assert rc == 0
    emb = table[tokens.t().index_select(1, ix.order64)]
    emb = emb * mask if masked else emb
    want = torch.cat([emb, style.index_select(0, ix.order64).expand(SEQ, -1, -1)], -1)[:ix.t_max]
    assert torch.equal(x, want)

    # adjoint: the kernel lays dX out as the stock expression's own intermediate gradients (pure movement: torch.equal with autograd
    # of that expression up to the two sums), into NaN-filled outputs
    dxa, dxb = _dev(torch.randn(ix.t_max, B, E + S, generator=g)), _dev(torch.randn(ix.t_max, B, E + S, generator=g))
    tok_sorted = tokens.t().index_select(1, ix.order64)
    for second in (dxb, None):
        d_cat, d_emb, idx = _nan(SEQ, B, E + S), _nan(SEQ, B, E), torch.full((SEQ, B), -7, dtype=torch.int64, device=DEV)
        rc = lib.dwc_txt_operand_bwd(dxa.data_ptr(), ops._p(second), tokens.data_ptr(), ix.order.data_ptr(), ops._p(mask),
                                     d_cat.data_ptr(), d_emb.data_ptr(), idx.data_ptr(), ix.t_max, B, SEQ, E, S, ops._stream())
        assert rc == 0
        dx = dxa + second if second is not None else dxa
        emb_in = torch.zeros(SEQ, B, E, device=DEV, requires_grad=True)
        sty_in = torch.zeros(SEQ, B, S, device=DEV, requires_grad=True)          # the expanded style rows, sorted order
        emb = emb_in * mask if masked else emb_in * 1.0
        want_emb, want_sty = torch.autograd.grad(torch.cat([emb, sty_in], -1)[:ix.t_max], [emb_in, sty_in], dx)
        assert torch.equal(idx, tok_sorted)
        assert torch.equal(d_emb, want_emb)
        assert torch.equal(d_cat[:, :, E:], want_sty.index_select(1, ix.unsort64))     # (caller order)
        assert torch.isnan(d_cat[:, :, :E]).all()                                       # (columns the kernel does not own)
    # the wrapper's two sums are the stock path's reductions on these tensors: same bits as autograd of the stock expression
    table_p, style_p = table.clone().requires_grad_(True), style.clone().requires_grad_(True)
    emb = torch.nn.functional.embedding(tok_sorted, table_p, PAD)
    emb = emb * mask if masked else emb
    x_stock = torch.cat([emb, style_p.index_select(0, ix.order64).expand(SEQ, -1, -1)], -1)[:ix.t_max]
    want_table, want_style = torch.autograd.grad(x_stock, [table_p, style_p], dxa + dxb)
    d_style, d_table = txt.operand_bwd(dxa, dxb, tokens, ix.order, mask, E, VOCAB, PAD)
    assert torch.equal(d_table, want_table) and torch.equal(d_table[PAD], torch.zeros(E, device=DEV))
    # (autograd un-sorts the summed rows with index_add_; a permutation adds each row to a zero)
    assert torch.equal(d_style, want_style)
    # a frozen table / a style that needs no gradient: the other outputs alone; nothing asked for: refused
    d_cat = _nan(SEQ, B, E + S)
    assert lib.dwc_txt_operand_bwd(dxa.data_ptr(), None, tokens.data_ptr(), ix.order.data_ptr(), ops._p(mask), d_cat.data_ptr(), None, None,
                                   ix.t_max, B, SEQ, E, S, ops._stream()) == 0
    assert not torch.isnan(d_cat[:, :, E:]).any()
    assert lib.dwc_txt_operand_bwd(dxa.data_ptr(), None, tokens.data_ptr(), ix.order.data_ptr(), None, None, None, None,
                                   ix.t_max, B, SEQ, E, S, ops._stream()) == _lib_mod.EINVAL


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_prev_state_export(batch):
    lens, _ = BATCHES[batch]
    B, T = len(lens), max(lens)
    out = _dev(torch.randn(2, T, B, H, generator=torch.Generator().manual_seed(17)))
    for t_, o in ((T, out), (1, out[:, :1].contiguous())):
        hprev = _nan(2, t_, B, H)
        assert _lib_mod.load().dwc_txt_prev_state(o.data_ptr(), hprev.data_ptr(), t_, B, H, ops._stream()) == 0
        want = torch.zeros(2, t_, B, H, device=DEV)
        want[0, 1:] = o[0, :-1]
        want[1, :-1] = o[1, 1:]
        assert torch.equal(hprev, want)


@pytest.mark.parametrize("mask_kind", ["nomask", "padded", "packed"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_inter_exports(batch, mask_kind):
    lib = _lib_mod.load()
    lens, _ = BATCHES[batch]
    B, ix = len(lens), _indices(lens)
    T = ix.t_max
    g = torch.Generator().manual_seed(11)
    out = _dev(torch.randn(2, T, B, H, generator=g))
    mask = rows = None
    if mask_kind == "padded":
        mask = _keep_mask((T, B, 2 * H), 6)
        padded = mask
    elif mask_kind == "packed":
        mask = _keep_mask((sum(lens), 2 * H), 7)
        rows = networks_v2._packed_index(ix.lens_list, T, B, DEV)
        padded = mask.index_select(0, rows).view(T, B, -1)
    data = _nan(T, B, 2 * H)
    assert lib.dwc_txt_inter_fwd(out.data_ptr(), ops._p(mask), ops._p(rows), data.data_ptr(), T, B, H, ops._stream()) == 0
    want = torch.cat([out[0], out[1]], -1)
    want = want * padded if mask is not None else want
    assert torch.equal(data, want)

    # adjoint with the final-state rows of layer 0 of a two-layer d_feat folded in, against autograd of the stock expression
    dxa, dxb = _dev(torch.randn(T, B, 2 * H, generator=g)), _dev(torch.randn(T, B, 2 * H, generator=g))
    d_feat = _dev(torch.randn(B, 8 * H, generator=g))
    o0 = out.clone().requires_grad_(True)
    o1, c0, c1 = (_dev(torch.randn(2, T, B, H, generator=g)) for _ in range(3))
    nxt = torch.cat([o0[0], o0[1]], -1)
    nxt = nxt * padded if mask is not None else nxt
    for second in (dxb, None):
        dx = dxa + second if second is not None else dxa
        want, = torch.autograd.grad([nxt, _stock_feat([o0, o1], [c0, c1], ix, B)], [o0], [dx, d_feat], retain_graph=True)
        d_out = _nan(2, T, B, H)
        assert lib.dwc_txt_inter_bwd(dxa.data_ptr(), ops._p(second), ops._p(mask), ops._p(rows), d_feat.data_ptr(), ix.order.data_ptr(),
                                     ix.last.data_ptr(), 0, d_out.data_ptr(), T, B, H, ops._stream()) == 0
        assert torch.equal(d_out, want)


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_states_exports(batch, layers):
    lib = _lib_mod.load()
    lens, _ = BATCHES[batch]
    B, ix = len(lens), _indices(lens)
    T = ix.t_max
    g = torch.Generator().manual_seed(13)
    outs = [_dev(torch.randn(2, T, B, H, generator=g)).requires_grad_(True) for _ in range(layers)]
    cs = [_dev(torch.randn(2, T, B, H, generator=g)).requires_grad_(True) for _ in range(layers)]
    feat = _nan(B, 4 * layers * H)
    ly = txt._layers(outs, cs)
    assert lib.dwc_txt_states_fwd(ly, ix.last.data_ptr(), ix.unsort.data_ptr(), feat.data_ptr(), T, B, H, ops._stream()) == 0
    want = _stock_feat(outs, cs, ix, B)
    assert torch.equal(feat, want)

    d_feat = _dev(torch.randn(B, 4 * layers * H, generator=g))
    grads = torch.autograd.grad(want, outs + cs, d_feat)
    d_outs, d_cs = [_nan(2, T, B, H) for _ in range(layers)], [_nan(2, T, B, H) for _ in range(layers)]
    gl = txt._layers(d_outs, d_cs)
    assert lib.dwc_txt_states_bwd(d_feat.data_ptr(), ix.order.data_ptr(), ix.last.data_ptr(), gl, T, B, H, ops._stream()) == 0
    for got, ref in zip(d_outs + d_cs, grads):
        assert torch.equal(got, ref)
    # a NULL d_out is left alone (a lower layer's comes from dwc_txt_inter_bwd), the rest is still written
    d_cs2 = [_nan(2, T, B, H) for _ in range(layers)]
    gl = txt._layers([None] * layers, d_cs2)
    assert lib.dwc_txt_states_bwd(d_feat.data_ptr(), ix.order.data_ptr(), ix.last.data_ptr(), gl, T, B, H, ops._stream()) == 0
    for got, ref in zip(d_cs2, grads[layers:]):
        assert torch.equal(got, ref)
    gl.n = _lib_mod.TXT_MAX_LAYERS + 1
    assert lib.dwc_txt_states_bwd(d_feat.data_ptr(), ix.order.data_ptr(), ix.last.data_ptr(), gl, T, B, H, ops._stream()) == _lib_mod.EINVAL


@pytest.mark.parametrize("shape", [(SEQ, 3, E), (5, 3, 2 * H), (40, 16, 300), (40, 16, 600)], ids=str)
def test_dropout_mask_is_the_draw_of_f_dropout(shape):
    """What lets the fused path take ``DeviceNoise.dropout_mask(shape)`` where the stock path calls ``F.dropout`` on a tensor of that
    shape: same mask, same generator state afterwards, and x * mask has the bits of F.dropout(x)."""
    x = _dev(torch.randn(shape, generator=torch.Generator().manual_seed(1)))
    for p in (0.1, 0.5):
        torch.manual_seed(77)
        a = F.dropout(x, p=p, training=True)
        state_a = torch.cuda.get_rng_state(DEV)
        torch.manual_seed(77)
        mask = host.DeviceNoise().dropout_mask(shape, p, torch.device(DEV))
        assert torch.equal(torch.cuda.get_rng_state(DEV), state_a)
        assert torch.equal(x * mask, a)


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder on both paths
# ---------------------------------------------------------------------------------------------------------------------------------
_UNWRAPPED = (ops.lstm_layer_fwd, ops.lstm_layer_bwd, networks_v2.TxtEncoder._heads)


class _Recorder:
    """Wraps ops.lstm_layer_fwd / lstm_layer_bwd and TxtEncoder._heads (both paths go through them) and keeps what they were handed."""

    def __init__(self, monkeypatch):
        self.x, self.d_out, self.d_c, self.dx, self.feat = [], [], [], [], []
        fwd, bwd, heads = _UNWRAPPED

        def rec_fwd(x, *a, **k):
            self.x.append(x.detach().clone())
            return fwd(x, *a, **k)

        def rec_bwd(saved, d_out, d_c, *a, **k):
            self.d_out.append(d_out.detach().clone())
            self.d_c.append(d_c.detach().clone())
            res = bwd(saved, d_out, d_c, *a, **k)
            dx = res[0]
            if isinstance(dx, tuple):
                dx = dx[0] if dx[1] is None else dx[0] + dx[1]
            self.dx.append(None if dx is None else dx.detach().clone())
            return res

        def rec_heads(mod, feat):
            self.feat.append(feat.detach().clone())
            return heads(mod, feat)

        monkeypatch.setattr(ops, "lstm_layer_fwd", rec_fwd)
        monkeypatch.setattr(ops, "lstm_layer_bwd", rec_bwd)
        monkeypatch.setattr(networks_v2.TxtEncoder, "_heads", rec_heads)


def _recording(base):
    class Rec(base):
        def __init__(self):
            super().__init__()
            self.masks = []

        def dropout_mask(self, shape, p, device):
            m = super().dropout_mask(shape, p, device)
            self.masks.append(m)
            return m
    return Rec()


def _run(enc, fused, noise_cls, seed, style, tokens, lens, g_mu, g_lv, monkeypatch):
    """One forward + backward; everything the comparison needs."""
    monkeypatch.setattr(ops, "TXT_FUSED", int(fused))
    rec = _Recorder(monkeypatch)
    noise = host.set_noise(_recording(noise_cls))
    for p in enc.parameters():
        p.grad = None
    sty = style.clone().requires_grad_(True)
    torch.manual_seed(seed)
    mu, lv = enc(sty, tokens, lens)
    states = (torch.cuda.get_rng_state(DEV), torch.get_rng_state())
    ((mu.flat * g_mu).sum() + (lv.flat * g_lv).sum()).backward()
    grads = {n: p.grad.detach().clone() for n, p in enc.named_parameters() if p.grad is not None}
    grads["style"] = sty.grad.detach().clone()
    return types.SimpleNamespace(mu=mu.flat.detach(), lv=lv.flat.detach(), rec=rec, masks=noise.masks, states=states, grads=grads)


def _ref64(enc, style, tokens, lens, masks, aligned, g_mu, g_lv):
    """float64 evaluation of TxtEncoder.forward + backward on the CPU with the fp32 runs' masks: name -> gradient."""
    cpu = lambda t: t.detach().double().cpu()
    lens_sorted, order = torch.sort(torch.tensor(lens), descending=True)
    unsort, B, t_max = torch.sort(order)[1], len(lens), int(lens_sorted[0])
    masks = [cpu(m) for m in masks]
    table = cpu(enc.embed_tokens.weight).requires_grad_(True)
    sty = cpu(style).requires_grad_(True)
    emb = F.embedding(tokens.cpu().t().index_select(1, order), table, enc.embed_tokens.padding_idx)
    if enc.dropout_in > 0:
        emb = emb * masks.pop(0)
    data = torch.cat([emb, sty.index_select(0, order).expand(SEQ, -1, -1)], -1)[:t_max]
    hs, cs, layers = [], [], []
    for l in range(enc.num_layers):
        lstm = nn.LSTM(data.shape[2], H, 1, bidirectional=True).double()
        with torch.no_grad():
            for n, p in lstm.named_parameters():
                p.copy_(cpu(getattr(enc.lstm, n.replace("_l0", "_l%d" % l))))
        layers.append(lstm)
        o, (hn, cn) = lstm(pack_padded_sequence(data, lens_sorted))
        data = pad_packed_sequence(o, total_length=t_max)[0]
        hs.append(hn)
        cs.append(cn)
        if l + 1 < enc.num_layers and enc.dropout_out > 0:
            m = masks.pop(0)
            if aligned:
                m = m.index_select(0, networks_v2._packed_index(lens_sorted.tolist(), t_max, B, "cpu")).view(t_max, B, -1)
            data = data * m
    L = enc.num_layers
    h_n = torch.cat(hs).view(L, 2, B, -1).transpose(1, 2).reshape(L, B, -1).index_select(1, unsort)
    c_n = torch.cat(cs).view(L, 2, B, -1).transpose(1, 2).reshape(L, B, -1).index_select(1, unsort)
    feat = torch.cat([h_n, c_n], dim=1).view(B, -1)
    w = torch.cat([cpu(m.weight) for m in enc.fcs] + [cpu(m.weight) for m in enc.fcvars])
    b = torch.cat([cpu(m.bias) for m in enc.fcs] + [cpu(m.bias) for m in enc.fcvars])
    out = F.linear(feat, w, b)
    k = N_CLS * C_DIM
    ((out[:, :k] * cpu(g_mu)).sum() + (out[:, k:] * cpu(g_lv)).sum()).backward()
    grads = {"style": sty.grad, "embed_tokens.weight": table.grad}
    for l, lstm in enumerate(layers):
        for n, p in lstm.named_parameters():
            grads["lstm." + n.replace("_l0", "_l%d" % l)] = p.grad
    return grads


def _same_movement(a, b, what):
    for name in ("x", "feat", "d_out", "d_c", "dx"):
        ta, tb = getattr(a.rec, name), getattr(b.rec, name)
        assert len(ta) == len(tb) and len(ta) > 0, (what, name, len(ta), len(tb))
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert torch.equal(u, v), "%s: %s[%d] differs" % (what, name, i)
    assert torch.equal(a.mu, b.mu) and torch.equal(a.lv, b.lv), what
    assert torch.equal(a.states[0], b.states[0]) and torch.equal(a.states[1], b.states[1]), what + ": generator state"


@pytest.fixture
def restore_noise():
    yield
    host.set_noise(host.DeviceNoise())


def _held_to_float64(ref, bound_run, runs, tag):
    """Every summed gradient of each of ``runs`` (label -> run) within twice the error ``bound_run`` shows against ``ref``."""
    for name in sorted(ref):
        if name not in bound_run.grads:
            continue
        err_b = (bound_run.grads[name].double().cpu() - ref[name]).abs().max().item()
        for label, r in runs.items():
            err = (r.grads[name].double().cpu() - ref[name]).abs().max().item()
            print("TXT-FUSED %s: %s bound-run err %.3e %s err %.3e (scale %.3e)" % (tag, name, err_b, label, err, ref[name].abs().max().item()))
            assert err <= 2 * err_b, (tag, name, label, err, err_b)


@pytest.mark.parametrize("frozen", [False, True], ids=["trainable", "frozen"])
@pytest.mark.parametrize("noise_cls", [host.DeviceNoise, host.HostNoise], ids=["device", "host"])
@pytest.mark.parametrize("drop_out", [0.0, 0.3], ids=["noout", "out"])
@pytest.mark.parametrize("drop_in", [0.0, 0.3], ids=["noin", "in"])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_encoder_matches_stock_path(batch, layers, drop_in, drop_out, noise_cls, frozen, monkeypatch, restore_noise):
    lens, rows = BATCHES[batch]
    B = len(lens)
    aligned = noise_cls is host.HostNoise
    tag = "%s L%d in %.1f out %.1f %s" % (batch, layers, drop_in, drop_out, noise_cls.__name__)
    torch.manual_seed(2)
    vocab = types.SimpleNamespace(size=VOCAB, padding_idx=PAD)
    enc = networks_v2.TxtEncoder(vocab, E, H, C_DIM, N_CLS, layers, dropout_in=drop_in, dropout_out=drop_out).to(DEV).train()
    enc.embed_tokens.weight.requires_grad = not frozen
    g = torch.Generator().manual_seed(4)
    style, g_mu, g_lv = (_dev(torch.randn(B, S, generator=g)) for _ in range(3))
    tokens, lens_t = _dev(torch.tensor(rows)), torch.tensor(lens)
    run = lambda fused, seed: _run(enc, fused, noise_cls, seed, style, tokens, lens_t, g_mu, g_lv, monkeypatch)

    stock, fused = run(0, 21), run(1, 21)
    _same_movement(stock, fused, "first pass")
    assert set(stock.grads) == set(fused.grads) and ("embed_tokens.weight" in fused.grads) == (not frozen)
    # the draws: dropout_in's mask, one mask per layer boundary, parity mode's unused draw on the padded memory
    assert len(fused.masks) == (drop_in > 0) + (drop_out > 0) * ((layers - 1) + aligned)

    # summed gradients: both paths against float64, the fused one within twice the stock path's own error
    ref = _ref64(enc, style, tokens, lens, fused.masks, aligned, g_mu, g_lv)
    _held_to_float64(ref, stock, {"fused": fused}, tag)
    # and since every sum is taken by the same reduction on the same values, shapes and strides on either path: the same bits
    for name in sorted(fused.grads):
        assert torch.equal(stock.grads[name], fused.grads[name]), name
    if not frozen:
        assert torch.equal(fused.grads["embed_tokens.weight"][PAD], torch.zeros(E, device=DEV))

    # the same module again: the same bits
    again = run(1, 21)
    _same_movement(fused, again, "second pass")
    for name in fused.grads:
        assert torch.equal(fused.grads[name], again.grads[name]), name

    # Step the weights (in place: the parameters' versions move) and run again.  Both paths read the transposed w_hh and the bias sum
    # through ops._lstm_derived, so comparing them with each other cannot show an entry kept from before the step.  The reference
    # here is a run that keeps nothing (every derived tensor rebuilt from the stepped values) and float64 on the stepped weights:
    # a transpose or a bias sum one step old moves mu and every gradient by far more than rounding.
    with torch.no_grad():
        for i, p in enumerate(enc.parameters()):
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)).to(DEV))
    stock2, fused2 = run(0, 22), run(1, 22)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_lstm_derived", lambda kind, owners, stamp, build: build())
        mp.setattr(ops, "_LSTM_DERIVED", {})
        fresh = run(0, 22)
    _same_movement(fresh, stock2, "after the step, stock path against nothing kept")
    _same_movement(fresh, fused2, "after the step, fused path against nothing kept")
    assert not torch.equal(fused2.mu, fused.mu)
    assert set(fresh.grads) == set(stock2.grads) == set(fused2.grads)
    for name in sorted(fresh.grads):
        assert torch.equal(fresh.grads[name], stock2.grads[name]), name
        assert torch.equal(fresh.grads[name], fused2.grads[name]), name
    ref2 = _ref64(enc, style, tokens, lens, fused2.masks, aligned, g_mu, g_lv)
    _held_to_float64(ref2, fresh, {"stock": stock2, "fused": fused2}, tag + " after the step")
    # The bound run itself against float64, so that the 2x rule above does not rest on a run nobody checked: 1e-4 of the tensor's
    # scale is ~1700 roundings of 2^-24 -- more than the <= 5 recurrent steps and the few-hundred-term products of these shapes can
    # accumulate --, while weights moved by 0.05 against a scale of 0.25 change a gradient by percents.
    for name in sorted(ref2):
        if name in fresh.grads:
            err = (fresh.grads[name].double().cpu() - ref2[name]).abs().max().item()
            assert err <= 1e-4 * max(ref2[name].abs().max().item(), 1e-3), (name, err)


def test_int32_tokens_take_the_fused_path(monkeypatch):
    """nn.Embedding takes int32 ids; the kernels read int64: the fused path converts, and gives what it gives for int64 ids."""
    lens, rows = BATCHES["b3"]
    monkeypatch.setattr(ops, "TXT_FUSED", 1)
    torch.manual_seed(2)
    enc = networks_v2.TxtEncoder(types.SimpleNamespace(size=VOCAB, padding_idx=PAD), E, H, C_DIM, N_CLS, 2).to(DEV).eval()
    style = _dev(torch.randn(len(lens), S, generator=torch.Generator().manual_seed(4)))
    tokens = _dev(torch.tensor(rows))
    with torch.no_grad():
        a, b = enc(style, tokens, torch.tensor(lens)), enc(style, tokens.int(), torch.tensor(lens))
    assert torch.equal(a[0].flat, b[0].flat) and torch.equal(a[1].flat, b[1].flat)
