"""``TxtEncoder.forward_embed``: the text encoder from the caller's word vectors (csrc/txt_glue.hip ``dwc_txt_operand_embed_*``,
hipdwc/txt.py, networks/networks_v2.py; reference networks_v2.py:256-293).

CPU: the two new exports agree between header, ctypes table and library and refuse bad arguments before any launch; the method
refuses bad inputs before any device work; the fixture tests/golden/txt_embed.npz (recorded from the reference by
tests/golden/make_golden_embed.py) is consistent with itself.

GPU, S 8, H 16, seq_len 7; embedding widths 12, 260 (past one pass of the 256-thread column loop) and 300 (the shipped width);
batches [3, 5, 1] (unsorted, a length of 1, t_max < seq_len), [4] (batch 1) and [5, 3, 3, 1] (ties): the exports through the C ABI
into guarded, poisoned buffers against the stock tensor expression and the token kernels; the module against ``forward`` on the
matching tokens (a table with unique rows, every live slot its own id: the table gradient gathered at the tokens IS the gradient of
the embedded words, one row added to zero); NaN / Inf behind the lengths; ``ops.TXT_FUSED`` 1 against 0; the fixture.

Bounds.  Movement is compared with ``torch.equal``.  Summed gradients (style rows, LSTM weights) follow the rule of
tests/test_txt_fused.py: at most twice the stock path's own error against a float64 evaluation of the same expression, per tensor,
both printed.  Against the fixture the outputs are held to ``close(rel=1e-4)`` (tests/test_hip_parity.py: txt mu / txt logvar) and each
gradient's error against the float64 record to twice the error of ``forward`` (``TXT_FUSED=0``) on the same tokens against that
record, floored at one fp32 spacing of the record's largest value (what an fp32 tensor of that scale can resolve).  The fixture's own
fp32 records are held to 1e-4 of the float64 record's scale: ~1700 roundings of 2^-24, more than <= 5 recurrent steps and products
of at most 64 terms accumulate (the bound test_txt_fused.py puts on its bound run).
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import guarded_alloc as ga
from hipdwc import _lib, host, ops, txt
from networks import networks_v2

DEV = "cuda:0"
S, H, SEQ, PAD = 8, 16, 7, 0
C_DIM, N_CLS = 2, 4                          # style width S = C_DIM * N_CLS
WIDTHS = [12, 260, 300]
LENS = {"b3": [3, 5, 1], "b1": [4], "b4": [5, 3, 3, 1]}
NEW_SYMBOLS = {"dwc_txt_operand_embed_fwd", "dwc_txt_operand_embed_bwd"}
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "txt_embed.npz")
FIX_CASES = ("b4", "b1")
FIX_GRADS = ("emb", "style", "lstm.weight_ih_l0", "lstm.weight_hh_l1_reverse", "fcs.0.weight")


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_embed_symbols_header_table_library():
    header = open(os.path.join(os.path.dirname(HERE), "include", "dwcgan_hip.h")).read()
    declared = set(re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SIGNATURES)
    assert not any("syncbn" in n or "batchnorm" in n for n in NEW_SYMBOLS)
    assert int(re.search(r"#define\s+DWC_ABI_VERSION\s+(\d+)\b", header).group(1)) == _lib.ABI_VERSION == 11      # additive
    lib = _lib.load()
    assert lib.dwc_version() == 11
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n


def test_embed_exports_refuse_bad_arguments_before_any_launch():
    """No device is touched: the pointers are dummies and every call must return DWC_EINVAL from the host-side checks."""
    lib = _lib.load()
    p = 4096

    def fwd(emb=p, order=p, lens=p, mask=None, style=p, x=p, t_max=3, B=2, seq_len=7, E=12, S=8):
        return lib.dwc_txt_operand_embed_fwd(emb, order, lens, mask, style, x, t_max, B, seq_len, E, S, None)

    def bwd(dxa=p, dxb=None, order=p, lens=p, mask=None, d_cat=p, d_emb=p, t_max=3, B=2, seq_len=7, E=12, S=8):
        return lib.dwc_txt_operand_embed_bwd(dxa, dxb, order, lens, mask, d_cat, d_emb, t_max, B, seq_len, E, S, None)

    bad_fwd = [dict(emb=None), dict(order=None), dict(lens=None), dict(x=None), dict(style=None), dict(t_max=0), dict(t_max=-1),
               dict(t_max=8), dict(B=0), dict(B=-3), dict(E=0), dict(S=-1), dict(seq_len=0, t_max=0),
               dict(seq_len=65536, B=65536), dict(seq_len=1 << 30, B=2)]
    for kw in bad_fwd:
        assert fwd(**kw) == _lib.EINVAL, kw
    bad_bwd = [dict(dxa=None), dict(order=None), dict(lens=None), dict(d_cat=None, d_emb=None), dict(t_max=0), dict(t_max=8),
               dict(B=0), dict(E=0), dict(S=-1), dict(S=0), dict(seq_len=65536, B=65536), dict(seq_len=1 << 30, B=2)]
    for kw in bad_bwd:
        assert bwd(**kw) == _lib.EINVAL, kw


def _encoder(E, hidden, layers, vocab_size, drop_in=0.0, drop_out=0.0, bidirectional=True):
    return networks_v2.TxtEncoder(types.SimpleNamespace(size=vocab_size, padding_idx=PAD), E, hidden, C_DIM, N_CLS, layers,
                                  dropout_in=drop_in, dropout_out=drop_out, bidirectional=bidirectional)


def test_forward_embed_refuses_bad_inputs():
    torch.manual_seed(1)
    enc = _encoder(12, H, 1, 11).eval()
    style, emb = torch.randn(3, S), torch.randn(3, SEQ, 12)
    bad = [(emb[0], [3, 5, 1]),                                    # rank 2
           (emb[None], [3, 5, 1]),                                 # rank 4
           (torch.randn(3, SEQ, 13), [3, 5, 1]),                   # another width than embed_dim
           (emb, [3, 5]), (emb, torch.tensor([3, 5, 1, 2])),       # len(lengths) != B
           (emb, [3, 0, 1]), (emb, torch.tensor([3, SEQ + 1, 1])), (emb, [-1, 2, 2])]
    for e, lens in bad:
        with pytest.raises(ValueError):
            enc.forward_embed(style, e, lens)
    one_way = _encoder(12, H, 1, 11, bidirectional=False).eval()
    with pytest.raises(NotImplementedError):
        one_way.forward_embed(style, emb, [3, 5, 1])


def test_fixture_is_self_consistent():
    fx = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(HERE, "golden", "tiny_bn_step.npz"))
    for case in FIX_CASES:
        get = lambda k: fx["%s/%s" % (case, k)]
        lens = get("lengths").tolist()
        assert lens == sorted(lens, reverse=True)
        assert get("emb").shape == (len(lens), SEQ, 12)
        for b, n in enumerate(lens):
            assert np.isnan(get("emb")[b, n:]).all() and np.isfinite(get("emb")[b, :n]).all()
        # forward_embed on embed_tokens(tokens) IS forward on the tokens
        assert np.array_equal(get("mu"), get("mu_tok")) and np.array_equal(get("lv"), get("lv_tok"))
        for kind in ("g", "g64"):
            g = get(kind + "/emb")
            for b, n in enumerate(lens):
                assert (g[b, n:] == 0).all() and np.abs(g[b, :n]).max() > 0
        for k in ("mu", "lv"):
            assert np.abs(get(k) - get(k + "64")).max() <= 1e-4 * np.abs(get(k + "64")).max(), (case, k)
        for name in FIX_GRADS:
            a, b = get("g/" + name), get("g64/" + name)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), (case, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the exports through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _dev(t):
    return t.to(DEV)


def _indices(lens):
    lens_sorted, order = torch.sort(torch.tensor(lens), descending=True)
    unsort = torch.sort(order)[1]
    i32 = lambda t: _dev(t.to(torch.int32))
    return types.SimpleNamespace(order=i32(order), unsort=i32(unsort), lens=i32(lens_sorted), order64=_dev(order), unsort64=_dev(unsort),
                                 lens64=_dev(lens_sorted), t_max=int(lens_sorted[0]))


def _unique_tokens(lens):
    """[B, SEQ] int64: every live slot its own id (1 ..), the padding id behind each length; and the vocabulary size."""
    rows = torch.zeros(len(lens), SEQ, dtype=torch.int64)
    for b, n in enumerate(lens):
        rows[b, :n] = 1 + b * SEQ + torch.arange(n)
    return rows, 1 + len(lens) * SEQ


def _tails(emb, lens, value):
    out = emb.clone()
    for b, n in enumerate(lens):
        out[b, n:] = value
    return out


def _stock_operand(emb, style, ix, mask):
    """The stock tensor expression of the layer-1 operand (networks_v2.TxtEncoder.forward_embed / _stock)."""
    x = emb.transpose(0, 1).index_select(1, ix.order64)
    live = torch.arange(SEQ, device=DEV).view(-1, 1, 1) < ix.lens64.view(1, -1, 1)
    x = torch.where(live, x, torch.zeros((), device=DEV))
    x = x * mask if mask is not None else x
    return torch.cat([x, style.index_select(0, ix.order64).expand(SEQ, -1, -1)], -1)[:ix.t_max]


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("batch", sorted(LENS))
@pytest.mark.parametrize("E", WIDTHS)
def test_operand_embed_exports(E, batch, masked):
    lib = _lib.load()
    lens = LENS[batch]
    B, ix = len(lens), _indices(lens)
    g = torch.Generator().manual_seed(3)
    tokens, V = _unique_tokens(lens)
    table = torch.randn(V, E, generator=g)
    table[PAD] = 0
    style = ga.guarded_input(_dev(torch.randn(B, S, generator=g)))
    mask = ga.guarded_input(_dev((torch.rand((SEQ, B, E), generator=g) > 0.3).float() / 0.7)) if masked else None
    table, tokens = _dev(table), _dev(tokens)
    emb = ga.guarded_input(_tails(table[tokens], lens, float("nan")))

    x = ga.guarded((ix.t_max, B, E + S), torch.float32, DEV)
    assert lib.dwc_txt_operand_embed_fwd(emb.data_ptr(), ix.order.data_ptr(), ix.lens.data_ptr(), ops._p(mask), style.data_ptr(),
                                         x.data_ptr(), ix.t_max, B, SEQ, E, S, ops._stream()) == 0
    x_tok = ga.guarded((ix.t_max, B, E + S), torch.float32, DEV)
    assert lib.dwc_txt_operand_fwd(table.data_ptr(), tokens.data_ptr(), ix.order.data_ptr(), ops._p(mask), style.data_ptr(),
                                   x_tok.data_ptr(), ix.t_max, B, SEQ, E, S, V, ops._stream()) == 0
    assert torch.equal(x, _stock_operand(emb, style, ix, mask))
    assert torch.equal(x, x_tok) and torch.equal(torch.signbit(x), torch.signbit(x_tok))

    dxa, dxb = (ga.guarded_input(_dev(torch.randn(ix.t_max, B, E + S, generator=g))) for _ in range(2))
    for second in (dxb, None):
        d_cat, d_emb = ga.guarded((SEQ, B, E + S), torch.float32, DEV), ga.guarded((B, SEQ, E), torch.float32, DEV)
        assert lib.dwc_txt_operand_embed_bwd(dxa.data_ptr(), ops._p(second), ix.order.data_ptr(), ix.lens.data_ptr(), ops._p(mask),
                                             d_cat.data_ptr(), d_emb.data_ptr(), ix.t_max, B, SEQ, E, S, ops._stream()) == 0
        emb_in = emb.clone().requires_grad_(True)
        want, = torch.autograd.grad(_stock_operand(emb_in, style, ix, mask), [emb_in], dxa + second if second is not None else dxa)
        assert not torch.isnan(d_emb).any() and torch.equal(d_emb, want)
        dead = torch.ones(B, SEQ, dtype=torch.bool, device=DEV)
        for b, n in enumerate(lens):
            dead[b, :n] = False
        assert (d_emb[dead] == 0).all() and not torch.signbit(d_emb[dead]).any()         # +0.0 behind the lengths and from t_max on
        assert (d_emb[~dead] != 0).sum() > 0
        d_cat_tok, d_emb_tok = ga.guarded((SEQ, B, E + S), torch.float32, DEV), ga.guarded((SEQ, B, E), torch.float32, DEV)
        assert lib.dwc_txt_operand_bwd(dxa.data_ptr(), ops._p(second), tokens.data_ptr(), ix.order.data_ptr(), ops._p(mask),
                                       d_cat_tok.data_ptr(), d_emb_tok.data_ptr(), None, ix.t_max, B, SEQ, E, S, ops._stream()) == 0
        assert torch.equal(d_cat[:, :, E:], d_cat_tok[:, :, E:]) and not torch.isnan(d_cat[:, :, E:]).any()
        assert torch.isnan(d_cat[:, :, :E]).all()                                         # (columns the kernel does not own)
    # one output alone (a constant embedding / a style that needs no gradient); neither: refused
    d_cat, d_emb = ga.guarded((SEQ, B, E + S), torch.float32, DEV), ga.guarded((B, SEQ, E), torch.float32, DEV)
    assert lib.dwc_txt_operand_embed_bwd(dxa.data_ptr(), None, ix.order.data_ptr(), ix.lens.data_ptr(), ops._p(mask),
                                         d_cat.data_ptr(), None, ix.t_max, B, SEQ, E, S, ops._stream()) == 0
    assert lib.dwc_txt_operand_embed_bwd(dxa.data_ptr(), None, ix.order.data_ptr(), ix.lens.data_ptr(), ops._p(mask),
                                         None, d_emb.data_ptr(), ix.t_max, B, SEQ, E, S, ops._stream()) == 0
    assert torch.equal(d_cat[:, :, E:], d_cat_tok[:, :, E:]) and torch.equal(d_emb, want)
    assert lib.dwc_txt_operand_embed_bwd(dxa.data_ptr(), None, ix.order.data_ptr(), ix.lens.data_ptr(), None, None, None,
                                         ix.t_max, B, SEQ, E, S, ops._stream()) == _lib.EINVAL
    ga.verify()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the module
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def restore_noise():
    yield
    host.set_noise(host.DeviceNoise())


def _recording_noise():
    class Rec(host.DeviceNoise):
        def __init__(self):
            super().__init__()
            self.masks = []

        def dropout_mask(self, shape, p, device):
            m = super().dropout_mask(shape, p, device)
            self.masks.append(m)
            return m
    return Rec()


def _run(enc, fused, seed, style, lens, g_mu, g_lv, monkeypatch, emb=None, tokens=None, emb_grad=True):
    """One forward + backward of ``forward_embed`` (emb) or ``forward`` (tokens): outputs, generator states, masks, gradients."""
    monkeypatch.setattr(ops, "TXT_FUSED", int(fused))
    noise = host.set_noise(_recording_noise())
    for p in enc.parameters():
        p.grad = None
    sty = style.clone().requires_grad_(True)
    torch.manual_seed(seed)
    if emb is not None:
        e = emb.clone().requires_grad_(emb_grad)
        mu, lv = enc.forward_embed(sty, e, lens)
    else:
        mu, lv = enc(sty, tokens, lens)
    states = (torch.cuda.get_rng_state(DEV), torch.get_rng_state())
    ((mu.flat * g_mu).sum() + (lv.flat * g_lv).sum()).backward()
    grads = {n: p.grad.detach().clone() for n, p in enc.named_parameters() if p.grad is not None}
    grads["style"] = sty.grad.detach().clone()
    if emb is not None and emb_grad:
        grads["emb"] = e.grad.detach().float().clone()
    return types.SimpleNamespace(mu=mu.flat.detach(), lv=lv.flat.detach(), masks=noise.masks, states=states, grads=grads)


def _same_bits(a, b, what):
    assert torch.equal(a.mu, b.mu) and torch.equal(a.lv, b.lv), what
    assert torch.equal(a.states[0], b.states[0]) and torch.equal(a.states[1], b.states[1]), what + ": generator state"
    assert set(a.grads) == set(b.grads), (what, sorted(a.grads), sorted(b.grads))
    for name in sorted(a.grads):
        assert torch.equal(a.grads[name], b.grads[name]), "%s: gradient %s" % (what, name)


def _setup(E, batch, layers, drop_in, drop_out, train):
    lens = LENS[batch]
    B = len(lens)
    tokens, V = _unique_tokens(lens)
    torch.manual_seed(2)
    enc = _encoder(E, H, layers, V, drop_in, drop_out).to(DEV)
    enc.train(train)
    g = torch.Generator().manual_seed(4)
    style, g_mu, g_lv = (_dev(torch.randn(B, S, generator=g)) for _ in range(3))
    tokens = _dev(tokens)
    emb = enc.embed_tokens.weight.detach()[tokens]               # zeros behind the lengths: the padding row
    return types.SimpleNamespace(enc=enc, lens=lens, lens_t=torch.tensor(lens), B=B, tokens=tokens, emb=emb, style=style, g_mu=g_mu,
                                 g_lv=g_lv)


MODES = {"eval": (0.3, 0.3, False), "in": (0.3, 0.0, True), "out": (0.0, 0.3, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("batch", sorted(LENS))
@pytest.mark.parametrize("E", WIDTHS)
def test_forward_embed_is_forward_on_the_tokens(E, batch, layers, mode, monkeypatch, restore_noise):
    c = _setup(E, batch, layers, *MODES[mode])
    tok = _run(c.enc, 1, 21, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, tokens=c.tokens)
    emb = _run(c.enc, 1, 21, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=c.emb)
    drop_in, drop_out, train = MODES[mode]
    assert len(emb.masks) == len(tok.masks) == train * ((drop_in > 0) + (drop_out > 0) * (layers - 1))
    # the table gradient gathered at the tokens (unique ids: one row added to zero; the padding row is zero) is the embedding gradient
    tok.grads["emb"] = tok.grads.pop("embed_tokens.weight")[c.tokens]
    assert "embed_tokens.weight" not in emb.grads
    _same_bits(tok, emb, "forward_embed against forward")
    # lengths as a list and as a device tensor: the same call
    again = _run(c.enc, 1, 21, c.style, c.lens, c.g_mu, c.g_lv, monkeypatch, emb=c.emb)
    _same_bits(emb, again, "lengths as a list")
    again = _run(c.enc, 1, 21, c.style, _dev(c.lens_t), c.g_mu, c.g_lv, monkeypatch, emb=c.emb.double())
    _same_bits(emb, again, "lengths on the device, float64 embeddings cast by the method")


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "stock"])
@pytest.mark.parametrize("batch", sorted(LENS))
@pytest.mark.parametrize("E", WIDTHS)
def test_nothing_depends_on_what_lies_behind_the_lengths(E, batch, fused, monkeypatch, restore_noise):
    c = _setup(E, batch, 2, 0.3, 0.3, True)
    zero = _run(c.enc, fused, 23, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=c.emb)
    for t in [zero.mu, zero.lv] + list(zero.grads.values()):
        assert torch.isfinite(t).all()
    dead = torch.ones(c.B, SEQ, dtype=torch.bool, device=DEV)
    for b, n in enumerate(c.lens):
        dead[b, :n] = False
    for value in (float("nan"), float("inf"), -float("inf")):
        run = _run(c.enc, fused, 23, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=_tails(c.emb, c.lens, value))
        _same_bits(zero, run, "tails of %r" % value)
        assert (run.grads["emb"][dead] == 0).all() and not torch.signbit(run.grads["emb"][dead]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", sorted(LENS))
@pytest.mark.parametrize("E", WIDTHS)
def test_fused_against_stock_path(E, batch, monkeypatch, restore_noise):
    from test_txt_fused import _held_to_float64, _ref64
    c = _setup(E, batch, 2, 0.3, 0.3, True)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = txt.operand_embed_fwd, txt.operand_embed_bwd

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(txt, "operand_embed_fwd", count("fwd", fwd))
    monkeypatch.setattr(txt, "operand_embed_bwd", count("bwd", bwd))
    emb = _tails(c.emb, c.lens, float("nan"))
    stock = _run(c.enc, 0, 25, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=emb)
    assert calls == {"fwd": 0, "bwd": 0}
    fused = _run(c.enc, 1, 25, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=emb)
    assert calls == {"fwd": 1, "bwd": 1}
    assert torch.equal(stock.mu, fused.mu) and torch.equal(stock.lv, fused.lv)
    assert torch.equal(stock.states[0], fused.states[0]) and torch.equal(stock.states[1], fused.states[1])
    assert torch.equal(stock.grads["emb"], fused.grads["emb"])
    assert set(stock.grads) == set(fused.grads) and len(fused.masks) == 2
    # float64 of the same expression with the fp32 runs' masks, through the table: its gradient gathered at the (unique) tokens is
    # the embedding gradient
    ref = _ref64(c.enc, c.style, c.tokens, c.lens, fused.masks, False, c.g_mu, c.g_lv)
    ref["emb"] = ref.pop("embed_tokens.weight")[c.tokens.cpu()]
    assert set(ref) <= set(fused.grads)
    _held_to_float64(ref, stock, {"fused": fused}, "TXT-EMBED E%d %s" % (E, batch))


def _fixture_encoder(fx):
    enc = networks_v2.TxtEncoder(types.SimpleNamespace(size=11, padding_idx=PAD), 12, 8, C_DIM, N_CLS, 2, dropout_in=0.1, dropout_out=0.1)
    enc.load_state_dict({k[len("state/"):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("state/")})
    return enc.to(DEV).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIX_CASES)
def test_forward_embed_against_the_reference_fixture(case, monkeypatch, restore_noise):
    """The recorded reference (eval mode, NaN behind the lengths) on both paths; the bound run of the gradients is ``forward`` on the
    recorded tokens with ``TXT_FUSED=0``.  Every error is printed before it is asserted."""
    from test_hip_parity import close
    fx = np.load(FIXTURE)
    get = lambda k: torch.from_numpy(fx["%s/%s" % (case, k)])
    enc = _fixture_encoder(fx)
    lens, style, emb, tokens = get("lengths"), _dev(get("style")), _dev(get("emb")), _dev(get("tokens"))
    g_mu, g_lv = _dev(get("r_mu")), _dev(get("r_lv"))
    order = torch.sort(lens, descending=True)[1]
    unsort = _dev(torch.sort(order)[1])

    # bound run: the existing stock-op forward on the tokens; the gradient of its embedded words ([seq_len, B, E], sorted) by a hook
    kept = {}

    def keep_grad(mod, args, out):
        out.register_hook(lambda gr: kept.update(g=gr.detach().clone()))
    handle = enc.embed_tokens.register_forward_hook(keep_grad)
    bound = _run(enc, 0, 27, style, lens, g_mu, g_lv, monkeypatch, tokens=tokens)
    handle.remove()
    bound.grads["emb"] = kept["g"].index_select(1, unsort).transpose(0, 1)
    runs = {"fused": _run(enc, 1, 27, style, lens, g_mu, g_lv, monkeypatch, emb=emb),
            "stock": _run(enc, 0, 27, style, lens, g_mu, g_lv, monkeypatch, emb=emb)}
    for label, r in runs.items():
        close(r.mu, get("mu"), rel=1e-4, msg="%s %s mu" % (case, label))
        close(r.lv, get("lv"), rel=1e-4, msg="%s %s logvar" % (case, label))
        for name in FIX_GRADS:
            ref = get("g64/" + name)
            err_b = (bound.grads[name].double().cpu() - ref).abs().max().item()
            err = (r.grads[name].double().cpu() - ref).abs().max().item()
            floor = float(np.spacing(np.float32(ref.abs().max().item())))
            print("TXT-EMBED fixture %s %s: %s bound-run err %.3e err %.3e floor %.3e (scale %.3e)"
                  % (case, label, name, err_b, err, floor, ref.abs().max().item()))
            assert torch.isfinite(r.grads[name]).all()
            assert err <= max(2 * err_b, floor), (case, label, name, err, err_b, floor)


@pytest.mark.gpu
def test_runs_repeat_and_a_constant_embedding_forms_no_gradient(monkeypatch, restore_noise):
    c = _setup(300, "b3", 2, 0.3, 0.3, True)
    emb = _tails(c.emb, c.lens, float("nan"))
    a = _run(c.enc, 1, 29, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=emb)
    b = _run(c.enc, 1, 29, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=emb)
    _same_bits(a, b, "two consecutive runs")
    seen = []
    bwd = txt.operand_embed_bwd

    def spy(*args, need_style=True, need_emb=True):
        out = bwd(*args, need_style=need_style, need_emb=need_emb)
        seen.append((need_style, need_emb, out[0] is not None, out[1] is not None))
        return out
    monkeypatch.setattr(txt, "operand_embed_bwd", spy)
    const = _run(c.enc, 1, 29, c.style, c.lens_t, c.g_mu, c.g_lv, monkeypatch, emb=emb, emb_grad=False)
    assert seen == [(True, False, True, False)]
    a.grads.pop("emb")
    _same_bits(a, const, "embeddings that need no gradient")


@pytest.mark.gpu
def test_forward_embed_refuses_more_layers_than_the_kernels_take():
    enc = _encoder(12, H, _lib.TXT_MAX_LAYERS + 1, 11).to(DEV).eval()
    with pytest.raises(ValueError, match="DWC_TXT_MAX_LAYERS"):
        enc.forward_embed(_dev(torch.randn(1, S)), _dev(torch.randn(1, SEQ, 12)), [4])
