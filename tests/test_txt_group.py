"""The grouped text encoder on the device (csrc/txt_glue.hip ``dwc_txt_regroup_*``, hipdwc/txt.py ``regroup``, networks_v2.TxtEncoder
``group`` / ``sync``, Solver ``txt_group`` / ``sync_txt``).  The layout identities of the stock form are
tests/test_txt_regroup.py; here the kernels are held to that form and the modules to the reference.

Bounds.  Movement is compared with ``torch.equal``.  Against the fixture tests/golden/txt_group.npz (recorded from the reference,
called once per group, by tests/golden/make_golden_txt_group.py) ``mu`` / ``logvar`` are held to ``close(rel=1e-4)`` and every gradient
to the rule of tests/test_txt_embed.py: its error against the float64 record at most twice the error of the EXISTING ungrouped
``forward`` (``TXT_FUSED=0``) called once per group, floored at one fp32 spacing of the record's largest value.  Launches of different
batch size (virtual ranks against the concatenated batch, ``txt_group=1`` against batch-1 calls) are held to 1e-4 of the tensor's
scale, the bound tests/test_txt_fused.py puts on fp32 runs of this encoder: ~1700 roundings of 2^-24.
"""
import os
import types

import numpy as np
import pytest
import torch

import guarded_alloc as ga
from hipdwc import _lib, host, ops, synth, txt
from networks import networks_v2
from test_txt_regroup import GROUPS, LAYERS, RANKS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "txt_group.npz")
WIDTHS = [6, 8, 600]                                 # 2H: the scalar path, the 16-byte path, the shipped width
PAD = 0


def close(a, b, rel, msg):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err, lim = (a - b).abs().max().item(), rel * b.abs().max().item()
    print("%s: max err %.3e, limit %.3e" % (msg, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e" % (msg, err, lim)


@pytest.fixture
def restore_noise():
    yield
    host.set_noise(host.DeviceNoise())


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels against the stock form
# ---------------------------------------------------------------------------------------------------------------------------------
def _twice(fn, shape, *args):
    """The export into two guarded, poisoned buffers in a row -> the (equal, fully written) result."""
    outs = []
    for _ in range(2):
        out = ga.guarded(shape, torch.float32, DEV)
        assert fn(args[0].data_ptr(), out.data_ptr(), *args[1:], ops._stream()) == 0
        outs.append(out)
    ga.verify()
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("width", WIDTHS)
def test_group_exports_against_the_stock_form(width):
    lib = _lib.load()
    H = width // 2
    for L in LAYERS:
        for B, G in GROUPS:
            g = torch.Generator().manual_seed(L + 10 * B + G)
            feat = ga.guarded_input(torch.randn(B, 2 * L * width, generator=g).to(DEV))
            ct = ga.guarded_input(torch.randn(B, 2 * L * width, generator=g).to(DEV))
            rows = txt.group_rows(L, B, G).to(DEV)
            want = feat.reshape(-1, width).index_select(0, rows).reshape(B, -1)
            want_d = torch.empty_like(ct).reshape(-1, width).index_copy_(0, rows, ct.reshape(-1, width)).reshape(B, -1)
            assert torch.equal(_twice(lib.dwc_txt_regroup_fwd, feat.shape, feat, L, B, H, G), want), (L, B, G)
            assert torch.equal(_twice(lib.dwc_txt_regroup_bwd, ct.shape, ct, L, B, H, G), want_d), (L, B, G)
            if G != B:
                f = feat.clone().requires_grad_(True)
                out = txt.regroup(f, group=G, layers=L)
                assert type(out.grad_fn).__name__ == "_RegroupBackward" and torch.equal(out, want)
                assert torch.equal(torch.autograd.grad(out, f, ct)[0], want_d)


@pytest.mark.parametrize("width", WIDTHS)
def test_rank_exports_against_the_stock_form(width):
    lib = _lib.load()
    H = width // 2
    for L in LAYERS:
        for W, Bl in RANKS:
            g = torch.Generator().manual_seed(L + 10 * W + Bl)
            feats = ga.guarded_input(torch.randn(W, Bl, 2 * L * width, generator=g).to(DEV))
            cts = ga.guarded_input(torch.randn(W, Bl, 2 * L * width, generator=g).to(DEV))
            outs, grads = [], []
            for r in range(W):
                fwd, bwd = (t.to(DEV) for t in txt.rank_rows(L, W, Bl, r))
                want = feats.reshape(-1, width).index_select(0, fwd).reshape(Bl, -1)
                want_d = cts.reshape(-1, width).index_select(0, bwd).reshape(Bl, -1)
                outs.append(_twice(lib.dwc_txt_regroup_rank_fwd, want.shape, feats, L, W, Bl, H, r))
                grads.append(_twice(lib.dwc_txt_regroup_rank_bwd, want.shape, cts, L, W, Bl, H, r))
                assert torch.equal(outs[-1], want) and torch.equal(grads[-1], want_d), (L, W, Bl, r)
            # the ranks together are a permutation of the global buffer: its adjoint is its inverse
            back = torch.stack(grads)
            again = torch.cat([_twice(lib.dwc_txt_regroup_rank_fwd, (Bl, 2 * L * width), back, L, W, Bl, H, r) for r in range(W)])
            assert torch.equal(again, cts.reshape(W * Bl, -1)), (L, W, Bl)


def test_exports_take_the_scalar_path_on_pointers_off_16_bytes():
    lib = _lib.load()
    L, B, G, width = 2, 6, 2, 8
    n = B * 2 * L * width
    src = ga.guarded_input(torch.randn(n + 1, generator=torch.Generator().manual_seed(3)).to(DEV))
    dst = ga.guarded((n + 1,), torch.float32, DEV)
    feat = src[1:].view(B, -1)
    assert feat.data_ptr() % 16 == 4
    assert lib.dwc_txt_regroup_fwd(feat.data_ptr(), dst[1:].data_ptr(), L, B, width // 2, G, ops._stream()) == 0
    ga.verify()
    want = feat.reshape(-1, width).index_select(0, txt.group_rows(L, B, G).to(DEV)).reshape(-1)
    assert torch.equal(dst[1:], want) and torch.isnan(dst[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------
E, HID, C_DIM, N_CLS, SEQ = 12, 16, 4, 3, 7
S = C_DIM * N_CLS


def _encoder(layers=2, vocab_size=11, drop=0.1):
    return networks_v2.TxtEncoder(types.SimpleNamespace(size=vocab_size, padding_idx=PAD), E, HID, C_DIM, N_CLS, layers,
                                  dropout_in=drop, dropout_out=drop)


def _tokens(lens, vocab_size, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(1, vocab_size, (len(lens), SEQ), generator=g)
    for b, n in enumerate(lens):
        rows[b, n:] = PAD
    return rows


def _features(enc, monkeypatch):
    """Records what ``enc._heads`` is given."""
    seen = []
    heads = enc._heads

    def spy(feat):
        seen.append(feat.detach().clone())
        return heads(feat)
    monkeypatch.setattr(enc, "_heads", spy)
    return seen


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "stock"])
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_group_is_the_regroup_of_the_ungrouped_feature_buffer(layers, fused, monkeypatch):
    monkeypatch.setattr(ops, "TXT_FUSED", fused)
    torch.manual_seed(5)
    enc = _encoder(layers).to(DEV).eval()
    seen = _features(enc, monkeypatch)
    lens = [3, 7, 1, 5, 2, 4]
    B = len(lens)
    tokens, lens_t = _tokens(lens, 11, 6).to(DEV), torch.tensor(lens)
    style = torch.randn(B, S, generator=torch.Generator().manual_seed(7)).to(DEV)
    emb = enc.embed_tokens.weight.detach()[tokens]
    assert enc.group is None and enc.sync is None and not [k for k in enc.state_dict() if "group" in k or "sync" in k]
    with torch.no_grad():
        for call in (lambda **k: enc(style, tokens, lens_t, **k), lambda **k: enc.forward_embed(style, emb, lens_t, **k)):
            del seen[:]
            call()
            plain, = seen
            for G in (1, 2, 3, 6):
                del seen[:]
                mu, _ = call(group=G)
                want = txt._RegroupTorch.apply(plain, layers, G, None)
                assert torch.equal(seen[0], want) and (G == B or not torch.equal(want, plain)), G
                enc.group = G                                    # the attribute does what the argument does; the argument wins
                assert torch.equal(call()[0].flat, mu.flat)
                assert torch.equal(seen[-1], want)
                del seen[:]
                call(group=B)
                assert torch.equal(seen[0], plain)
                enc.group = None


def _run(enc, fused, style, tokens, lens, g_mu, g_lv, monkeypatch, group=None, per_group=None):
    """forward + backward of the loss; ``per_group``: the ungrouped forward once per slice of that many samples instead."""
    monkeypatch.setattr(ops, "TXT_FUSED", int(fused))
    for p in enc.parameters():
        p.grad = None
    sty = style.clone().requires_grad_(True)
    if per_group:
        outs = [enc(sty[a:a + per_group], tokens[a:a + per_group], lens[a:a + per_group]) for a in range(0, len(lens), per_group)]
        mu, lv = torch.cat([m.flat for m, _ in outs]), torch.cat([v.flat for _, v in outs])
    else:
        mu, lv = enc(sty, tokens, lens, group=group)
        mu, lv = mu.flat, lv.flat
    ((mu * g_mu).sum() + (lv * g_lv).sum()).backward()
    grads = {n: p.grad.detach().clone() for n, p in enc.named_parameters() if p.grad is not None}
    grads["style"] = sty.grad.detach().clone()
    return types.SimpleNamespace(mu=mu.detach(), lv=lv.detach(), grads=grads)


@pytest.mark.parametrize("G", [1, 2, 3])
def test_grouped_encoder_against_the_reference_fixture(G, monkeypatch, restore_noise):
    """One ``group=G`` call on the 6 recorded samples, fused and ``TXT_FUSED=0``, against the reference called once per group.  The
    bound run of the gradients is the existing ungrouped ``forward`` (``TXT_FUSED=0``) called once per group.  Every error is printed
    before it is asserted."""
    fx = np.load(FIXTURE)
    get = lambda k: torch.from_numpy(fx[k])
    enc = _encoder()
    state = {k[len("state/"):]: get(k) for k in fx.files if k.startswith("state/")}
    enc.load_state_dict(state)
    enc = enc.to(DEV).eval()
    lens, style, tokens = get("lengths"), get("style").to(DEV), get("tokens").to(DEV)
    g_mu, g_lv = get("r_mu").to(DEV), get("r_lv").to(DEV)
    ref, flat, o = {}, get("g%d/g64" % G), 0
    for name, shape in [(k, v.shape) for k, v in state.items()] + [("style", style.shape)]:
        ref[name] = flat[o:o + shape.numel()].reshape(shape)
        o += shape.numel()
    assert o == flat.numel()
    bound = _run(enc, 0, style, tokens, lens, g_mu, g_lv, monkeypatch, per_group=G)
    runs = {"fused": _run(enc, 1, style, tokens, lens, g_mu, g_lv, monkeypatch, group=G),
            "stock": _run(enc, 0, style, tokens, lens, g_mu, g_lv, monkeypatch, group=G)}
    failed = []
    for label, r in runs.items():
        close(r.mu, get("g%d/mu" % G), 1e-4, "G%d %s mu" % (G, label))
        close(r.lv, get("g%d/lv" % G), 1e-4, "G%d %s logvar" % (G, label))
        assert set(r.grads) == set(ref) == set(bound.grads)
        for name in sorted(ref):
            err_b = (bound.grads[name].double().cpu() - ref[name]).abs().max().item()
            err = (r.grads[name].double().cpu() - ref[name]).abs().max().item()
            floor = float(np.spacing(np.float32(ref[name].abs().max().item())))
            print("TXT-GROUP fixture G%d %s: %s bound-run err %.3e err %.3e floor %.3e (scale %.3e)"
                  % (G, label, name, err_b, err, floor, ref[name].abs().max().item()))
            assert torch.isfinite(r.grads[name]).all()
            if not err <= max(2 * err_b, floor):
                failed.append((label, name, err, err_b, floor))
    assert not failed, failed


class QueueSync:
    """The ``sync`` of one virtual rank: the k-th all_gather returns the k-th precomputed [W, ...] array with this rank's own
    contribution at ``rank`` (first call: the forward's feature buffers, second: the backward's output gradients)."""

    def __init__(self, world, rank, queue):
        self.world, self.rank, self.force, self.queue, self.seen = world, rank, True, list(queue), []

    def all_gather(self, t):
        out = self.queue.pop(0).clone()
        assert out.shape[0] == self.world and out.shape[1:] == t.shape
        self.seen.append(t.detach().clone())
        out[self.rank] = t
        return out


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "stock"])
@pytest.mark.parametrize("W,Bl", [(2, 2), (2, 3), (3, 2), (3, 3)])
def test_virtual_ranks_against_the_concatenated_batch(W, Bl, fused, monkeypatch):
    monkeypatch.setattr(ops, "TXT_FUSED", fused)
    torch.manual_seed(8)
    enc = _encoder().to(DEV).eval()
    seen = _features(enc, monkeypatch)
    B = W * Bl
    lens = [3, 7, 1, 5, 2, 4, 6, 3, 2][:B]
    g = torch.Generator().manual_seed(9)
    tokens, lens_t = _tokens(lens, 11, 10).to(DEV), torch.tensor(lens)
    style, g_mu, g_lv = (torch.randn(B, S, generator=g).to(DEV) for _ in range(3))
    part = lambda t, r: t[r * Bl:(r + 1) * Bl]

    # one device, the concatenated batch
    want = _run(enc, fused, style, tokens, lens_t, g_mu, g_lv, monkeypatch)
    feat_global = seen.pop()
    # the other ranks' buffers and cotangents first: the local feature buffers, then the gradient each rank's heads send back
    with torch.no_grad():
        for r in range(W):
            enc(part(style, r), part(tokens, r), part(lens_t, r))
    feats = torch.stack(seen)
    del seen[:]
    outs, cots = [], []
    for r in range(W):
        fwd, _ = txt.rank_rows(2, W, Bl, r)
        out = feats.reshape(-1, 2 * HID).index_select(0, fwd.to(DEV)).reshape(Bl, -1).requires_grad_(True)
        mu, lv = enc._heads(out)
        cots.append(torch.autograd.grad((mu.flat * part(g_mu, r)).sum() + (lv.flat * part(g_lv, r)).sum(), out)[0])
        outs.append(out.detach())
    del seen[:]
    cots = torch.stack(cots)
    close(torch.cat(outs), feat_global, 1e-4, "W%d Bl%d features of the ranks against the concatenated batch" % (W, Bl))

    mus, lvs, d_style, summed = [], [], [], {}
    for r in range(W):
        for p in enc.parameters():                               # (a rank's gradients are taken on their own and added here: the two
            p.grad = None                                        # bias gradients of a layer share storage, nothing may accumulate into them)
        enc.sync = QueueSync(W, r, [feats, cots])
        sty = part(style, r).clone().requires_grad_(True)
        mu, lv = enc(sty, part(tokens, r), part(lens_t, r))
        assert torch.equal(seen.pop(), outs[r])                  # features: equal after the regroup of identical buffers
        ((mu.flat * part(g_mu, r)).sum() + (lv.flat * part(g_lv, r)).sum()).backward()
        for name, p in enc.named_parameters():
            summed[name] = p.grad.detach().clone() if r == 0 else summed[name] + p.grad
        assert not enc.sync.queue and len(enc.sync.seen) == 2
        assert torch.equal(enc.sync.seen[0], feats[r]) and torch.equal(enc.sync.seen[1], cots[r])
        mus.append(mu.flat.detach())
        lvs.append(lv.flat.detach())
        d_style.append(sty.grad)
    enc.sync = None
    close(torch.cat(mus), want.mu, 1e-4, "W%d Bl%d mu" % (W, Bl))
    close(torch.cat(lvs), want.lv, 1e-4, "W%d Bl%d logvar" % (W, Bl))
    close(torch.cat(d_style), want.grads["style"], 1e-4, "W%d Bl%d style gradient" % (W, Bl))
    for name in sorted(summed):
        close(summed[name], want.grads[name], 1e-4, "W%d Bl%d summed gradient %s" % (W, Bl, name))
    # group together with an active sync is refused
    enc.sync = QueueSync(W, 0, [])
    with pytest.raises(ValueError, match="exclude each other"):
        enc(part(style, 0), part(tokens, 0), part(lens_t, 0), group=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the Solver
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_NAMES = ["loss_dis", "loss_dis_all", "loss_ds", "loss_gen_adv", "loss_gen_cycrecon_x", "loss_gen_recon_c_fake",
              "loss_gen_recon_c_rand", "loss_gen_recon_c_real", "loss_gen_recon_s_fake", "loss_gen_recon_s_rand",
              "loss_gen_recon_s_real", "loss_gen_recon_x", "loss_gen_total", "loss_gen_vgg", "loss_kl_trg", "loss_kl_x"]


def _trainer(cfg, dev):
    host.set_noise(host.HostNoise())
    torch.manual_seed(1234)
    from solver import Solver
    return Solver(cfg, dev, None).to(dev)


def test_solver_forward_txt_group_1_is_batch_1_calls(restore_noise):
    dev = torch.device(DEV)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    trainer = _trainer(cfg, dev).eval()
    assert trainer.use_attention                                 # the blend x*a + x_real*(1-a) is part of what is compared
    batch = {k: v.to(dev) for k, v in synth.make_batch(3, 32, seed=5).items()}
    x, t, n = batch["x_real"], batch["txt"], batch["txt_lens"]
    with torch.no_grad():
        got = trainer(x, t, n, txt_group=1)
        mixed = trainer(x, t, n)
        want = torch.cat([trainer(x[i:i + 1], t[i:i + 1], n[i:i + 1]) for i in range(3)])
    close(got, want, 1e-4, "forward(txt_group=1) against three batch-1 calls")
    assert (mixed - want).abs().max() > 10 * (got - want).abs().max()        # the reference layout mixes the sentences


def _two_iterations(dev, cfg, batch, dp_kwargs=None):
    trainer = _trainer(cfg, dev)
    trainer.copy_nets()
    if dp_kwargs is not None:
        trainer.enable_data_parallel(**dp_kwargs)
    grads, losses = {}, []
    for it in range(2):
        torch.manual_seed(99 + it)
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, it)
        trainer.dis_update(*a)
        grads["dis%d" % it] = {k: p.grad.detach().clone() for k, p in trainer.dis.named_parameters() if p.grad is not None}
        trainer.gen_update(*a)
        grads["gen%d" % it] = {k: p.grad.detach().clone() for k, p in trainer.gen.named_parameters() if p.grad is not None}
        losses.append({k: float(getattr(trainer, k)) for k in LOSS_NAMES})
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
    torch.cuda.synchronize()
    return trainer, grads, losses


def test_tiny_solver_with_txt_group_1(restore_noise):
    dev = torch.device(DEV)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    batch = {k: v.to(dev) for k, v in synth.make_batch(3, 32, seed=5).items()}
    plain, g_plain, _ = _two_iterations(dev, cfg, batch)
    cfg["gen"]["txt_group"] = 1
    grouped, g_grouped, losses = _two_iterations(dev, cfg, batch)
    assert plain.gen.enc_txt.group is None and grouped.gen.enc_txt.group == 1 and grouped.gen_copy.enc_txt.group == 1
    assert list(plain.gen.state_dict()) == list(grouped.gen.state_dict())
    for it in range(2):
        assert len(losses[it]) == 16 and all(np.isfinite(v) for v in losses[it].values()), losses[it]
        names = [k for k, _ in grouped.gen.enc_txt.named_parameters()]
        assert names and all("enc_txt." + k in g_grouped["gen%d" % it] for k in names)
        assert all(torch.isfinite(g_grouped["gen%d" % it]["enc_txt." + k]).all() for k in names)
    assert any(not torch.equal(g_plain["gen0"][k], g_grouped["gen0"][k]) for k in g_plain["gen0"])      # another function is trained


def test_one_rank_rccl_sync_txt_equals_plain_trainer(tmp_path, monkeypatch, restore_noise):
    """enable_data_parallel(sync_txt=True) with DWC_FORCE_DP=1 on a world_size-1 RCCL group, in this process (file rendezvous): the
    rank form with W = 1 and real all-gathers.  Two iterations reproduce the plain trainer's gradients and parameters exactly."""
    import torch.distributed as dist
    from hipdwc import syncbn
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    batch = {k: v.to(dev) for k, v in synth.make_batch(3, 32, seed=5).items()}
    monkeypatch.setenv("DWC_FORCE_DP", "1")
    dist.init_process_group("nccl", device_id=dev, init_method="file://" + str(tmp_path / "rdv"), rank=0, world_size=1)
    try:
        plain, g_plain, l_plain = _two_iterations(dev, cfg, batch)
        dp_, g_dp, l_dp = _two_iterations(dev, cfg, batch, dict(bucket_bytes=64 << 10, sync_txt=True))
    finally:
        dist.destroy_process_group()
    sync = dp_.gen.enc_txt.sync
    assert plain.gen.enc_txt.sync is None
    assert isinstance(sync, syncbn.GroupSync) and sync.force and sync.world == 1
    print("text encoder: %d all-gathers, %d bytes" % (sync.calls, sync.bytes))
    assert sync.calls >= 4 and "sync" not in " ".join(dp_.gen.state_dict())
    assert l_plain == l_dp
    for step in g_plain:
        assert set(g_plain[step]) == set(g_dp[step]), step
        for k in g_plain[step]:
            assert torch.equal(g_plain[step][k], g_dp[step][k]), (step, k)
    for (k, p), (_, q) in zip(list(plain.gen.named_parameters()) + list(plain.dis.named_parameters()),
                              list(dp_.gen.named_parameters()) + list(dp_.dis.named_parameters())):
        assert torch.equal(p, q), k
