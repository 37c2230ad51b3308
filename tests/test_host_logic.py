"""CPU-only checks of the host side of the product: module tree / state_dict contract, seeded
initialisation equal to the reference's, the C-ABI library's exported symbols, and that the
product refuses to compute on CPU tensors (no fallback)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from hipdwc import _lib, host, ops, synth
from solver import Solver

T = torch.from_numpy


def _build(cfg, seed=1234):
    torch.manual_seed(seed)
    s = Solver(cfg, torch.device("cpu"), None)
    s.copy_nets()
    return s


def test_tiny_init_equals_reference(golden_dir):
    tiny = np.load(os.path.join(golden_dir, "tiny_step.npz"))
    s = _build(synth.make_config(image_size=32, tiny=True))
    for prefix, mod in (("init/gen/", s.gen), ("init/dis/", s.dis)):
        sd = mod.state_dict()
        want = {k[len(prefix):]: tiny[k] for k in tiny.files if k.startswith(prefix)}
        assert list(sd.keys()) == list(want.keys()) or set(sd.keys()) == set(want.keys())
        for k, v in want.items():
            assert sd[k].shape == v.shape, k
            assert torch.equal(sd[k], T(v)), k          # same seed, same draw order: bit-exact
    # and the random stream is left exactly where the reference leaves it
    assert torch.equal(torch.get_rng_state(), T(tiny["rng_state_after_init"]))


@pytest.mark.parametrize("S", [64, 128])
def test_full_init_checksums(golden_dir, S):
    with open(os.path.join(golden_dir, "init_checksums.json")) as f:
        ref = json.load(f)["S%d" % S]
    s = _build(synth.make_config(image_size=S))
    assert sum(p.numel() for p in s.gen.parameters()) == ref["n_gen"]
    assert sum(p.numel() for p in s.dis.parameters()) == ref["n_dis"]
    for name, mod in (("gen", s.gen), ("dis", s.dis)):
        sd = mod.state_dict()
        assert set(sd.keys()) == set(ref[name].keys())
        for k, (s1, s2) in ref[name].items():
            t = sd[k].double()
            assert abs(float(t.sum()) - s1) <= 1e-9 * max(1.0, abs(s1)), k
            assert abs(float((t * t).sum()) - s2) <= 1e-9 * max(1.0, abs(s2)), k


def test_solver_api_surface():
    s = _build(synth.make_config(image_size=32, tiny=True))
    for m in ("dis_update", "gen_update", "smooth_moving", "update_learning_rate", "update_attention_status", "sample",
              "copy_nets", "resume", "save", "init_network", "forward"):
        assert callable(getattr(s, m))
    assert hasattr(s, "gen_copy") and hasattr(s, "dis_copy")
    assert s.gen_opt.param_groups[0]["lr"] == 1e-4 and s.gen_opt.param_groups[0]["betas"] == (0.5, 0.999)
    assert s.gen_opt.param_groups[0]["weight_decay"] == 1e-4
    n_adain = sum(1 for m in s.gen.dec.modules() if m.__class__.__name__ == "AdaptiveInstanceNorm2d")
    assert n_adain == 2 * 2 and s.gen.get_num_adain_params(s.gen.dec) == n_adain * 2 * 32
    s.update_attention_status(0)
    assert s.use_attention is False
    s.update_attention_status(10000)
    assert s.use_attention is True
    lr0 = s.gen_opt.param_groups[0]["lr"]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # scheduler stepped before any optimizer step (no GPU here)
        s.update_learning_rate()
    assert s.gen_opt.param_groups[0]["lr"] == lr0          # StepLR(100000): unchanged after one step


def test_ema_matches_reference_rule():
    s = _build(synth.make_config(image_size=32, tiny=True))
    with torch.no_grad():
        for p in s.gen.parameters():
            p.add_(0.5)
    before = [p.detach().clone() for p in s.gen_copy.parameters()]
    s.smooth_moving()
    for p, c0, c1 in zip(s.gen.parameters(), before, s.gen_copy.parameters()):
        torch.testing.assert_close(c1, torch.lerp(p.detach(), c0, 0.999), rtol=0, atol=1e-7)


def test_sampling_layout_and_host_noise(golden_dir):
    ops_g = np.load(os.path.join(golden_dir, "ops_golden.npz"))
    from tools import dist_sampling_split, asign_label
    host.set_noise(host.HostNoise())
    try:
        torch.manual_seed(99)
        z = dist_sampling_split(T(ops_g["sample/c"]), 8, 0.5, torch.device("cpu"))
        assert torch.equal(z, T(ops_g["sample/z_seed99"]))
        # dropout masks: same stream consumption as F.dropout on the tensor itself
        torch.manual_seed(5)
        x = torch.randn(3, 7)
        st = torch.get_rng_state()
        a = torch.nn.functional.dropout(x, 0.1, True)
        torch.set_rng_state(st)
        b = host.noise().dropout(x, 0.1, True)
        assert torch.equal(a, b)
    finally:
        host.set_noise(host.DeviceNoise())
    lab = torch.tensor([[0.0, 1.0]])
    assert torch.equal(asign_label(lab), torch.tensor([[-1.0, 1.0]]))


def test_gmm_losses_match_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "ops_golden.npz"))
    from gmm import gmm_kl_distance_sp, gmm_earth_mover_distance_sp
    mus, lvs, c = list(T(g["gmm/mus"])), list(T(g["gmm/logvars"])), T(g["gmm/c"])
    assert abs(float(gmm_kl_distance_sp(mus, lvs, c, torch.tensor(0.25))) - float(g["gmm/kl"])) < 1e-4
    assert abs(float(gmm_earth_mover_distance_sp(mus, c)) - float(g["gmm/em"])) < 1e-5


def test_library_exports_every_declared_symbol():
    """include/dwcgan_hip.h <-> libdwcgan_hip.so <-> the ctypes table, no compute calls."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    declared = set(re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES.keys())
    assert os.path.exists(_lib.LIB_PATH), "build the library first: make -C dwc-gan_amd/csrc"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.load().dwc_version() >= 1
    # pure host-side helper entry points (no kernel launch)
    assert _lib.load().dwc_instnorm_ws_bytes(2, 64, 16) >= 2 * 2 * 16 * 4
    assert _lib.load().dwc_conv2d_bwd_weight_ws_bytes(2, 8, 8, 16, 16, 3, 3, 1, 1) >= 9 * 16 * 16 * 4


def test_plan_queries_agree_with_the_scratch_sizes():
    """dwc_[bf16_]conv2d_fwd_plan / _bwd_weight_plan are host code: they answer without a device, refuse what the entry points refuse,
    and their splits are the ones the *_ws_bytes functions size the scratch for."""
    lib = _lib.load()
    shapes = [(3, 4, 4, 256, 128, 4, 4, 1, 0), (7, 32, 32, 256, 512, 1, 1, 1, 0), (4, 96, 96, 16, 192, 3, 3, 1, 1), (2, 21, 19, 16, 40, 3, 3, 1, 1),
              (8, 32, 32, 16, 64, 3, 3, 1, 1), (2, 64, 64, 128, 256, 4, 4, 2, 1)]
    for pre, bk, slab in (("dwc_", 32, 32), ("dwc_bf16_", 64, 64)):
        for s in shapes:
            B, H, W, ci, co, kh, kw, st, p = s
            M = B * ((H + 2 * p - kh) // st + 1) * ((W + 2 * p - kw) // st + 1)
            K = kh * kw * ci
            bm, bn, splits, kt = _lib.plan(pre + "conv2d_fwd_plan", *s)
            assert bm > 0 and bn > 0 and splits >= 1 and (splits - 1) * kt < (K + bk - 1) // bk <= splits * kt
            assert getattr(lib, pre + "conv2d_fwd_ws_bytes")(*s) == (splits * M * co * 4 if splits > 1 else 0)
            wbn, wsplits, chunk, wide = _lib.plan(pre + "conv2d_bwd_weight_plan", *s)
            assert wbn >= min(co, 128) and chunk % slab == 0              # (one column tile up to 128 channels)
            assert (wsplits - 1) * chunk < M <= wsplits * chunk and wide in (0, 1)
            assert not (wide and wsplits == 1)                             # (a single range has nothing to reduce widely)
            assert getattr(lib, pre + "conv2d_bwd_weight_ws_bytes")(*s) == wsplits * K * co * 4
        out = (ctypes.c_int * 4)(*([-7] * 4))
        for bad in ((0, 8, 8, 16, 16, 3, 3, 1, 1), (1, 8, 8, 12, 16, 3, 3, 1, 1), (1, 8, 8, 16, 16, 3, 3, 3, 1), (1, 8, 8, 16, 16, 3, 3, 1, 8),
                    (1, 8, 8, 16, 18, 3, 3, 1, 1)):
            assert getattr(lib, pre + "conv2d_fwd_plan")(*bad, out) == _lib.EINVAL
            assert getattr(lib, pre + "conv2d_bwd_weight_plan")(*bad, out) == _lib.EINVAL
        assert list(out) == [-7] * 4
        assert getattr(lib, pre + "conv2d_fwd_plan")(1, 8, 8, 16, 16, 3, 3, 1, 1, None) == _lib.EINVAL
    # 4 output channels: a multiple of 4 is enough for fp32, bf16 needs 8
    assert lib.dwc_conv2d_fwd_plan(1, 8, 8, 16, 4, 3, 3, 1, 1, out) == 0
    assert lib.dwc_bf16_conv2d_fwd_plan(1, 8, 8, 16, 4, 3, 3, 1, 1, out) == _lib.EINVAL
    assert lib.dwc_bf16_conv2d_bwd_weight_plan(1, 8, 8, 16, 4, 3, 3, 1, 1, out) == _lib.EINVAL


def test_no_cpu_fallback():
    x = torch.randn(1, 4, 8, 8)
    w = torch.randn(8, 4, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.conv2d(x, w, None, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.instance_norm(torch.randn(1, 8, 4, 4))
    import networks.networks as nets
    blk = nets.Conv2dBlock(4, 8, 3, 1, 1, norm="in", activation="relu", pad_type="reflect")
    with pytest.raises(RuntimeError, match="no CPU"):
        blk(x)


def test_checkpoint_save_resume_roundtrip(tmp_path):
    """reference solver.py:359-413: file names and keys ({'a': gen}, {'b': dis}, *_avg copies, optimizer.pt), the
    iteration parsed back from the name, schedulers advanced to it."""
    from solver import Solver
    cfg = synth.make_config(image_size=32, tiny=True)
    cfg["step_size"], cfg["gamma"] = 3, 0.5
    torch.manual_seed(5)
    a = Solver(cfg, torch.device("cpu"), None)
    a.copy_nets()
    with torch.no_grad():
        for p in a.gen_copy.parameters():
            p.mul_(0.5)
    a.save(str(tmp_path), 6)
    names = sorted(os.listdir(tmp_path))
    assert names == ["dis_00000007.pt", "dis_00000007_avg.pt", "gen_00000007.pt", "gen_00000007_avg.pt", "optimizer.pt"]
    assert set(torch.load(tmp_path / "gen_00000007.pt").keys()) == {"a"} and set(torch.load(tmp_path / "dis_00000007.pt").keys()) == {"b"}
    torch.manual_seed(99)
    b = Solver(cfg, torch.device("cpu"), None)
    it = b.resume(str(tmp_path), cfg)
    assert it == 7
    # the newest file whose name contains 'gen' is the averaged copy, exactly as in the reference (sorted()[-1])
    src = a.gen_copy.state_dict()
    for k, v in b.gen.state_dict().items():
        assert torch.equal(v, src[k]), k
    # the reference rebuilds the schedulers with last_epoch=iterations AND steps them `iterations` times under torch != 0.4.1
    # (solver.py:374-379): the learning rate after resume is that recipe's, reproduced here on a dummy optimiser
    dummy = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=cfg["lr"])
    dummy.param_groups[0]["initial_lr"] = cfg["lr"]
    sch = torch.optim.lr_scheduler.StepLR(dummy, step_size=3, gamma=0.5, last_epoch=7)
    for _ in range(7):
        sch.step()
    assert b.gen_opt.param_groups[0]["lr"] == pytest.approx(dummy.param_groups[0]["lr"])
    assert b.dis_opt.param_groups[0]["lr"] == pytest.approx(dummy.param_groups[0]["lr"])


def test_resume_can_reload_optimizer_state(tmp_path):
    """save() writes optimizer.pt like the reference (solver.py:413); resume(load_optimizer=True) restores Adam's moments
    and step counts from it (the reference leaves that reload commented out, solver.py:370-372), the default does not."""
    from solver import Solver
    cfg = synth.make_config(image_size=32, tiny=True)
    torch.manual_seed(5)
    a = Solver(cfg, torch.device("cpu"), None)
    a.copy_nets()
    g = torch.Generator().manual_seed(1)
    for opt in (a.gen_opt, a.dis_opt):            # fabricate a non-trivial optimiser state (FusedAdam.step itself needs the GPU)
        for p in opt.param_groups[0]["params"]:
            opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=g),
                            "exp_avg_sq": torch.rand(p.shape, generator=g)}
    a.save(str(tmp_path), 6)
    b = Solver(cfg, torch.device("cpu"), None)
    assert b.resume(str(tmp_path), cfg) == 7 and len(b.gen_opt.state) == 0
    c = Solver(cfg, torch.device("cpu"), None)
    assert c.resume(str(tmp_path), cfg, load_optimizer=True) == 7
    for oa, oc in ((a.gen_opt, c.gen_opt), (a.dis_opt, c.dis_opt)):
        pa, pc = oa.param_groups[0]["params"], oc.param_groups[0]["params"]
        assert len(oc.state) == len(pa)
        for x, y in zip(pa, pc):
            assert float(oc.state[y]["step"]) == 7.0
            assert torch.equal(oc.state[y]["exp_avg"], oa.state[x]["exp_avg"])
            assert torch.equal(oc.state[y]["exp_avg_sq"], oa.state[x]["exp_avg_sq"])
        assert oc.param_groups[0]["lr"] == pytest.approx(b.gen_opt.param_groups[0]["lr"])
    with pytest.raises(FileNotFoundError):
        os.remove(tmp_path / "optimizer.pt")
        Solver(cfg, torch.device("cpu"), None).resume(str(tmp_path), cfg, load_optimizer=True)


def _device_noise_checks(device):
    """DeviceNoise is the random source of bench.py and of real training (HostNoise only exists for parity runs): layout,
    moments and keep rates of its three draws, against the reference's definitions (tools.py:65-70, networks_v2.py:119,222)."""
    noise = host.DeviceNoise()
    g = torch.Generator().manual_seed(3)
    B, A, c_dim = 64, 8, 8
    # layout: with a vanishing stddev the sample IS the centre, so the attribute-major [B, A*c_dim] order is exact to see
    mu = torch.randn(B, A, generator=g).to(device)
    z = noise.style_sample(mu, c_dim, 1e-7)
    assert z.shape == (B, A * c_dim) and z.device.type == torch.device(device).type
    assert torch.allclose(z.view(B, A, c_dim), mu.unsqueeze(2).expand(B, A, c_dim), atol=1e-5)
    # same layout as the parity source (same call, host generator)
    zh = host.HostNoise().style_sample(mu.cpu(), c_dim, 1e-7)
    assert torch.allclose(z.cpu(), zh, atol=1e-5)
    # moments: N(mu, stddev^2) per entry
    mu2 = torch.tensor([[-1.0, 1.0] * 4]).repeat(4096, 1).to(device)
    z2 = noise.style_sample(mu2, c_dim, 0.5).view(4096, A, c_dim) - mu2.unsqueeze(2)
    n = z2.numel()
    assert abs(float(z2.mean())) < 5 * 0.5 / n ** 0.5
    assert abs(float(z2.std()) - 0.5) < 5 * 0.5 / (2 * n) ** 0.5
    assert abs(float((z2 ** 4).mean()) / 0.5 ** 4 - 3.0) < 0.1              # Gaussian kurtosis
    per_attr = z2.mean(dim=(0, 2))
    assert float(per_attr.abs().max()) < 6 * 0.5 / (4096 * c_dim) ** 0.5   # no attribute column is biased
    # draws differ between calls and between rows
    assert not torch.equal(noise.style_sample(mu, c_dim, 0.5), noise.style_sample(mu, c_dim, 0.5))
    # dropout mask: values {0, 1/(1-p)}, keep rate 1-p
    for p in (0.1, 0.5):
        m = noise.dropout_mask((2048, 256), p, torch.device(device))
        vals = torch.unique(m).cpu()
        assert vals.numel() == 2 and float(vals[0]) == 0.0 and abs(float(vals[1]) - 1.0 / (1.0 - p)) < 1e-6
        keep = float((m > 0).float().mean())
        assert abs(keep - (1.0 - p)) < 5 * (p * (1 - p) / m.numel()) ** 0.5
        x = torch.randn(2048, 256, generator=g).to(device)
        y = noise.dropout(x, p, True)
        kept = y != 0
        assert torch.allclose(y[kept], x[kept] / (1.0 - p), rtol=1e-6) and abs(float(kept.float().mean()) - (1.0 - p)) < 0.01
    assert torch.equal(noise.dropout(x, 0.1, False), x)                     # eval mode: identity


def test_device_noise_layout_and_moments_cpu():
    torch.manual_seed(11)
    _device_noise_checks("cpu")


@pytest.mark.gpu
def test_device_noise_layout_and_moments_gpu():
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    _device_noise_checks("cuda:0")


def test_dis_update_tapes_content_only_when_a_gen_update_follows():
    """reference train.py:105 runs gen_update every n_critic-th iteration: the content code dis_update tapes for it is only
    taped on those iterations, and an unmodified caller (attribute left at 1) is detected after one unconsumed tape."""
    import inspect
    src = inspect.getsource(Solver.dis_update)
    assert "n_critic" in src and "_tape_content" in src
