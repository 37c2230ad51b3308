"""The device half of the input pipeline (csrc/image_u8.hip, hipdwc.u8image, data_loader.get_loader(device_transform=True);
DESIGN.md 25): uint8 HWC crops -> internal image buffer, bit-equal to the CPU chain (PIL resize, to-float, normalise) + pack_image.

Reference: ``Image.resize(..., Image.BILINEAR)`` of the installed Pillow and ``ImageTransform``'s normalise expression, on the CPU.
Every comparison is ``torch.equal`` / 0 differing bytes: PIL's 8-bit resize is integer arithmetic, and the normalised value of a
byte comes from a table built with the loader's own expression, so there is nothing to tolerate.  The one toleranced check is the
solver-level one: losses of a step fed from the device mode against a step fed from the default loader, bounded by 4x what two
runs of the DEFAULT loader differ by (existing code), floored at one fp32 spacing of the value.
"""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

import data_loader
from data_ios.celeba_data import CelebA
from hipdwc import _lib, ops, u8image

import guarded_alloc                            # noqa: E402  (tests/ is on the path: conftest)
from test_input_pipeline import GOLD, _attr_file

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))

# (Hin, Win, hout, wout)
GEOMETRIES = [(178, 178, 128, 128),     # the real CelebA case
              (178, 178, 64, 64),
              (178, 178, 256, 256),     # upscale, ksize 3
              (178, 178, 32, 32),       # ksize 13
              (178, 178, 96, 96),
              (170, 170, 128, 128),
              (128, 128, 64, 64),
              (64, 64, 128, 128),
              (100, 100, 100, 100),     # identity weights
              (37, 37, 16, 16),         # ragged row bytes
              (20, 31, 7, 9),           # non-square, band remainder
              (218, 178, 157, 128),
              (5, 5, 16, 16),           # every window clipped at an edge
              (3, 3, 2, 2)]
# the two other plans of the kernel: a 16-row band's source rows exceed the LDS and an 8-row band's fit; a single output row's
# source rows exceed it (13 rows x 2048 x 3 bytes), so the 8-bit intermediate goes to caller scratch
PLAN_GEOMETRIES = [(64, 1024, 32, 1024), (12, 2048, 2, 2048)]
CONTENTS = ("uniform", "binary", "white")
B = 3
_gid = lambda g: "%dx%d-to-%dx%d" % g


def make_u8(geom, content, batch=B):
    hin, win = geom[:2]
    rng = np.random.RandomState(hin * 7919 + win * 31 + geom[2] + CONTENTS.index(content))
    if content == "uniform":
        a = rng.randint(0, 256, (batch, hin, win, 3), dtype=np.uint8)
    elif content == "binary":
        a = (rng.randint(0, 2, (batch, hin, win, 3)) * 255).astype(np.uint8)
    else:
        a = np.full((batch, hin, win, 3), 255, dtype=np.uint8)
    return torch.from_numpy(a)


def pil_resize(u8, hout, wout):
    """uint8 [B, H, W, 3] -> uint8 [B, hout, wout, 3] through the installed Pillow."""
    return torch.from_numpy(np.stack([np.asarray(Image.fromarray(img).resize((wout, hout), Image.BILINEAR)) for img in u8.numpy()]))


def cpu_chain(u8, hout, wout):
    """What the default loader mode makes of the crops: PIL resize, then ImageTransform's expression.  fp32 NCHW."""
    return pil_resize(u8, hout, wout).permute(0, 3, 1, 2).float().div_(255.0).sub_(0.5).div_(0.5)


_REFERENCE = {}


def reference(geom, content):
    """(u8 crops, cpu_chain of them), computed once per case and shared; nobody writes to either."""
    key = (geom, content)
    if key not in _REFERENCE:
        u8 = make_u8(geom, content)
        _REFERENCE[key] = (u8, cpu_chain(u8, geom[2], geom[3]))
    return _REFERENCE[key]


def resample_pass(img, start, coef, axis):
    """One pass of the integer rule along ``axis`` of a uint8 array, from the windows of ``resample_table``."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(start),) + src.shape[1:], dtype=np.int64)
    for i in range(len(start)):
        taps = min(coef.shape[1], src.shape[0] - int(start[i]))
        acc = np.tensordot(coef[i, :taps].astype(np.int64), src[start[i]:start[i] + taps], axes=1)
        assert np.abs(acc).max() + (1 << 21) < 2 ** 31                 # the kernel's 32-bit sums hold it
        out[i] = np.clip(((1 << 21) + acc) >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", GEOMETRIES + PLAN_GEOMETRIES, ids=_gid)
def test_resample_table_restates_pil(geom):
    hin, win, hout, wout = geom
    ystart, ycoef = u8image.resample_table(hin, hout)
    xstart, xcoef = u8image.resample_table(win, wout)
    assert ystart.dtype == ycoef.dtype == np.int32 and ystart.shape == (hout,) and xcoef.shape[0] == wout
    for n_in, n_out, start, coef in ((hin, hout, ystart, ycoef), (win, wout, xstart, xcoef)):
        assert coef.shape[1] == 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1
        assert (np.diff(start) >= 0).all() and start.min() >= 0 and start.max() < n_in      # what the kernel's band walk relies on
        assert (coef >= 0).all() and (np.abs(coef.sum(1) - (1 << 22)) <= coef.shape[1]).all()
    for content in CONTENTS:
        u8 = make_u8(geom, content)
        got = np.stack([resample_pass(resample_pass(img, xstart, xcoef, 1), ystart, ycoef, 0) for img in u8.numpy()])
        differing = int((got != pil_resize(u8, hout, wout).numpy()).sum())
        print("%s %s: %d differing bytes (Pillow %s)" % (_gid(geom), content, differing, Image.__version__))
        assert differing == 0


def test_value_table_is_the_loaders_expression():
    lut = u8image.value_table()
    assert lut.dtype == torch.float32 and lut.shape == (256,) and float(lut[0]) == -1.0 and float(lut[255]) == 1.0
    img = Image.fromarray(np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2))
    via_loader = data_loader.ImageTransform(16, 16, flip=False, square=False)(img)
    assert torch.equal(via_loader[0].reshape(-1), lut)


def _celeba_dir(tmp_path, n_images, seed):
    ap = str(tmp_path / "attr.txt")
    _attr_file(ap)
    g = np.random.RandomState(seed)
    for mode in ("train", "test"):
        probe = CelebA(str(tmp_path), ap, GOLD["selected"], None, mode)
        for name, _ in (probe.train_dataset if mode == "train" else probe.test_dataset)[:n_images]:
            Image.fromarray(g.randint(0, 256, (218, 178, 3), dtype=np.uint8)).save(str(tmp_path / name), quality=95)
    return ap


def _first_batch(tmp_path, ap, image_size, n, mode, seed, **kw):
    loader = data_loader.get_loader(str(tmp_path), 178, image_size, n, ap, GOLD["selected"], "CelebA", mode, num_workers=0, **kw)
    sub = torch.utils.data.Subset(loader.dataset, list(range(n)))
    random.seed(seed)
    return next(iter(torch.utils.data.DataLoader(sub, batch_size=n, shuffle=False, num_workers=0)))


def test_loader_device_mode_delivers_the_crops_of_the_default_mode(tmp_path):
    ap = _celeba_dir(tmp_path, 8, seed=3)
    default = _first_batch(tmp_path, ap, 128, 8, "train", seed=11)
    crops = _first_batch(tmp_path, ap, 128, 8, "train", seed=11, device_transform=True)
    assert crops[0].dtype == torch.uint8 and tuple(crops[0].shape) == (8, 178, 178, 3) and crops[0].is_contiguous()
    assert default[0].dtype == torch.float32 and tuple(default[0].shape) == (8, 3, 128, 128)
    for a, b in zip(default[1:], crops[1:]):                             # labels, target labels, tokens, lengths
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert torch.equal(cpu_chain(crops[0], 128, 128), default[0])        # the same flips too
    # the seed-11 draws flip some of the eight images and not others, so the equality above has seen both
    files = [os.path.join(str(tmp_path), name) for name, _ in CelebA(str(tmp_path), ap, GOLD["selected"], None, "train").train_dataset[:8]]
    plain = torch.stack([torch.from_numpy(np.asarray(Image.open(f).convert("RGB"))[20:198].copy()) for f in files])
    flipped = [not torch.equal(c, p) for c, p in zip(crops[0], plain)]
    assert any(flipped) and not all(flipped)
    assert all(torch.equal(c, p.flip(1)) for c, p, f in zip(crops[0], plain, flipped) if f)
    # mode "test": no flip, whatever the draws
    for seed in (0, 1, 2):
        test_crops = _first_batch(tmp_path, ap, 128, 4, "test", seed=seed, device_transform=True)
        tfiles = [os.path.join(str(tmp_path), name) for name, _ in CelebA(str(tmp_path), ap, GOLD["selected"], None, "test").test_dataset[:4]]
        want = torch.stack([torch.from_numpy(np.asarray(Image.open(f).convert("RGB"))[20:198].copy()) for f in tfiles])
        assert torch.equal(test_crops[0], want)
    # the positional signature of ImageTransform stays; the crop-only form is a keyword
    assert data_loader.ImageTransform(178, 128, False, False).resize is True
    with pytest.raises(NotImplementedError):
        data_loader.ImageTransform(178, 128, False, True, resize=False)


def test_entry_points_refuse_before_any_launch():
    """No device is touched: the pointers are dummies, so every call must return from the host-side checks."""
    lib = _lib.load()
    p = 4096
    big = 1 << 30
    for fn in (lib.dwc_image_u8_to_nhwc4, lib.dwc_bf16_image_u8_to_nhwc8):
        call = lambda B, hin, win, c, hout, wout, ws=p, nbytes=big: fn(p, p, p, p, p, p, p, B, hin, win, c, hout, wout, ws, nbytes, None)
        for shape in ((0, 178, 178, 3, 128, 128), (-1, 178, 178, 3, 128, 128), (2, 0, 178, 3, 128, 128), (2, 178, -5, 3, 128, 128),
                      (2, 178, 178, 3, 0, 128), (2, 178, 178, 3, 128, -1),            # zero or negative sizes
                      (2, 178, 178, 1, 128, 128), (2, 178, 178, 4, 128, 128),         # channel counts other than 3
                      (2, 178, 16385, 3, 128, 128), (2, 178, 178, 3, 128, 16385), (2, 16385, 178, 3, 128, 128),   # over-large extents
                      (65536, 8, 8, 3, 8, 8),                                         # more images than the grid's second axis holds
                      (2, 2048, 3, 3, 5, 2)):                                         # Image.resize goes vertical-first here
            assert call(*shape) == _lib.EINVAL, shape
            assert lib.dwc_image_u8_ws_bytes(*shape) == 0, shape
        assert fn(None, p, p, p, p, p, p, 2, 20, 31, 3, 7, 9, p, big, None) == _lib.EINVAL         # a missing pointer
        assert fn(p, p, p, p, p, p, None, 2, 20, 31, 3, 7, 9, p, big, None) == _lib.EINVAL
        # the intermediate of one output row does not fit the LDS: scratch is needed, and too little of it is refused
        need = lib.dwc_image_u8_ws_bytes(2, 12, 2048, 3, 2, 2048)
        assert need >= 2 * 12 * 2048 * 3
        assert call(2, 12, 2048, 3, 2, 2048, nbytes=need - 1) == -2                                 # DWC_EWORKSPACE
        assert call(2, 12, 2048, 3, 2, 2048, ws=None, nbytes=need) == -2
    assert lib.dwc_image_u8_ws_bytes(128, 178, 178, 3, 128, 128) == 0                               # the LDS holds a band
    assert lib.dwc_image_u8_ksize(178, 128) == 5 and lib.dwc_image_u8_ksize(178, 32) == 13 and lib.dwc_image_u8_ksize(64, 128) == 3
    assert lib.dwc_image_u8_ksize(0, 4) == 0 and lib.dwc_image_u8_ksize(4, 16385) == 0
    for n_in, n_out in ((178, 128), (5, 16), (2048, 5), (16384, 1), (1, 16384), (100, 100), (37, 16)):
        assert lib.dwc_image_u8_ksize(n_in, n_out) == u8image.resample_table(n_in, n_out)[1].shape[1]


def test_image_from_u8_refuses_malformed_input():
    good = torch.zeros(2, 20, 31, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        u8image.image_from_u8(good, 8)
    with pytest.raises(TypeError):
        u8image.image_from_u8(good.float(), 8)
    with pytest.raises(TypeError):
        u8image.image_from_u8(good.numpy(), 8)
    with pytest.raises(ValueError, match="HWC"):
        u8image.image_from_u8(good.permute(0, 3, 1, 2).contiguous(), 8)        # NCHW
    with pytest.raises(ValueError, match="HWC"):
        u8image.image_from_u8(good[0], 8)                                      # rank 3
    with pytest.raises(ValueError, match="HWC"):
        u8image.image_from_u8(torch.zeros(2, 20, 31, 4, dtype=torch.uint8), 8)
    with pytest.raises(ValueError, match="contiguous"):
        u8image.image_from_u8(torch.zeros(2, 3, 20, 31, dtype=torch.uint8).permute(0, 2, 3, 1), 8)   # HWC view of NCHW memory
    with pytest.raises(ValueError, match="contiguous"):
        u8image.image_from_u8(torch.zeros(2, 20, 62, 3, dtype=torch.uint8)[:, :, ::2], 8)


def test_abi_declares_the_new_symbols_at_version_11():
    header = open(os.path.join(os.path.dirname(HERE), "include", "dwcgan_hip.h")).read()
    for name in ("dwc_image_u8_ksize", "dwc_image_u8_ws_bytes", "dwc_image_u8_to_nhwc4", "dwc_bf16_image_u8_to_nhwc8"):
        protos = re.findall(r"\b%s\s*\(([^)]*)\)\s*;" % name, header)
        assert len(protos) == 1, name
        assert len(protos[0].split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert re.search(r"#define\s+DWC_ABI_VERSION\s+11\b", header)
    assert _lib.ABI_VERSION == 11 and _lib.load().dwc_version() == 11
    assert not hasattr(ops, "image_from_u8")                                   # one home: hipdwc.u8image


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def precision(request):
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision("fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("geom", GEOMETRIES + PLAN_GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("precision", ["fp32", "bf16"], indirect=True)
def test_image_from_u8_is_bit_equal_to_the_cpu_chain(precision, geom, content):
    u8, chain = reference(geom, content)
    want = ops.pack_image(chain.to(DEV))
    got = u8image.image_from_u8(u8.to(DEV), geom[2:])
    torch.cuda.synchronize()
    assert got.dtype == want.dtype == ops.act_dtype() and got.shape == want.shape == (B, ops.image_planes(), geom[2], geom[3])
    assert ops.is_image(got) and ops.pack_image(got) is got
    differing = int((got != want).sum())
    print("%s %s %s: %d differing elements" % (precision, _gid(geom), content, differing))
    assert torch.equal(got, want)                                              # the padding planes too
    assert not got[:, 3:].any()
    again = u8image.image_from_u8(u8.to(DEV), geom[2:])
    assert torch.equal(got, again)
    if geom[2] == geom[3]:
        assert torch.equal(u8image.image_from_u8(u8.to(DEV), geom[2]), got)    # an int is a square size


def _guard_tables(alloc, monkeypatch, geom):
    """The cached windows and the value table between guards as well (0xFF bytes: a window read past its end would be -1s)."""
    hin, win, hout, wout = geom
    dev = torch.device(DEV)
    tables = {}
    for n_in, n_out in {(hin, hout), (win, wout)}:
        start, coef = u8image.resample_table(n_in, n_out)
        tables[(n_in, n_out) + u8image._key(dev)] = (alloc.guarded_input(torch.from_numpy(start), dev),
                                                     alloc.guarded_input(torch.from_numpy(coef), dev))
    monkeypatch.setattr(u8image, "_TABLES", tables)
    monkeypatch.setattr(u8image, "_VALUES", {u8image._key(dev): alloc.guarded_input(u8image.value_table(), dev)})


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(37, 37, 16, 16), (20, 31, 7, 9)] + PLAN_GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("precision", ["fp32", "bf16"], indirect=True)
def test_image_from_u8_under_guarded_buffers(precision, geom, monkeypatch):
    """Input, windows, value table, output and scratch between guard zones, output and scratch poisoned with NaN: no guard byte
    changes, no NaN comes out, and the result is still the CPU chain's."""
    alloc = guarded_alloc.GuardedAllocator()
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    _guard_tables(alloc, monkeypatch, geom)
    u8, chain = reference(geom, "uniform")
    want = ops.pack_image(chain.to(DEV))
    before = dict(alloc.handed)
    got = u8image.image_from_u8(alloc.guarded_input(u8, DEV, channels_last=False), geom[2:])
    alloc.verify()
    assert alloc.handed.get("workspace", 0) == before.get("workspace", 0) + 1
    assert alloc.handed.get("empty_cl", 0) == before.get("empty_cl", 0) + 1
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_solver_step_from_the_device_mode(tmp_path):
    """One dis_update + gen_update + sample of the tiny configuration, three times under the same seeds: A and B fed from the
    default loader, C from the device mode."""
    from hipdwc import host, synth
    from solver import Solver
    from tools import asign_label
    dev = torch.device(DEV)
    ap = _celeba_dir(tmp_path, 4, seed=2)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.1)

    def run(device_mode):
        batch = _first_batch(tmp_path, ap, 32, 4, "train", seed=5, **({"device_transform": True} if device_mode else {}))
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        host.set_noise(host.DeviceNoise())
        trainer = Solver(cfg, dev, None).to(dev)
        trainer.copy_nets()
        x, label_src, label_trg, txt, lens = batch
        c_src = asign_label(label_src, cfg["c_dim"], "CelebA").to(dev)
        c_trg = asign_label(label_trg, cfg["c_dim"], "CelebA").to(dev)
        x, label_src, label_trg, txt, lens = (t.to(dev, non_blocking=True) for t in (x, label_src, label_trg, txt, lens))
        x_real = u8image.image_from_u8(x, 32) if device_mode else x
        packed = ops.pack_image(x_real).clone()
        trainer.dis_update(x_real, c_src, c_trg, txt, lens, label_src, label_trg, cfg, 0)
        trainer.gen_update(x_real, c_src, c_trg, txt, lens, label_src, label_trg, cfg, 0)
        torch.cuda.synchronize()
        losses = {k: float(torch.as_tensor(getattr(trainer, k)).detach()) for k in dir(trainer)
                  if k.startswith("loss_") and not callable(getattr(trainer, k))}
        outs = trainer.sample(x_real, txt, lens)
        return packed, losses, outs, x

    pa, la, oa, xa = run(False)
    pb, lb, ob, _ = run(False)
    pc, lc, oc, xc = run(True)
    assert xc.dtype == torch.uint8 and tuple(xc.shape) == (4, 178, 178, 3)
    assert torch.equal(pa, pb) and torch.equal(pc, pa)
    assert la and set(la) == set(lb) == set(lc) and all(np.isfinite(v) for v in la.values())
    for k in sorted(la):
        bound = max(4.0 * abs(la[k] - lb[k]), float(np.spacing(np.float32(abs(la[k])))))
        print("%s: A %.9g  |A-B| %.3g  |A-C| %.3g  bound %.3g" % (k, la[k], abs(la[k] - lb[k]), abs(la[k] - lc[k]), bound))
        assert abs(lc[k] - la[k]) <= bound, (k, la[k], lb[k], lc[k])
    assert oc[0].dtype == torch.float32 and tuple(oc[0].shape) == (4, 3, 32, 32) and oc[0].is_contiguous()
    assert torch.equal(oc[0], xa) and oa[0] is xa                              # the image writers get the default mode's tensor
    assert len(oc) == len(oa) and all(c.shape == a.shape and torch.isfinite(c).all() for c, a in zip(oc, oa))
