"""``utils``: the names the reference's train.py and solver.py import from its ``utils`` module (reference utils.py), re-implemented
by contract without torchvision or tensorboardX.  Only the device branch of ``write_loss`` needs a GPU; the image writers are
exercised in tests/test_u8_out.py.
"""
import os
import re

import pytest
import torch

import utils
from hipdwc import host


def test_the_names_train_py_imports_exist():
    for name in ("prepare_sub_folder", "write_html", "write_loss", "get_config", "write_2images_single", "write_2images", "Timer",
                 "write_grid"):
        assert callable(getattr(utils, name)), name
    for name in ("weights_init", "get_scheduler", "moving_average", "load_vgg16", "vgg_preprocess"):
        assert getattr(utils, name) is getattr(host, name), name
    assert set(utils.__all__) <= set(dir(utils))


def test_prepare_sub_folder(tmp_path, capsys):
    out = str(tmp_path / "outputs" / "run1")
    got = utils.prepare_sub_folder(out)
    assert got == (os.path.join(out, "checkpoints"), os.path.join(out, "images"))            # the reference's order
    assert os.path.isdir(got[0]) and os.path.isdir(got[1])
    said = capsys.readouterr().out
    assert said.count("\n") == 2 and got[0] in said and got[1] in said                        # each new folder is reported
    assert utils.prepare_sub_folder(out) == got                                               # both exist: nothing to do
    assert capsys.readouterr().out == ""


def test_get_config_reads_yaml(tmp_path):
    path = tmp_path / "c.yaml"
    path.write_text("# a comment\nimage_save_iter: 10000\nlr: 0.0001\nuse_r1: false\ndataset: CelebA\n"
                    "gen:\n  dim: 64\n  activ: relu\n  use_attention: True\nlist: [1, 2, 3]\nname: \"caf\\u00e9\"\n", encoding="utf-8")
    cfg = utils.get_config(str(path))
    assert cfg == {"image_save_iter": 10000, "lr": 0.0001, "use_r1": False, "dataset": "CelebA",
                   "gen": {"dim": 64, "activ": "relu", "use_attention": True}, "list": [1, 2, 3], "name": "café"}


class _Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, name, value, step):
        self.calls.append((name, value, step))


class _Trainer:
    """CPU tensors and floats under names the rule picks, and everything it must pass over."""

    def __init__(self):
        self.loss_gen_total = torch.tensor(1.5, requires_grad=True)
        self.loss_dis_all = torch.tensor([0.25])
        self.loss_gen_vgg = 0
        self.loss_ds = 2.75
        self.grad_norm_dis = torch.tensor(3.0, dtype=torch.float64)
        self.nwd_x = -0.5
        self.lossy = torch.tensor(7, dtype=torch.int64)
        self.iterations = 41                       # no loss / grad / nwd in the name
        self.weight = torch.tensor(9.0)
        self.grad_sync = None                      # the rule picks it; it holds no scalar
        self.__loss_dunder__ = 5.0

    def loss_fn(self):                             # callable: not picked
        return 0.0

    def gradient_penalty(self, y, x):
        return 0.0


def test_write_loss_picks_by_the_reference_rule():
    w = _Writer()
    utils.write_loss(99, _Trainer(), w)
    want = {"loss_gen_total": 1.5, "loss_dis_all": 0.25, "loss_gen_vgg": 0.0, "loss_ds": 2.75, "grad_norm_dis": 3.0, "nwd_x": -0.5,
            "lossy": 7.0}
    assert sorted(c[0] for c in w.calls) == sorted(want)                       # exactly these, each once
    for name, value, step in w.calls:
        assert type(value) is float and value == want[name], name
        assert step == 100


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", [False, True], ids=["one-dtype", "mixed-dtypes"])
def test_write_loss_fetches_device_scalars_in_one_transfer(mixed, monkeypatch):
    """Device scalars (of one dtype, or of several: then they travel as float64, which holds each exactly) reach the writer with
    their values, beside host values, after ONE device-to-host copy."""
    t = _Trainer()
    t.loss_gen_total = torch.tensor(1.5, device="cuda:0", requires_grad=True)
    t.loss_dis_all = torch.tensor([0.1], device="cuda:0")                        # 0.1f: its float64 value is not 0.1
    t.loss_kl_x = torch.tensor(2 ** 40 + 1 if mixed else 5.0, device="cuda:0", dtype=torch.float64 if mixed else torch.float32)
    if mixed:
        t.lossy = torch.tensor(7, device="cuda:0", dtype=torch.int64)
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.device.type), real_cpu(self, *a, **k))[1])
    w = _Writer()
    utils.write_loss(9, t, w)
    assert copies == ["cuda"]
    got = {name: value for name, value, step in w.calls}
    assert all(step == 10 and type(value) is float for _, value, step in w.calls)
    want = {"loss_gen_total": 1.5, "loss_dis_all": float(torch.tensor(0.1)), "loss_kl_x": float(2 ** 40 + 1) if mixed else 5.0,
            "loss_gen_vgg": 0.0, "loss_ds": 2.75, "grad_norm_dis": 3.0, "nwd_x": -0.5, "lossy": 7.0}
    assert got == want


def test_write_html_lists_the_files_newest_first(tmp_path):
    page = tmp_path / "index.html"
    utils.write_html(str(page), 25000, 10000, "images", all_size=512)
    text = page.read_text()
    files = re.findall(r'<img src="([^"]+)"', text)
    per_iter = lambda j: ["images/gen_a2b_test_%08d.jpg" % j, "images/gen_b2a_test_%08d.jpg" % j,
                          "images/gen_a2b_train_%08d.jpg" % j, "images/gen_b2a_train_%08d.jpg" % j]
    assert files == ["images/gen_a2b_train_current.jpg", "images/gen_b2a_train_current.jpg"] + per_iter(20000) + per_iter(10000)
    assert re.findall(r'<a href="([^"]+)"', text) == files
    assert "index.html" in text and "512px" in text and text.lstrip().lower().startswith("<!doctype html>")
    # an iteration that is itself a multiple is listed; before the first save only the current grids are
    utils.write_html(str(page), 20000, 10000, "images")
    assert re.findall(r'<img src="([^"]+)"', page.read_text())[2:] == per_iter(20000) + per_iter(10000)
    utils.write_html(str(page), 500, 10000, "images")
    assert len(re.findall(r"<img ", page.read_text())) == 2


def test_timer_prints_the_elapsed_time(capsys):
    with utils.Timer("Elapsed time in update: %f"):
        pass
    out = capsys.readouterr().out
    m = re.fullmatch(r"Elapsed time in update: (\d+\.\d+)\n", out)
    assert m and 0.0 <= float(m.group(1)) < 5.0
