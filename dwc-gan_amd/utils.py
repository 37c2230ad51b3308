"""The names the reference's ``train.py`` and ``solver.py`` import from ``utils`` (reference utils.py), behind the same signatures
and file names, without torchvision: the image writers turn the outputs of ``Solver.sample`` into bytes on the device
(``hipdwc.u8image.grid_u8``) and hand them to PIL.  ``tensorboardX`` stays the caller's: ``write_loss`` takes
whatever object has ``add_scalar``.
"""
import numbers
import os
import time

import torch
import yaml
from PIL import Image

from hipdwc import u8image
from hipdwc.host import get_scheduler, load_vgg16, moving_average, vgg_preprocess, weights_init  # noqa: F401  (re-exported)

__all__ = ["get_config", "prepare_sub_folder", "Timer", "write_grid", "write_2images", "write_2images_single", "write_html",
           "write_loss", "weights_init", "get_scheduler", "moving_average", "load_vgg16", "vgg_preprocess"]


def get_config(config):
    """The YAML file ``config`` as a dict."""
    with open(config, "r", encoding="utf-8") as stream:
        return yaml.safe_load(stream)


def prepare_sub_folder(output_directory):
    """Makes sure a run's two output folders exist and returns them as ``(checkpoint_directory, image_directory)``; a folder it had
    to make is reported on stdout."""
    made = []
    for leaf in ("checkpoints", "images"):
        folder = os.path.join(output_directory, leaf)
        if not os.path.isdir(folder):
            os.makedirs(folder, exist_ok=True)
            print("new output folder %s" % folder)
        made.append(folder)
    return tuple(made)


class Timer:
    """``with Timer("update took %f s"):`` -- on leaving the block, prints the template filled with the seconds spent inside."""

    def __init__(self, msg):
        self._template = msg
        self._entered = None

    def __enter__(self):
        self._entered = time.perf_counter()
        return self

    def __exit__(self, *exc):
        print(self._template % (time.perf_counter() - self._entered))
        return False


# ---- image writers ------------------------------------------------------------------------------------------------------------------
_PINNED = {}                 # device index -> pinned host bytes the grids are copied into (grown on demand)


def _to_host(u8):
    """Device uint8 tensor -> numpy view of a pinned host copy, waiting for that copy alone (an event, not the device)."""
    key = u8.device.index
    buf = _PINNED.get(key)
    if buf is None or buf.numel() < u8.numel():
        buf = _PINNED[key] = torch.empty(u8.numel(), dtype=torch.uint8, pin_memory=True)
    host = buf[:u8.numel()].view(u8.shape)
    host.copy_(u8, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    return host.numpy()


def write_grid(image_outputs, display_image_num, file_name):
    """The first ``display_image_num`` images of every tensor of ``image_outputs``, one tensor per row, normalised to their common
    minimum and maximum, as an image file whose format follows from the extension (reference utils.py:69-73)."""
    grid = u8image.grid_u8(list(image_outputs), display_image_num)
    Image.fromarray(_to_host(grid)).save(file_name)


def _grid_file(image_directory, side, postfix):
    """The reference's name of a sample grid: ``gen_<a2b|b2a>_<postfix>.jpg`` under ``image_directory``."""
    return "%s/gen_%s_%s.jpg" % (image_directory, side, postfix)


def write_2images(image_outputs, display_image_num, image_directory, postfix):
    """The first half of the list as the a2b grid, the rest as the b2a grid."""
    half = len(image_outputs) // 2
    for side, part in (("a2b", image_outputs[:half]), ("b2a", image_outputs[half:])):
        write_grid(part, display_image_num, _grid_file(image_directory, side, postfix))


def write_2images_single(image_outputs, display_image_num, image_directory, postfix):
    """The whole list as one (a2b) grid."""
    write_grid(image_outputs, display_image_num, _grid_file(image_directory, "a2b", postfix))


_PAGE = """<!DOCTYPE html>
<html lang="en">
<head>
<meta charset="utf-8">
<meta http-equiv="refresh" content="60">
<title>%(name)s: sample grids</title>
</head>
<body>
<h1>%(name)s</h1>
%(figures)s</body>
</html>
"""
_FIGURE = '<figure>\n  <figcaption>iteration %(it)d: %(base)s</figcaption>\n  <a href="%(path)s"><img src="%(path)s" alt="%(base)s" style="width:%(px)dpx"></a>\n</figure>\n'


def write_html(filename, iterations, image_save_iterations, image_directory, all_size=1536):
    """An index page (it reloads itself every minute) of the sample grids: the two ``*_train_current.jpg`` first, then, for every
    multiple of ``image_save_iterations`` up to ``iterations``, newest first, the test and the train grids of both directions."""
    sides = ("a2b", "b2a")
    shown = [(iterations, _grid_file(image_directory, side, "train_current")) for side in sides]
    step = int(image_save_iterations)
    for saved in range(iterations // step * step, 0, -step):
        shown += [(saved, _grid_file(image_directory, side, "%s_%08d" % (split, saved))) for split in ("test", "train") for side in sides]
    figures = "".join(_FIGURE % {"it": it, "path": path, "base": os.path.basename(path), "px": all_size} for it, path in shown)
    with open(filename, "w") as page:
        page.write(_PAGE % {"name": os.path.basename(filename), "figures": figures})


# ---- scalars ------------------------------------------------------------------------------------------------------------------------
def write_loss(iterations, trainer, train_writer):
    """``train_writer.add_scalar(name, value, iterations + 1)`` for every attribute of ``trainer`` that is not callable, not a dunder
    and has ``loss``, ``grad`` or ``nwd`` in its name (the reference's rule).  Values arrive as Python floats; the scalars that live
    on a device come to the host in ONE transfer.  An attribute the rule picks that holds no scalar (``Solver.grad_sync``: None or
    an object) is passed over."""
    picked = []
    for name in dir(trainer):
        if name.startswith("__") or not ("loss" in name or "grad" in name or "nwd" in name):
            continue
        value = getattr(trainer, name)
        if callable(value):
            continue
        if isinstance(value, torch.Tensor):
            if value.numel() == 1:
                picked.append((name, value.detach().reshape(())))
        elif isinstance(value, numbers.Real):
            picked.append((name, float(value)))
    on_device = [(i, v) for i, (_, v) in enumerate(picked) if isinstance(v, torch.Tensor) and v.device.type != "cpu"]
    if on_device:
        mixed = len({v.dtype for _, v in on_device}) > 1          # (one dtype, the usual case: no conversion launches)
        host = torch.stack([v.double() if mixed else v for _, v in on_device]).cpu().tolist()
        for (i, _), v in zip(on_device, host):
            picked[i] = (picked[i][0], v)
    for name, value in picked:
        train_writer.add_scalar(name, float(value), iterations + 1)
