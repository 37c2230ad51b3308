"""What the device half of the input pipeline costs beside the default one (csrc/image_u8.hip, hipdwc.u8image).

CPU part (one thread): ms per ``CelebA.__getitem__`` in both loader modes over ``--images`` in-memory synthetic 178x218 JPEGs
(quality 90; ``Image.open`` is handed the bytes, so no file system is in the figure), and the decode / transform split: decode =
``Image.open(...).convert("RGB")`` alone, transform = ``ImageTransform`` on the decoded image in either mode.

Device part: HIP-event time of what a step does with a batch that sits in pinned host memory, 178 -> 128:

  (a) default   H2D of the fp32 NCHW batch, then ``ops.pack_image``
  (b) device    H2D of the uint8 HWC batch, then ``u8image.image_from_u8``

at B = 16 in fp32 and B = 128 in bf16, and each form's launch alone on a batch that is already resident (``*_kernel``).  The forms
ALTERNATE inside one process: ``--rounds`` windows of ``--calls`` back-to-back calls each between device events (round 0 warms them
up and is not counted); per form the median and max - min over the rounds.

    python benchmarks/u8_pipeline_overhead.py [--images 300] [--calls 50] [--rounds 7] [--skip-device]
"""
import argparse
import io
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

import data_loader  # noqa: E402
from data_ios import celeba_data  # noqa: E402


def synthetic_jpegs(n):
    """Smooth random fields (a JPEG of white noise decodes unrepresentatively slowly), 178 wide x 218 high, quality 90."""
    g = np.random.RandomState(0)
    out = []
    for _ in range(n):
        small = g.randint(0, 256, (28, 23, 3), dtype=np.uint8)
        img = Image.fromarray(small).resize((178, 218), Image.BICUBIC)
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=90)
        out.append(buf.getvalue())
    return out


class MemoryCelebA(celeba_data.CelebA):
    """``CelebA`` with the attribute file and the images in memory: ``__getitem__`` is the class's own."""

    def __init__(self, jpegs, transform):
        self.jpegs = jpegs
        self.names = ["%06d.jpg" % (i + 1) for i in range(len(jpegs))]
        super().__init__("", None, ["Black_Hair", "Blond_Hair", "Brown_Hair", "Male", "Smiling", "Young", "Eyeglasses", "No_Beard"],
                         transform, "train")

    def preprocess(self):
        g = random.Random(1)
        self.train_dataset = [[name, [int(g.random() < 0.4) for _ in self.selected_attrs]] for name in self.names]


def cpu_part(n_images):
    torch.set_num_threads(1)
    jpegs = synthetic_jpegs(n_images)
    by_name = {"%06d.jpg" % (i + 1): b for i, b in enumerate(jpegs)}
    real_open = Image.open
    celeba_data.Image.open = lambda path, *a, **k: real_open(io.BytesIO(by_name[os.path.basename(path)]), *a, **k)
    res = {"what": "cpu", "images": n_images, "pillow": Image.__version__, "threads": torch.get_num_threads()}
    try:
        for mode, resize in (("default", True), ("device", False)):
            tf = data_loader.ImageTransform(178, 128, flip=True, square=False, resize=resize)
            ds = MemoryCelebA(jpegs, tf)
            for timed in (False, True):                               # one untimed pass first
                random.seed(3)
                t0 = time.perf_counter()
                for i in range(n_images):
                    ds[i]
                dt = time.perf_counter() - t0
            res["getitem_%s_ms" % mode] = round(1e3 * dt / n_images, 4)
            decoded = [real_open(io.BytesIO(b)).convert("RGB") for b in jpegs]
            random.seed(3)
            t0 = time.perf_counter()
            for img in decoded:
                tf(img)
            res["transform_%s_ms" % mode] = round(1e3 * (time.perf_counter() - t0) / n_images, 4)
        t0 = time.perf_counter()
        for b in jpegs:
            real_open(io.BytesIO(b)).convert("RGB")
        res["decode_ms"] = round(1e3 * (time.perf_counter() - t0) / n_images, 4)
    finally:
        celeba_data.Image.open = real_open
    print(json.dumps(res), flush=True)


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps                            # us per call


def device_part(calls, rounds):
    from hipdwc import ops, u8image
    if not torch.cuda.is_available():
        raise SystemExit("the device part needs the GPU (--skip-device runs the CPU part alone)")
    dev = torch.device("cuda:0")
    for B, precision in ((16, "fp32"), (128, "bf16")):
        ops.set_precision(precision)
        g = torch.Generator().manual_seed(B)
        u8 = torch.randint(0, 256, (B, 178, 178, 3), dtype=torch.uint8, generator=g).pin_memory()
        f32 = (torch.rand(B, 3, 128, 128, generator=g) * 2 - 1).pin_memory()
        u8_dev, f32_dev = u8.to(dev), f32.to(dev)
        fns = {"default": lambda: ops.pack_image(f32.to(dev, non_blocking=True)),
               "device": lambda: u8image.image_from_u8(u8.to(dev, non_blocking=True), 128),
               "default_kernel": lambda: ops.pack_image(f32_dev),              # the launches alone, on resident batches
               "device_kernel": lambda: u8image.image_from_u8(u8_dev, 128)}
        times = {k: [] for k in fns}
        for r in range(rounds + 1):
            for name, fn in fns.items():
                t = events(fn, calls)
                if r:
                    times[name].append(t)
        res = {"what": "device", "B": B, "precision": precision, "calls": calls, "rounds": rounds,
               "h2d_bytes": {"default": f32.numel() * 4, "device": u8.numel()}}
        for name, v in times.items():
            res[name + "_us"] = {"median": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1),
                                 "windows": [round(t, 1) for t in v]}
        res["device_minus_default_us"] = round(res["device_us"]["median"] - res["default_us"]["median"], 1)
        print(json.dumps(res), flush=True)
    ops.set_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-device", action="store_true")
    args = ap.parse_args()
    cpu_part(args.images)
    if not args.skip_device:
        device_part(args.calls, args.rounds)


if __name__ == "__main__":
    main()
