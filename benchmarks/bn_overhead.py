"""What batch normalisation (dis.norm 'bn') costs, and whether the HIP kernels earn their keep against stock device ops.

1. Iteration time (dis_update + gen_update) with dis.norm 'none', 'bn' on csrc/norm.hip (DWC_BN_HIP=1) and 'bn' on the stock-op form
   of the same segmented semantics (DWC_BN_HIP=0: F.batch_norm per segment, hipdwc.batchnorm), at the c1 shape (128x128, B = 16,
   fp32) and the c2 shape (128x128, B = 128, bf16).  The three variants ALTERNATE inside one process, ``--repeats`` rounds of
   ``--steps`` iterations each between device events; mean and spread (min .. max) over the rounds are reported.
2. The batch-norm launches alone at the discriminator's shapes -- the D step's [x_fake | x_fake1 | x_real] (S = 3) -- forward and
   backward, between device events on warmed shapes: us and GB/s (2 tensor passes forward, 3 backward: what any implementation must
   move) for the HIP form, the stock-op form and ``ops.instance_norm`` at the same shape.  A shape where the HIP form loses to the
   stock-op form is flagged ``hip_loses``.

    python benchmarks/bn_overhead.py [--steps 8] [--warmup 3] [--repeats 5] [--configs c1,c2] [--skip-steps]
"""
import argparse
import contextlib
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from hipdwc import batchnorm, ops, synth  # noqa: E402
from solver import Solver  # noqa: E402

SHAPES = {"c1": (128, 16, "fp32"), "c2": (128, 128, "bf16")}
VARIANTS = (("none", 1), ("bn", 1), ("bn", 0))          # (dis.norm, BN_HIP)


def spread(v):
    return {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure_steps(conf, steps, warmup, repeats):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    runs = []
    for norm, hip in VARIANTS:
        cfg = synth.make_config(image_size=S)
        cfg["dis"]["norm"] = norm
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Solver(cfg, dev, None).to(dev)
        tr.copy_nets()
        runs.append({"norm": norm, "hip": hip, "tr": tr, "cfg": cfg, "it": 0, "ms": []})
    for rnd in range(repeats + 1):                         # round 0 warms every variant up
        for r in runs:
            batchnorm.BN_HIP = r["hip"]

            def one(r=r):
                bench.run_iteration(r["tr"], batch, r["cfg"], r["it"])
                r["it"] += 1
            if rnd == 0:
                for _ in range(warmup):
                    one()
                torch.cuda.synchronize()
            else:
                r["ms"].append(events(one, steps))
    batchnorm.BN_HIP = 1
    ops.set_precision("fp32")
    base = sum(runs[0]["ms"]) / len(runs[0]["ms"])
    for r in runs:
        mean = sum(r["ms"]) / len(r["ms"])
        print(json.dumps({"config": conf, "batch": B, "precision": precision, "dis_norm": r["norm"], "DWC_BN_HIP": r["hip"],
                          "ms_per_iter": spread(r["ms"]), "vs_norm_none": round(mean / base, 4)}))


def dis_bn_shapes(image_size, cfg):
    """(C, H) of every batch-norm layer of the discriminator (networks.MsImageDis._make_net: layer 0 has no norm)."""
    d = cfg["dis"]
    out = []
    for s in range(d["num_scales"]):
        dim, h = d["dim"], image_size // (2 ** s) // 2
        for l in range(1, d["n_layer"]):
            dim, h = min(dim * 2, 512), h // 2
            out.append((dim, h))
    return sorted(set(out), reverse=True)


def measure_kernels(conf, repeats, reps=20):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    dt = ops.act_dtype()
    cfg = synth.make_config(image_size=S)
    seg = 3
    for C, H in dis_bn_shapes(S, cfg):
        N = seg * B
        x = torch.randn(N, C, H, H, device=dev).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        gy = torch.randn(N, C, H, H, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
        w, b = (torch.rand(C, device=dev) + 0.5).requires_grad_(True), torch.zeros(C, device=dev, requires_grad=True)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbytes = x.numel() * x.element_size()
        forms = {
            "hip": lambda: batchnorm.batch_norm(x, w, b, rm, rv, segments=seg, order=(0, 2, 1, 2), act="lrelu"),
            "stock": lambda: batchnorm.batch_norm(x, w, b, rm, rv, segments=seg, order=(0, 2, 1, 2), act="lrelu"),
            "instance_norm": lambda: ops.instance_norm(x, None, None, relu=True),
        }
        row = {"config": conf, "precision": precision, "shape": [N, H, H, C], "segments": seg}
        for name, fwd in forms.items():
            batchnorm.BN_HIP = 0 if name == "stock" else 1
            f_us, b_us = [], []
            for rnd in range(repeats + 1):                 # round 0: warm-up
                f = events(fwd, reps) * 1e3
                y = fwd()

                def bwd():
                    x.grad = w.grad = b.grad = None
                    y.backward(gy, retain_graph=True)
                t = events(bwd, reps) * 1e3
                if rnd:
                    f_us.append(f)
                    b_us.append(t)
            fm, bm = sum(f_us) / len(f_us), sum(b_us) / len(b_us)
            row[name] = {"fwd_us": spread(f_us), "bwd_us": spread(b_us), "fwd_GBps": round(2 * nbytes / fm / 1e3, 1),
                         "bwd_GBps": round(3 * nbytes / bm / 1e3, 1)}
        batchnorm.BN_HIP = 1
        row["hip_loses"] = [d for d in ("fwd", "bwd") if row["hip"][d + "_us"]["mean"] > row["stock"][d + "_us"]["mean"]]
        print(json.dumps(row))
    ops.set_precision("fp32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="c1,c2")
    ap.add_argument("--skip-steps", action="store_true", help="only the per-launch table")
    args = ap.parse_args()
    for conf in args.configs.split(","):
        measure_kernels(conf, args.repeats)
        if not args.skip_steps:
            measure_steps(conf, args.steps, args.warmup, args.repeats)


if __name__ == "__main__":
    main()
