"""What ``pad_type: zero`` costs against ``reflect``, and what the zero rule inside the kernels is worth against a device pad.

At the c1 shape (128x128, B = 16, fp32) and the c2 shape (128x128, B = 128, bf16):
  (a) the whole iteration (dis_update + gen_update + moving averages) with gen.pad_type = dis.pad_type = 'zero' against 'reflect';
  (b) Conv2dBlock forward + backward at the ResBlock shape (256 -> 256, 3x3, 32x32, norm 'in', relu; the config's batch): the zero
      rule inside the kernels (ops.ZERO_PAD_HIP = 1) against the route from before it (ZERO_PAD_HIP = 0: F.pad on the device, then
      the unpadded convolution on the larger tensor).
  (s) the convolution launches of ONE iteration by kind under both rules (ops.KernelTimer spans between device events, after three
      warm-up iterations): milliseconds and launches per kind, every kind of at least 0.05 ms -- where the difference of (a) goes.
The two variants of a comparison ALTERNATE inside one process, ``--rounds`` windows of ``--steps`` steps each between device
events (round 0 warms both up and is not counted); per variant mean and spread (min .. max) over the rounds, so that a variant's own
spread stands beside every difference.  ``verdict``: 'within spread' when the difference of the means is at most the larger of the
two spreads (max - min), else which variant is faster.  (Protocol of benchmarks/lrelu_fused_overhead.py.)

    python benchmarks/zero_pad_overhead.py [--steps 6] [--warmup 3] [--rounds 5] [--configs c1,c2] [--parts a,b,s]
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
from hipdwc import ops, synth  # noqa: E402
from solver import Solver  # noqa: E402

SHAPES = {"c1": (128, 16, "fp32"), "c2": (128, 128, "bf16")}


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


def iteration_variants(conf, dev):
    S, B, _ = SHAPES[conf]
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    runs = []
    for label in ("zero", "reflect"):
        cfg = synth.make_config(image_size=S)
        cfg["gen"]["pad_type"] = cfg["dis"]["pad_type"] = label
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Solver(cfg, dev, None).to(dev)
        tr.copy_nets()
        state = {"it": 0}

        def one(tr=tr, cfg=cfg, state=state):
            bench.run_iteration(tr, batch, cfg, state["it"])
            state["it"] += 1
        runs.append({"label": "pad_type " + label, "hip": 1, "one": one, "ms": []})
    return runs


def block_variants(conf, dev):
    import networks.networks as nets
    _, B, _ = SHAPES[conf]
    torch.manual_seed(1)
    blk = nets.Conv2dBlock(256, 256, 3, 1, 1, norm="in", activation="relu", pad_type="zero").to(dev)
    x = torch.randn(B, 256, 32, 32, device=dev).to(ops.act_dtype()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gy = torch.randn(B, 256, 32, 32, device=dev).to(ops.act_dtype()).contiguous(memory_format=torch.channels_last)

    def one():
        x.grad = None
        blk.zero_grad(set_to_none=True)
        blk(x).backward(gy)
    return [{"label": "zero in kernel", "hip": 1, "one": one, "ms": []}, {"label": "F.pad + unpadded conv", "hip": 0, "one": one, "ms": []}]


PARTS = {"a": ("iteration", iteration_variants), "b": ("Conv2dBlock 256>256 k3 32x32 fwd+bwd", block_variants)}


def measure(conf, part, steps, warmup, rounds):
    _, B, precision = SHAPES[conf]
    what, make = PARTS[part]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    try:
        runs = make(conf, dev)
        for rnd in range(rounds + 1):                          # round 0 warms both variants up
            for r in runs:
                ops.ZERO_PAD_HIP = r["hip"]
                if rnd == 0:
                    for _ in range(warmup):
                        r["one"]()
                    torch.cuda.synchronize()
                else:
                    r["ms"].append(events(r["one"], steps))
    finally:
        ops.ZERO_PAD_HIP = 1
        ops.set_precision("fp32")
    first, second = runs
    m1, m2 = sum(first["ms"]) / rounds, sum(second["ms"]) / rounds
    widest = max(max(r["ms"]) - min(r["ms"]) for r in runs)
    verdict = "within spread" if abs(m1 - m2) <= widest else ("%s faster" % (first["label"] if m1 < m2 else second["label"]))
    print(json.dumps({"part": part, "timed": what, "config": conf, "batch": B, "precision": precision,
                      first["label"]: {"ms": spread(first["ms"])}, second["label"]: {"ms": spread(second["ms"])},
                      "ratio_first_over_second": round(m1 / m2, 4), "widest_spread_ms": round(widest, 3), "verdict": verdict}), flush=True)


def spans(conf):
    """Part (s): per launch kind of one iteration, zero against reflect."""
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    try:
        batch = synth.make_batch(B, S, seed=1, device=dev)
        batch["txt_lens"] = batch["txt_lens"].cpu()
        res = {}
        for pad in ("zero", "reflect"):
            cfg = synth.make_config(image_size=S)
            cfg["gen"]["pad_type"] = cfg["dis"]["pad_type"] = pad
            torch.manual_seed(1)
            with contextlib.redirect_stdout(io.StringIO()):
                tr = Solver(cfg, dev, None).to(dev)
            tr.copy_nets()
            for it in range(3):
                bench.run_iteration(tr, batch, cfg, it)
            torch.cuda.synchronize()
            ops.TIMER = ops.KernelTimer()
            try:
                bench.run_iteration(tr, batch, cfg, 3)
                res[pad] = ops.TIMER.ledger()
            finally:
                ops.TIMER = None
            del tr
    finally:
        ops.set_precision("fp32")
    total = {p: sum(v["ms"] for v in res[p].values()) for p in res}
    print("part s, %s (%s, B=%d): convolution launches of one iteration, ms: zero %.2f, reflect %.2f" % (conf, precision, B, total["zero"],
                                                                                                     total["reflect"]), flush=True)
    none = {"ms": 0.0, "launches": 0}
    for kind in sorted(set(res["zero"]) | set(res["reflect"])):
        z, r = res["zero"].get(kind, none), res["reflect"].get(kind, none)
        if max(z["ms"], r["ms"]) >= 0.05:
            print("  %-26s zero %7.3f ms (%3d)   reflect %7.3f ms (%3d)" % (kind, z["ms"], z["launches"], r["ms"], r["launches"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="c1,c2")
    ap.add_argument("--parts", default="a,b,s")
    args = ap.parse_args()
    for conf in args.configs.split(","):
        for part in args.parts.split(","):
            if part == "s":
                spans(conf)
            else:
                measure(conf, part, args.steps, args.warmup, args.rounds)


if __name__ == "__main__":
    main()
