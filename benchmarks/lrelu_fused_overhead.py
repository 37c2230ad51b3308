"""What LeakyReLU fused into the IN / AdaIN / LN kernels (csrc/norm.hip) is worth, and what ``gen.activ: lrelu`` costs.

At the c1 shape (128x128, B = 16, fp32) and the c2 shape (128x128, B = 128, bf16):
  (a) the D step (dis_update) with dis.norm 'in' and the default dis.activ 'lrelu': fused (ops.NORM_ACT_FUSED = 1) against the route
      from before the fused form (NORM_ACT_FUSED = 0: the norm unfused, then torch's leaky_relu, the bias gradient reduced);
  (b) the same with dis.norm 'ln';
  (c) the whole iteration (dis_update + gen_update + moving averages) with gen.activ 'lrelu' against gen.activ 'relu'.
The two variants of a comparison ALTERNATE inside one process, ``--rounds`` windows of ``--steps`` steps each between device
events (round 0 warms both up and is not counted); per variant mean and spread (min .. max) over the rounds, so that a variant's own
spread stands beside every difference.  ``verdict``: 'within spread' when the difference of the means is at most the larger of the
two spreads (max - min), else which variant is faster.

    python benchmarks/lrelu_fused_overhead.py [--steps 6] [--warmup 3] [--rounds 5] [--configs c1,c2] [--parts a,b,c]
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
# part -> (what is timed, [(label, dis.norm, gen.activ, NORM_ACT_FUSED), the two variants])
PARTS = {
    "a": ("dis_update", [("in fused", "in", "relu", 1), ("in unfused", "in", "relu", 0)]),
    "b": ("dis_update", [("ln fused", "ln", "relu", 1), ("ln unfused", "ln", "relu", 0)]),
    "c": ("iteration", [("gen lrelu", "none", "lrelu", 1), ("gen relu", "none", "relu", 1)]),
}


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


def measure(conf, part, steps, warmup, rounds):
    S, B, precision = SHAPES[conf]
    what, variants = PARTS[part]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    runs = []
    for label, dis_norm, gen_activ, fused in variants:
        cfg = synth.make_config(image_size=S)
        cfg["dis"]["norm"] = dis_norm
        cfg["gen"]["activ"] = gen_activ
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Solver(cfg, dev, None).to(dev)
        tr.copy_nets()
        runs.append({"label": label, "fused": fused, "tr": tr, "cfg": cfg, "it": 0, "ms": []})
    try:
        for rnd in range(rounds + 1):                          # round 0 warms both variants up
            for r in runs:
                ops.NORM_ACT_FUSED = r["fused"]

                def one(r=r):
                    if what == "iteration":
                        bench.run_iteration(r["tr"], batch, r["cfg"], r["it"])
                    else:
                        r["tr"].dis_update(batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"],
                                           batch["label_src"], batch["label_trg"], r["cfg"], r["it"])
                    r["it"] += 1
                if rnd == 0:
                    for _ in range(warmup):
                        one()
                    torch.cuda.synchronize()
                else:
                    r["ms"].append(events(one, steps))
    finally:
        ops.NORM_ACT_FUSED = 1
        ops.set_precision("fp32")
    first, second = runs
    m1, m2 = sum(first["ms"]) / rounds, sum(second["ms"]) / rounds
    widest = max(max(r["ms"]) - min(r["ms"]) for r in runs)
    verdict = "within spread" if abs(m1 - m2) <= widest else ("%s faster" % (first["label"] if m1 < m2 else second["label"]))
    print(json.dumps({"part": part, "timed": what, "config": conf, "batch": B, "precision": precision,
                      first["label"]: {"ms": spread(first["ms"])}, second["label"]: {"ms": spread(second["ms"])},
                      "ratio_first_over_second": round(m1 / m2, 4), "widest_spread_ms": round(widest, 3), "verdict": verdict}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="c1,c2")
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    for conf in args.configs.split(","):
        for part in args.parts.split(","):
            measure(conf, part, args.steps, args.warmup, args.rounds)


if __name__ == "__main__":
    main()
