"""What the one-launch adversarial loss tails are worth for ``dis.gan_type: nsgan`` and ``wgan``.

At the c1 shape (128x128, B = 16, fp32) and, with ``--configs c1,c2``, the c2 shape (128x128, B = 128, bf16), per gan_type: dis_update
and gen_update with the objective on the tails (ops.ADV_TAIL_GAN = 1: one dwc_adv_tail_gan_fwd / _bwd launch per scale) against the
term-by-term route (ADV_TAIL_GAN = 0: split_outputs + MsImageDis.dis_loss_terms / gen_loss_terms -- torch.split, sigmoid, ones_like,
binary_cross_entropy, mean, scalar algebra and the backward of each), which is the route these objectives took before the tails.
The two variants ALTERNATE inside one process, ``--rounds`` windows of ``--steps`` steps each between device events (round 0 warms
both up and is not counted); per variant mean and spread (min .. max) over the rounds.  ``verdict``: 'within spread' when the
difference of the means is at most the larger of the two spreads (max - min), else which variant is faster.
``torch_ops``: non-view aten ops on device tensors in ONE untimed step of each kind, counted under a TorchDispatchMode
(benchmarks/torch_op_sites.py) -- bench.py's ledger holds the convolution launches only, so the stock-torch count comes from there.

    python benchmarks/gan_tail_overhead.py [--steps 6] [--warmup 3] [--rounds 5] [--configs c1] [--gan nsgan,wgan] [--out FILE]
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
sys.path.insert(0, os.path.join(REPO, "benchmarks"))
import torch  # noqa: E402

from hipdwc import ops, synth  # noqa: E402
from solver import Solver  # noqa: E402
from torch_op_sites import Log  # noqa: E402

SHAPES = {"c1": (128, 16, "fp32"), "c2": (128, 128, "bf16")}
VARIANTS = [("tail", 1), ("term by term", 0)]
STEPS = ("dis_update", "gen_update")


def spread(v):
    return {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def measure(conf, gan_type, steps, warmup, rounds, emit):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    runs = []
    for label, flag in VARIANTS:
        cfg = synth.make_config(image_size=S)
        cfg["dis"]["gan_type"] = gan_type
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Solver(cfg, dev, None).to(dev)
        tr.copy_nets()
        runs.append({"label": label, "flag": flag, "tr": tr, "cfg": cfg, "it": 0, "ms": {k: [] for k in STEPS}, "torch_ops": {}})

    def step(r, what):
        getattr(r["tr"], what)(batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                               batch["label_trg"], r["cfg"], r["it"])

    def window(r, reps, timed):
        """reps iterations; device time of the D steps and of the G steps apart (events around each step, one sync at the end)."""
        ev = []
        for _ in range(reps):
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            marks[0].record()
            step(r, "dis_update")
            marks[1].record()
            step(r, "gen_update")
            marks[2].record()
            r["tr"].smooth_moving()
            r["tr"].update_learning_rate()
            r["tr"].update_attention_status(r["it"])
            r["it"] += 1
            ev.append(marks)
        torch.cuda.synchronize()
        if timed:
            for i, what in enumerate(STEPS):
                r["ms"][what].append(sum(m[i].elapsed_time(m[i + 1]) for m in ev) / reps)

    try:
        for rnd in range(rounds + 1):                          # round 0 warms both variants up
            for r in runs:
                ops.ADV_TAIL_GAN = r["flag"]
                window(r, warmup if rnd == 0 else steps, rnd > 0)
        for r in runs:                                         # stock-torch device ops of one step of each kind (untimed)
            ops.ADV_TAIL_GAN = r["flag"]
            for what in STEPS:
                log = Log()
                with log:
                    step(r, what)
                torch.cuda.synchronize()
                r["torch_ops"][what] = sum(log.sites.values())
    finally:
        ops.ADV_TAIL_GAN = 1
        ops.set_precision("fp32")
    first, second = runs
    for what in STEPS:
        m1, m2 = sum(first["ms"][what]) / rounds, sum(second["ms"][what]) / rounds
        widest = max(max(r["ms"][what]) - min(r["ms"][what]) for r in runs)
        verdict = "within spread" if abs(m1 - m2) <= widest else ("%s faster" % (first["label"] if m1 < m2 else second["label"]))
        emit({"gan_type": gan_type, "timed": what, "config": conf, "batch": B, "precision": precision,
              first["label"]: {"ms": spread(first["ms"][what]), "torch_ops": first["torch_ops"][what]},
              second["label"]: {"ms": spread(second["ms"][what]), "torch_ops": second["torch_ops"][what]},
              "ratio_first_over_second": round(m1 / m2, 4), "widest_spread_ms": round(widest, 3), "verdict": verdict})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="c1")
    ap.add_argument("--gan", default="nsgan,wgan")
    ap.add_argument("--out", default=None, help="append every result line to this file as well")
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for conf in args.configs.split(","):
        for gan_type in args.gan.split(","):
            measure(conf, gan_type, args.steps, args.warmup, args.rounds, emit)


if __name__ == "__main__":
    main()
