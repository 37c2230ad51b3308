"""What the gradient penalty (gp_w = 10) and the R1 penalty (use_r1, regularised on EVERY step: d_reg_every = 1) add to the D step, on
the closed-form HIP branch (hipdwc.penalty, ops.PENALTY_HIP = 1) and on torch's double backward (= 0), at the c1 shape (128x128,
B = 16, fp32) and the c2 shape (128x128, B = 128, bf16).  One process, one trainer per shape; the variants are timed in alternation,
``--rounds`` windows of ``--steps`` dis_update calls each (device events around the window), so that the run-to-run spread of a
variant (max - min over its windows) stands beside every difference between two variants.

    python benchmarks/penalty_overhead.py [--steps 10] [--warmup 3] [--rounds 3] [--configs c1,c2] [--norm none|in|ln]
                                          [--out profiles/penalty_overhead.json]

``--norm in / ln`` sets ``dis.norm``: the HIP branch is then hipdwc.normjvp (the tangent of the norm), the torch branch
the double backward through the norm.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import torch  # noqa: E402

from hipdwc import ops, synth  # noqa: E402
from solver import Solver  # noqa: E402

SHAPES = {"c1": (128, 16, "fp32"), "c2": (128, 128, "bf16")}
PENALTIES = {"none": dict(gp_w=0.0, use_r1=False), "r1": dict(gp_w=0.0, use_r1=True), "gp": dict(gp_w=10.0, use_r1=False)}
VARIANTS = [("none", 1), ("r1", 0), ("r1", 1), ("gp", 0), ("gp", 1)]          # (penalty, ops.PENALTY_HIP)


def window(tr, batch, cfg, hip, steps, it0):
    ops.PENALTY_HIP = hip
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for it in range(it0, it0 + steps):
        tr.dis_update(batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
                      batch["label_trg"], cfg, it, tape_content=False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def measure(conf, steps, warmup, rounds, norm="none"):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    base = synth.make_config(image_size=S)
    base["dis"]["norm"] = norm                        # (in / ln: the HIP branch is hipdwc.normjvp, the tangent of the norm)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = Solver(base, dev, None).to(dev)
    tr.copy_nets()
    tr.d_reg_every = 1
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    cfgs = {name: dict(base, **kw) for name, kw in PENALTIES.items()}
    times = {v: [] for v in VARIANTS}
    it = 0
    for name, hip in VARIANTS:                        # every variant's shapes, layouts and library algorithms warmed up first
        window(tr, batch, cfgs[name], hip, warmup, it)
        it += warmup
    for _ in range(rounds):
        for name, hip in VARIANTS:
            times[(name, hip)].append(window(tr, batch, cfgs[name], hip, steps, it))
            it += steps
    ops.set_precision("fp32")
    rows = []
    for (name, hip), ms in times.items():
        rows.append({"config": conf, "batch": B, "precision": precision, "dis_norm": norm, "penalty": name, "penalty_hip": hip,
                     "d_step_ms_windows": [round(m, 3) for m in ms], "d_step_ms_median": round(statistics.median(ms), 3),
                     "spread_ms": round(max(ms) - min(ms), 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", default="c1,c2")
    ap.add_argument("--norm", default="none", choices=["none", "in", "ln"], help="dis.norm of the discriminator under the penalties")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    default = ops.PENALTY_HIP
    rows = []
    try:
        for conf in args.configs.split(","):
            part = measure(conf, args.steps, args.warmup, args.rounds, args.norm)
            med = {(r["penalty"], r["penalty_hip"]): r["d_step_ms_median"] for r in part}
            for name in ("r1", "gp"):
                part.append({"config": conf, "dis_norm": args.norm, "penalty": name, "hip_over_torch_d_step": round(med[(name, 1)] / med[(name, 0)], 4),
                             "added_ms_torch": round(med[(name, 0)] - med[("none", 1)], 3),
                             "added_ms_hip": round(med[(name, 1)] - med[("none", 1)], 3)})
            for r in part:
                print(json.dumps(r), flush=True)
            rows += part
    finally:
        ops.PENALTY_HIP = default
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "dis_norm": args.norm, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
