"""What spectral normalisation (dis.norm 'sn') costs per training iteration: dis_update + gen_update with dis.norm 'none' and 'sn' at
the c1 shape (128x128, B = 16, fp32) and the c2 shape (128x128, B = 128, bf16), and the time of the SN kernels themselves (power
iteration, segmented epilogues, weight-gradient term) from one instrumented iteration (hipdwc.ops.KernelTimer).  With SN the D step
runs 4B samples instead of 3B: the reference evaluates x_real under two different sigmas.

    python benchmarks/sn_overhead.py [--steps 10] [--warmup 3] [--configs c1,c2]
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


def measure(conf, norm, steps, warmup):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    cfg = synth.make_config(image_size=S)
    cfg["dis"]["norm"] = norm
    torch.manual_seed(1)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = Solver(cfg, dev, None).to(dev)
    tr.copy_nets()
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    for it in range(warmup):
        bench.run_iteration(tr, batch, cfg, it)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for it in range(warmup, warmup + steps):
        bench.run_iteration(tr, batch, cfg, it)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    sn_ms, sn_launches = 0.0, 0
    if norm == "sn":
        ops.TIMER = ops.KernelTimer()
        try:
            bench.run_iteration(tr, batch, cfg, warmup + steps)
            ledger = ops.TIMER.ledger()
        finally:
            ops.TIMER = None
        for kind, ent in ledger.items():
            if kind.startswith("sn-"):
                sn_ms += ent["ms"]
                sn_launches += ent["launches"]
    ops.set_precision("fp32")
    return {"config": conf, "norm": norm, "batch": B, "precision": precision, "ms_per_iter": round(ms, 3),
            "images_per_s": round(B / ms * 1e3, 1), "sn_kernels_ms_per_iter": round(sn_ms, 4), "sn_calls_per_iter": sn_launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="c1,c2")
    args = ap.parse_args()
    for conf in args.configs.split(","):
        rows = [measure(conf, norm, args.steps, args.warmup) for norm in ("none", "sn")]
        for r in rows:
            print(json.dumps(r))
        print(json.dumps({"config": conf, "sn_vs_none_step_ratio": round(rows[1]["ms_per_iter"] / rows[0]["ms_per_iter"], 4)}))


if __name__ == "__main__":
    main()
