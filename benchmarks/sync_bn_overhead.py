"""What the phase path of synchronised batch norm (hipdwc.syncbn) costs on ONE device.

Iteration time (dis_update + gen_update) with dis.norm 'bn' at the c1 shape (128x128, B = 16, fp32) and the c2 shape (128x128,
B = 128, bf16): the plain three-launch chains against the five phases with a FORCED one-rank exchange -- a world_size-1 RCCL group
initialised in this process, every batch-norm layer of D carrying a ``GroupSync(force=True)``, no gradient reducer.  The two
variants ALTERNATE inside one process, ``--repeats`` rounds of ``--steps`` iterations each between device events; mean and spread
(min .. max) over the rounds, and the all-gathers issued per iteration.

This measures the extra launches (two per layer and pass) and a ONE-RANK collective (a device copy plus RCCL's launch overhead).
It does not measure what 4 small all-gathers per batch-norm layer and step cost over xGMI at 2 to 8 ranks: no multi-GPU node has
run this project.

    python benchmarks/sync_bn_overhead.py [--steps 8] [--warmup 3] [--repeats 5] [--configs c1,c2]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import bench  # noqa: E402
from hipdwc import ops, syncbn, synth  # noqa: E402
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


def measure(conf, steps, warmup, repeats):
    S, B, precision = SHAPES[conf]
    ops.set_precision(precision)
    dev = torch.device("cuda:0")
    batch = synth.make_batch(B, S, seed=1, device=dev)
    batch["txt_lens"] = batch["txt_lens"].cpu()
    runs = []
    for forced in (False, True):
        cfg = synth.make_config(image_size=S)
        cfg["dis"]["norm"] = "bn"
        torch.manual_seed(1)
        with contextlib.redirect_stdout(io.StringIO()):
            tr = Solver(cfg, dev, None).to(dev)
        tr.copy_nets()
        if forced:
            for m in tr.dis.bn_layers():
                m.sync = syncbn.GroupSync(None, force=True)
        runs.append({"forced": forced, "tr": tr, "cfg": cfg, "it": 0, "ms": []})
    for rnd in range(repeats + 1):                         # round 0 warms both variants up
        for r in runs:
            def one(r=r):
                bench.run_iteration(r["tr"], batch, r["cfg"], r["it"])
                r["it"] += 1
            if rnd == 0:
                for _ in range(warmup):
                    one()
                torch.cuda.synchronize()
            else:
                r["ms"].append(events(one, steps))
    ops.set_precision("fp32")
    base = sum(runs[0]["ms"]) / len(runs[0]["ms"])
    for r in runs:
        mean = sum(r["ms"]) / len(r["ms"])
        layers = r["tr"].dis.bn_layers()
        gathers = sum(m.sync.calls for m in layers) / r["it"] if r["forced"] else 0
        print(json.dumps({"config": conf, "batch": B, "precision": precision, "variant": "sync_forced_one_rank" if r["forced"] else "plain",
                          "bn_layers": len(layers), "all_gathers_per_iter": gathers, "ms_per_iter": spread(r["ms"]),
                          "vs_plain": round(mean / base, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="c1,c2")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0), init_method="file://" + os.path.join(d, "rdv"), rank=0,
                                world_size=1)
        try:
            for conf in args.configs.split(","):
                measure(conf, args.steps, args.warmup, args.repeats)
        finally:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
