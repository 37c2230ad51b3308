"""What the text encoder's ``group`` costs and what batched inference gains (csrc/txt_glue.hip ``dwc_txt_regroup_*``).

The shipped generator configuration's ``TxtEncoder`` (embed 300, style 64, hidden 300, two layers, both dropouts 0.1) on the tokens
and lengths ``synth.make_batch`` draws.  The variants of a table ALTERNATE inside one process: ``--rounds`` windows of ``--calls``
back-to-back calls each between device events (round 0 warms all of them up and is not counted); per variant the median and
max - min over the rounds, in microseconds per call:

  training    forward + backward in train mode at B = 16 and 128 with ``group`` None (no regroup launch), 1 and B/8
  inference   eval mode, no_grad, at B = 8 and 64: B batch-1 calls (what ``Solver.sample`` does) against ONE ``group=1`` call

The differences to ``group`` None are one regroup launch each way plus its output allocation; nothing here fixes a threshold.  The
rank form (``sync``) adds an all-gather of the [B, 4LH] buffer each way, whose cost over xGMI one device cannot show.

    python benchmarks/txt_group_overhead.py [--calls 100] [--rounds 5] [--out profiles/txt_group.txt]
"""
import argparse
import json
import os
import statistics
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import torch  # noqa: E402

from hipdwc import synth  # noqa: E402
from networks.networks_v2 import TxtEncoder  # noqa: E402


def setup(B, train):
    dev = torch.device("cuda:0")
    gen = synth.DEFAULT_CONFIG["gen"]
    torch.manual_seed(1)
    vocab = types.SimpleNamespace(size=synth.VOCAB_SIZE, padding_idx=synth.PAD_IDX)
    enc = TxtEncoder(vocab, gen["embed_dim"], gen["hidden_size"], gen["c_dim"], gen["num_cls"], gen["num_layers"], gen["dropout_in"],
                     gen["dropout_out"]).to(dev).train(train)
    batch = synth.make_batch(B, 8, seed=1)
    style = torch.randn(B, gen["c_dim"] * gen["num_cls"], device=dev).requires_grad_(train)
    return enc, style, batch["txt"].to(dev), batch["txt_lens"]


def training(B):
    enc, style, tokens, lens = setup(B, True)
    leaves = list(enc.parameters()) + [style]

    def step(group):
        def fn():
            for p in leaves:                                       # (as the solver's zero_grad: no accumulating add per leaf)
                p.grad = None
            mu, lv = enc(style, tokens, lens, group=group)
            (mu.flat.sum() + lv.flat.sum()).backward()
        return fn
    return {"group_none": step(None), "group_1": step(1), "group_%d" % (B // 8): step(B // 8)}


def inference(B):
    enc, style, tokens, lens = setup(B, False)

    def single():
        with torch.no_grad():
            for i in range(B):
                enc(style[i:i + 1], tokens[i:i + 1], lens[i:i + 1])

    def batched():
        with torch.no_grad():
            enc(style, tokens, lens, group=1)
    return {"batch_1_calls": single, "one_group_1_call": batched}


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps                          # us per call


def measure(fns, calls, rounds):
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for name, fn in fns.items():
            t = events(fn, calls)
            if r:
                times[name].append(t)
    return {name + "_us": {"median": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1)} for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "txt_group.txt"))
    args = ap.parse_args()
    lines = []
    for what, table, batches in (("train_fwd_bwd", training, (16, 128)), ("eval_fwd", inference, (8, 64))):
        for B in batches:
            res = {"what": what, "B": B, "calls": args.calls if what != "eval_fwd" else max(1, args.calls // 10), "rounds": args.rounds}
            res.update(measure(table(B), res["calls"], args.rounds))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("benchmarks/txt_group_overhead.py (us per call: median and max - min over the rounds; variants alternate)\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
