"""What ``TxtEncoder.forward_embed`` costs beside ``forward`` (csrc/txt_glue.hip ``dwc_txt_operand_embed_*``).

One ``TxtEncoder`` forward + backward (embed 300, style 64, hidden 300, two layers, both dropouts 0.1: the shipped generator
configuration) at B = 16 and B = 128 on the tokens and lengths ``synth.make_batch`` draws.  Three variants ALTERNATE inside one
process: ``--rounds`` windows of ``--calls`` back-to-back calls each between device events (round 0 warms all three up and is not
counted); per variant the median and max - min over the rounds:

  (a) tokens        ``forward(tokens)``: the table lookup, gradient into the table
  (b) embed         ``forward_embed(embed_tokens(tokens).detach())``, gradient into the embeddings
  (c) embed_stock   (b) with ``ops.TXT_FUSED = 0``: the stock-tensor-op expression

    python benchmarks/txt_embed_overhead.py [--calls 100] [--rounds 5] [--batches 16,128]
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

from hipdwc import ops, synth  # noqa: E402
from networks.networks_v2 import TxtEncoder  # noqa: E402


def setup(B):
    dev = torch.device("cuda:0")
    gen = synth.DEFAULT_CONFIG["gen"]
    torch.manual_seed(1)
    vocab = types.SimpleNamespace(size=synth.VOCAB_SIZE, padding_idx=synth.PAD_IDX)
    enc = TxtEncoder(vocab, gen["embed_dim"], gen["hidden_size"], gen["c_dim"], gen["num_cls"], gen["num_layers"], gen["dropout_in"],
                     gen["dropout_out"]).to(dev).train()
    batch = synth.make_batch(B, 8, seed=1)
    style = torch.randn(B, gen["c_dim"] * gen["num_cls"], device=dev).requires_grad_(True)
    tokens = batch["txt"].to(dev)
    emb = enc.embed_tokens(tokens).detach().requires_grad_(True)
    return enc, style, tokens, emb, batch["txt_lens"]


def variants(enc, style, tokens, emb, lens):
    leaves = list(enc.parameters()) + [style, emb]

    def step(fused, call):
        def fn():
            ops.TXT_FUSED = fused
            for p in leaves:                                       # (as the solver's zero_grad: no accumulating add per leaf)
                p.grad = None
            mu, lv = call()
            (mu.flat.sum() + lv.flat.sum()).backward()
        return fn
    return {"tokens": step(1, lambda: enc(style, tokens, lens)),
            "embed": step(1, lambda: enc.forward_embed(style, emb, lens)),
            "embed_stock": step(0, lambda: enc.forward_embed(style, emb, lens))}


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps                          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="16,128")
    args = ap.parse_args()
    keep = ops.TXT_FUSED
    for B in (int(b) for b in args.batches.split(",")):
        enc, style, tokens, emb, lens = setup(B)
        fns = variants(enc, style, tokens, emb, lens)
        times = {k: [] for k in fns}
        for r in range(args.rounds + 1):
            for name, fn in fns.items():
                t = events(fn, args.calls)
                if r:
                    times[name].append(t)
        res = {"B": B, "t_max": int(lens.max()), "what": "fwd_bwd", "calls": args.calls, "rounds": args.rounds}
        for name, v in times.items():
            res[name + "_us"] = {"median": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1)}
        res["embed_minus_tokens_us"] = round(res["embed_us"]["median"] - res["tokens_us"]["median"], 1)
        res["stock_minus_embed_us"] = round(res["embed_stock_us"]["median"] - res["embed_us"]["median"], 1)
        print(json.dumps(res), flush=True)
    ops.TXT_FUSED = keep


if __name__ == "__main__":
    main()
