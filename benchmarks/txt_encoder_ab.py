"""What the fused data movement of the text encoder (csrc/txt_glue.hip, hipdwc/txt.py) is worth at kernel level.

One ``TxtEncoder`` forward + backward (embed 300, hidden 300, two layers, both dropouts 0.1, trainable table: the shipped generator
configuration) on synthetic tokens at the c1 shape (B = 16) and the c2 shape (B = 128), longest sequence 40.  The two paths
(``ops.TXT_FUSED`` 0 and 1) ALTERNATE inside one process: ``--rounds`` windows of ``--calls`` back-to-back calls each between device
events (round 0 warms both up and is not counted); per path the median and min .. max over the rounds, forward alone (no tape, as
``dis_update`` runs it) and forward + backward.

``TXT_FUSED = 0`` is NOT the state before the fused path existed: both paths share ``ops.lstm_layer_bwd``, i.e. the one-launch
previous-state tensor, the transposed ``w_hh`` / bias sum kept per optimiser step and the single re-layout copy per weight gradient.
What those gained is in neither column's difference; only a whole-step A/B of two checkouts shows it.

    python benchmarks/txt_encoder_ab.py [--calls 20] [--rounds 5] [--shapes c1,c2]
    python benchmarks/txt_encoder_ab.py --once [--fused 0|1] [--shape c1]     # one warm-up and ONE forward + backward, for a kernel
                                                                             # trace: the launches between the three prefix-sum
                                                                             # (cumsum) kernels are the forward's and the backward's
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

BATCH = {"c1": 16, "c2": 128}


def setup(shape):
    dev = torch.device("cuda:0")
    B = BATCH[shape]
    gen = synth.DEFAULT_CONFIG["gen"]
    torch.manual_seed(1)
    vocab = types.SimpleNamespace(size=synth.VOCAB_SIZE, padding_idx=synth.PAD_IDX)
    enc = TxtEncoder(vocab, gen["embed_dim"], gen["hidden_size"], gen["c_dim"], gen["num_cls"], gen["num_layers"], gen["dropout_in"],
                     gen["dropout_out"]).to(dev).train()
    batch = synth.make_batch(B, 8, seed=1)
    lens = batch["txt_lens"].clone()
    lens[0] = 40                                                   # the longest sequence the loader hands out: T = 40 in every run
    style = torch.randn(B, gen["c_dim"] * gen["num_cls"], device=dev).requires_grad_(True)
    return enc, style, batch["txt"].to(dev), lens


def calls(enc, style, tokens, lens):
    def fwd():
        with torch.no_grad():
            enc(style, tokens, lens)

    params = list(enc.parameters())

    def fwd_bwd():
        for p in params + [style]:                                 # (as the solver's zero_grad: no accumulating add per parameter)
            p.grad = None
        mu, lv = enc(style, tokens, lens)
        (mu.flat.sum() + lv.flat.sum()).backward()
    return {"fwd": fwd, "fwd_bwd": fwd_bwd}


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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c2")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--fused", type=int, default=1)
    ap.add_argument("--shape", default="c1")
    args = ap.parse_args()
    if args.once:
        ops.TXT_FUSED = args.fused
        enc, style, tokens, lens = setup(args.shape)
        calls(enc, style, tokens, lens)["fwd_bwd"]()
        torch.cuda.synchronize()
        for p in list(enc.parameters()) + [style]:
            p.grad = None
        # three prefix-sum launches (a kernel the encoder never runs) fence the traced forward and the traced backward
        fence = torch.ones(64, device=style.device)
        torch.cumsum(fence, 0)
        mu, lv = enc(style, tokens, lens)
        torch.cumsum(fence, 0)
        (mu.flat.sum() + lv.flat.sum()).backward()
        torch.cumsum(fence, 0)
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "shape": args.shape, "fused": args.fused}))
        return
    for shape in args.shapes.split(","):
        fns = calls(*setup(shape))
        for what, fn in fns.items():
            times = {0: [], 1: []}
            for r in range(args.rounds + 1):
                for fused in (0, 1):
                    ops.TXT_FUSED = fused
                    t = events(fn, args.calls)
                    if r:
                        times[fused].append(t)
            res = {"shape": shape, "B": BATCH[shape], "what": what, "calls": args.calls, "rounds": args.rounds}
            for fused, label in ((0, "stock"), (1, "fused")):
                v = times[fused]
                res[label + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            res["saved_us"] = round(res["stock_us"]["median"] - res["fused_us"]["median"], 1)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
