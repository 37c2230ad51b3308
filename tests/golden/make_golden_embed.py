#!/usr/bin/env python3
"""Record the fixture of ``TxtEncoder.forward_embed`` (reference networks_v2.py:256-293) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden.py, whose helpers it imports); tests/test_txt_embed.py reads
the file it writes:

    python tests/golden/make_golden_embed.py          # txt_embed.npz; seconds

* the reference ``TxtEncoder`` with E 12, S 8 (c_dim 2 x 4 classes), H 8, 2 layers, vocab 11, seq_len 7, eval mode: its
  ``state_dict`` under ``state/<key>``;
* per case (lengths [5, 3, 3, 1] and [4]; the reference takes decreasing lengths only) under ``<case>/``:
  ``tokens``, ``lengths``, ``style``, ``emb`` = embed_tokens(tokens) with NaN behind each length, the upstream weights ``r_mu`` /
  ``r_lv`` of the loss sum(mu * r_mu) + sum(logvar * r_lv); ``mu`` / ``lv`` of ``forward_embed`` (the K heads concatenated along
  dim 1) and the gradients ``g/<name>`` with respect to emb, style, lstm.weight_ih_l0, lstm.weight_hh_l1_reverse and fcs.0.weight;
  the same from the module in float64 (``mu64``, ``lv64``, ``g64/<name>``; emb, style and weights are the fp32 values, exactly
  representable); ``mu_tok`` / ``lv_tok``: ``forward`` on the tokens.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import_reference, t2n)

E, C_DIM, N_CLS, H, LAYERS, VOCAB, SEQ, PAD = 12, 2, 4, 8, 2, 11, 7, 0
CASES = {
    "b4": ([5, 3, 3, 1], [[4, 7, 4, 9, 1, 0, 0], [2, 4, 9, 0, 0, 0, 0], [10, 3, 2, 0, 0, 0, 0], [7, 0, 0, 0, 0, 0, 0]]),
    "b1": ([4], [[5, 5, 3, 8, 0, 0, 0]]),
}
GRADS = ("lstm.weight_ih_l0", "lstm.weight_hh_l1_reverse", "fcs.0.weight")


def run(enc, emb, style, lens, r_mu, r_lv):
    """forward_embed + backward of the loss on ``enc`` (any dtype): mu, lv, name -> gradient."""
    dt = next(enc.parameters()).dtype
    emb, style = emb.detach().to(dt).clone().requires_grad_(True), style.detach().to(dt).clone().requires_grad_(True)
    enc.zero_grad()
    mus, lvs = enc.forward_embed(style, emb, lens)
    mu, lv = torch.cat(mus, 1), torch.cat(lvs, 1)
    ((mu * r_mu.to(dt)).sum() + (lv * r_lv.to(dt)).sum()).backward()
    grads = {"emb": emb.grad, "style": style.grad}
    params = dict(enc.named_parameters())
    for n in GRADS:
        grads[n] = params[n].grad.clone()
    return mu, lv, grads


def main():
    _, _, ref_v2, _, _ = mg.import_reference()
    torch.manual_seed(31)
    vocab = types.SimpleNamespace(size=VOCAB, padding_idx=PAD, itos=[str(i) for i in range(VOCAB)])
    enc = ref_v2.TxtEncoder(vocab, E, H, C_DIM, N_CLS, LAYERS, dropout_in=0.1, dropout_out=0.1).eval()
    enc64 = copy.deepcopy(enc).double()
    out = {"state/" + k: mg.t2n(v) for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(32)
    for name, (lens, rows) in CASES.items():
        B = len(lens)
        tokens, lengths = torch.tensor(rows), torch.tensor(lens)
        style = torch.randn(B, C_DIM * N_CLS, generator=g)
        r_mu, r_lv = torch.randn(B, C_DIM * N_CLS, generator=g), torch.randn(B, C_DIM * N_CLS, generator=g)
        emb = enc.embed_tokens(tokens).detach().clone()
        for b, n in enumerate(lens):
            emb[b, n:] = float("nan")
        mu, lv, grads = run(enc, emb, style, lengths, r_mu, r_lv)
        mu64, lv64, grads64 = run(enc64, emb, style, lengths, r_mu, r_lv)
        with torch.no_grad():
            mus, lvs = enc(style, tokens, lengths)
        rec = {"tokens": tokens, "lengths": lengths, "style": style, "emb": emb, "r_mu": r_mu, "r_lv": r_lv, "mu": mu, "lv": lv,
               "mu64": mu64, "lv64": lv64, "mu_tok": torch.cat(mus, 1), "lv_tok": torch.cat(lvs, 1)}
        rec.update({"g/" + k: v for k, v in grads.items()})
        rec.update({"g64/" + k: v for k, v in grads64.items()})
        for k, v in rec.items():
            out["%s/%s" % (name, k)] = mg.t2n(v)
    path = os.path.join(HERE, "txt_embed.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
