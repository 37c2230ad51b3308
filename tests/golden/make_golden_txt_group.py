#!/usr/bin/env python3
"""Record the fixture of the grouped text encoder (``TxtEncoder(group=G)``) by IMPORTING the reference.

Runs only where the reference tree is available (like make_golden_embed.py); tests/test_txt_group.py reads the file it writes:

    python tests/golden/make_golden_txt_group.py          # txt_group.npz; seconds

* the reference ``TxtEncoder`` with E 12, S 12 (c_dim 4 x 3 classes), H 16, 2 layers, vocab 11, seq_len 7, eval mode: its
  ``state_dict`` under ``state/<key>``;
* one batch of 6 samples with unequal lengths: ``tokens``, ``lengths``, ``style``, and the upstream weights ``r_mu`` / ``r_lv`` of the
  loss sum(mu * r_mu) + sum(logvar * r_lv);
* per group size G in 1, 2, 3 under ``g<G>/``: the reference ``forward`` called ONCE PER GROUP of G consecutive samples -- ``mu`` /
  ``lv`` [6, 12] (the K heads concatenated along dim 1, the groups along dim 0), the same from the module in float64 (``mu64`` /
  ``lv64``) and ``g64``: the float64 gradients of the loss with respect to every parameter, in ``state_dict`` order, and then to
  ``style``, summed over the groups, flattened into ONE vector (an archive member costs ~300 bytes of headers; tokens, style and
  weights are the fp32 values, exactly representable).

Size.  The file has to stay below tiny_bn_step.npz, and 3 x 15 000 float64 gradients alone do not (random mantissas do not compress).
Two measures, both made BEFORE / AFTER the reference runs, never in between: the seeded weights are rounded to 8 mantissa bits
before the first call (the encoder under test is that rounded one; its state packs to half), and each recorded float64 gradient is
rounded to nearest at 28 mantissa bits (``keep28``: relative 2^-29, 1/64 of the fp32 spacing that floors the test's bound).
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

E, C_DIM, N_CLS, H, LAYERS, VOCAB, SEQ, PAD = 12, 4, 3, 16, 2, 11, 7, 0
LENS = [3, 7, 1, 5, 2, 4]
ROWS = [[4, 7, 4, 0, 0, 0, 0], [2, 4, 9, 1, 10, 3, 6], [10, 0, 0, 0, 0, 0, 0], [7, 8, 5, 5, 3, 0, 0], [6, 1, 0, 0, 0, 0, 0],
        [9, 2, 8, 4, 0, 0, 0]]
GROUPS = (1, 2, 3)


def keep28(t):
    """float64 ``t`` rounded to nearest at 28 mantissa bits: the low three bytes of every value are zero and pack to nothing."""
    bits = t.detach().double().contiguous().view(torch.int64)
    return ((bits + (1 << 23)) & ~((1 << 24) - 1)).view(torch.float64)


def run(enc, tokens, lengths, style, r_mu, r_lv, G):
    """The reference forward once per group of G samples + backward of the loss: mu, lv, name -> gradient summed over the groups."""
    dt = next(enc.parameters()).dtype
    style = style.detach().to(dt).clone().requires_grad_(True)
    enc.zero_grad()
    mus, lvs = [], []
    for a in range(0, len(LENS), G):
        m, v = enc(style[a:a + G], tokens[a:a + G], lengths[a:a + G])
        mus.append(torch.cat(m, 1))
        lvs.append(torch.cat(v, 1))
    mu, lv = torch.cat(mus), torch.cat(lvs)
    ((mu * r_mu.to(dt)).sum() + (lv * r_lv.to(dt)).sum()).backward()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    grads["style"] = style.grad
    return mu, lv, grads


def main():
    _, _, ref_v2, _, _ = mg.import_reference()
    torch.manual_seed(41)
    vocab = types.SimpleNamespace(size=VOCAB, padding_idx=PAD, itos=[str(i) for i in range(VOCAB)])
    enc = ref_v2.TxtEncoder(vocab, E, H, C_DIM, N_CLS, LAYERS, dropout_in=0.1, dropout_out=0.1).eval()
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    enc64 = copy.deepcopy(enc).double()
    out = {"state/" + k: mg.t2n(v) for k, v in enc.state_dict().items()}
    g = torch.Generator().manual_seed(42)
    B, S = len(LENS), C_DIM * N_CLS
    tokens, lengths = torch.tensor(ROWS), torch.tensor(LENS)
    style, r_mu, r_lv = torch.randn(B, S, generator=g), torch.randn(B, S, generator=g), torch.randn(B, S, generator=g)
    for k, v in (("tokens", tokens), ("lengths", lengths), ("style", style), ("r_mu", r_mu), ("r_lv", r_lv)):
        out[k] = mg.t2n(v)
    for G in GROUPS:
        mu, lv, _ = run(enc, tokens, lengths, style, r_mu, r_lv, G)
        mu64, lv64, grads64 = run(enc64, tokens, lengths, style, r_mu, r_lv, G)
        rec = {"mu": mu, "lv": lv, "mu64": mu64, "lv64": lv64}
        assert list(grads64) == list(enc.state_dict()) + ["style"]
        rec["g64"] = keep28(torch.cat([v.reshape(-1) for v in grads64.values()]))
        for k, v in rec.items():
            out["g%d/%s" % (G, k)] = mg.t2n(v)
    path = os.path.join(HERE, "txt_group.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "tiny_bn_step.npz"))
    print("wrote %s: %d arrays, %d bytes (limit %d)" % (path, len(out), size, limit))
    assert size < limit


if __name__ == "__main__":
    main()
