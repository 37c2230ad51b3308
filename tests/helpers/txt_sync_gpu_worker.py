"""Rank process of test_two_rank_rccl_txt_sync (launched with torch.distributed.run, one rank per GPU, backend nccl = RCCL).

The tiny configuration's generator in eval mode, ``enable_data_parallel(sync_txt=True)``: every rank encodes its 3 of 6 sentences, the
text encoder gathers the ranks' feature buffers (and, in the backward, their gradients) over RCCL.  Every rank then runs the
single-process emulation -- the same encoder without ``sync`` on all 6 samples -- and reports how far its own rows of ``mu`` /
``logvar`` and of the style gradient are from it, relative to the emulation's scale."""
import json
import os
import sys

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "dwc-gan_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from hipdwc import dp, host, synth            # noqa: E402
from networks.networks_v2 import flat_heads   # noqa: E402
from solver import Solver                     # noqa: E402

PER_RANK = 3


def encode(gen, style, txt, lens):
    style = style.clone().requires_grad_(True)
    mu, lv = gen.encode_txt(style, txt, lens)
    mu, lv = flat_heads(mu), flat_heads(lv)
    (mu.sum() + 2.0 * lv.sum()).backward()
    return mu.detach(), lv.detach(), style.grad.detach()


def main():
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", device_id=dev)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    host.set_noise(host.HostNoise())
    torch.manual_seed(1234)
    trainer = Solver(cfg, dev, None).to(dev)
    dp.broadcast_module(trainer.gen)
    trainer.enable_data_parallel(bucket_bytes=64 << 10, sync_txt=True)
    gen = trainer.gen.eval()
    sync = gen.enc_txt.sync
    B = PER_RANK * world
    full = synth.make_batch(B, 32, seed=5)
    style = torch.randn(B, cfg["gen"]["c_dim"] * cfg["gen"]["num_cls"], generator=torch.Generator().manual_seed(6))
    txt, lens, style = full["txt"].to(dev), full["txt_lens"].to(dev), style.to(dev)
    rows = slice(rank * PER_RANK, (rank + 1) * PER_RANK)
    got = encode(gen, style[rows], txt[rows], lens[rows])
    gathers = sync.calls
    gen.enc_txt.sync = None                                       # the emulation: one device, the concatenated batch, group None
    want = encode(gen, style, txt, lens)
    errs = [float((g - w[rows]).abs().max() / w.abs().max()) for g, w in zip(got, want)]
    res = {"rank": rank, "world": sync.world, "all_gathers": gathers, "errs": errs,
           "finite": bool(all(torch.isfinite(g).all() for g in got))}
    print("TXTSYNCRESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
