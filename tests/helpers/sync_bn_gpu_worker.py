"""Rank process of test_two_rank_rccl_sync_bn (launched with torch.distributed.run, one rank per GPU, backend nccl = RCCL).

Two data-parallel training iterations of the tiny configuration with dis.norm 'bn' and ``enable_data_parallel(sync_bn=True)``: every
batch-norm layer exchanges its moments and backward sums over RCCL.  Afterwards every parameter of G and D AND every batch-norm
buffer must be bit-identical across the ranks (without synchronisation the buffers are each rank's own), each layer must have issued
two all-gathers per taped call, and no per-rank-statistics warning may have been raised."""
import json
import os
import sys
import warnings

import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(REPO, "dwc-gan_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from hipdwc import dp, host, synth            # noqa: E402
from solver import Solver                     # noqa: E402


def main():
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", device_id=dev)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    cfg["dis"]["norm"] = "bn"
    host.set_noise(host.HostNoise())
    torch.manual_seed(1234)
    trainer = Solver(cfg, dev, None).to(dev)
    dp.broadcast_module(trainer.gen)
    dp.broadcast_module(trainer.dis)
    trainer.copy_nets()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        trainer.enable_data_parallel(bucket_bytes=64 << 10, sync_bn=True)
    full = synth.make_batch(2 * world, 32, seed=5)
    mine = {k: v.to(dev) for k, v in dp.shard_batch(full, rank, world).items()}      # different samples on every rank
    for it in range(2):
        torch.manual_seed(777 + 10 * it + rank)
        a = (mine["x_real"], mine["c_src"], mine["c_trg"], mine["txt"], mine["txt_lens"], mine["label_src"], mine["label_trg"],
             cfg, it)
        trainer.dis_update(*a)
        trainer.gen_update(*a)
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
    torch.cuda.synchronize()

    def same(tensors):
        flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
        gathered = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(gathered, flat)
        return bool(all(torch.equal(gathered[0], g) for g in gathered))
    layers = trainer.dis.bn_layers()
    buffers = [b for m in layers for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
    res = {"rank": rank, "same_params": same(list(trainer.gen.parameters()) + list(trainer.dis.parameters())),
           "same_buffers": same(buffers), "buffers_moved": bool(any(m.running_mean.abs().max() > 0 for m in layers)),
           "all_gathers": [m.sync.calls for m in layers], "worlds": [m.sync.world for m in layers],
           "warnings": [str(w.message) for w in caught if "bn" in str(w.message)]}
    print("SYNCBNRESULT " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
