"""Synchronised batch norm over a real process group on CPU: two gloo ranks, the stock-op form of hipdwc.syncbn through
``GroupSync`` (the GPU runs use the same exchange over RCCL).  Each rank's y / dx equal its slice of the full-batch float64 result,
the running buffers are bit-identical across the ranks, and the rank-averaged dgamma / dbeta are the full-batch values over R."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["DWC_BN_HIP"] = "0"
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import networks.networks as nets
        from hipdwc import dp, syncbn
        C, Bs, S = 6, 2, 2
        g = torch.Generator().manual_seed(21)                       # the same global batch on both ranks
        full = {"x": torch.cat([torch.randn(world * Bs, C, 4, 3, generator=g, dtype=torch.float64) * (1 + j) + 3 * j +
                                4.0 * torch.arange(world * Bs, dtype=torch.float64)[:, None, None, None] for j in range(S)]),
                "gy": torch.randn(S * world * Bs, C, 4, 3, generator=g, dtype=torch.float64)}
        # a segment's samples are contiguous in the global batch: shard each segment, as the trainer's concatenation of sharded parts
        mine = {k: torch.cat([dp.shard_batch({k: seg}, rank, world)[k] for seg in v.chunk(S)]) for k, v in full.items()}
        ref = torch.nn.BatchNorm2d(C).double()
        mod = nets.SegmentedBatchNorm2d(C).double()
        with torch.no_grad():
            for m in (ref, mod):
                m.weight.copy_(torch.linspace(-1.0, 1.5, C))
                m.bias.copy_(torch.linspace(0.3, -0.2, C))
        mod.sync = syncbn.GroupSync()
        xr = full["x"].clone().requires_grad_(True)
        want = torch.cat([F.leaky_relu(ref(seg), 0.1) for seg in xr.chunk(S)])
        (want * full["gy"]).sum().backward()                         # a toy loss: a sum over samples, so shards add up to it

        x = mine["x"].clone().requires_grad_(True)
        y = mod(x, act="lrelu", segments=S)
        (y * mine["gy"]).sum().backward()

        def my_slice(t):
            return torch.cat([seg[rank * Bs:(rank + 1) * Bs] for seg in t.chunk(S)])
        errs = {"y": _rel(y.detach(), my_slice(want.detach())), "dx": _rel(x.grad, my_slice(xr.grad)),
                "running_mean": _rel(mod.running_mean, ref.running_mean), "running_var": _rel(mod.running_var, ref.running_var)}
        dp.GradAllReduce()([mod.weight, mod.bias])                   # averages, like the trainer's reducer
        errs["dgamma"] = _rel(mod.weight.grad, ref.weight.grad / world)
        errs["dbeta"] = _rel(mod.bias.grad, ref.bias.grad / world)
        bufs = torch.cat([mod.running_mean, mod.running_var])
        both = [torch.zeros_like(bufs) for _ in range(world)]
        dist.all_gather(both, bufs)
        same = all(torch.equal(both[0], t) for t in both)
        ok = mod.sync.calls == 2 and int(mod.num_batches_tracked) == S and type(y.grad_fn).__name__.startswith("_SyncBatchNormTorch")
        q.put((rank, errs, bool(same), bool(ok), ""))
        dist.destroy_process_group()
    except Exception as e:  # surface the failure in the parent
        import traceback
        q.put((rank, {}, False, False, repr(e) + traceback.format_exc()[-800:]))


def test_sync_bn_world2_gloo():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, errs, same, ok, why in sorted(results, key=lambda r: r[0]):
        assert not why, (rank, why)
        assert same, "rank %d: running buffers differ between the ranks" % rank
        assert ok, rank
        for k, lim in (("y", 1e-12), ("dx", 1e-10), ("dgamma", 1e-10), ("dbeta", 1e-10), ("running_mean", 1e-12),
                       ("running_var", 1e-12)):
            assert errs[k] <= lim, (rank, k, errs[k])
