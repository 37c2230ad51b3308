"""What the device half of the output pipeline costs beside the two ways of doing without it (csrc/image_out_u8.hip,
hipdwc.u8image.grid_u8 / image_to_u8).

Two workloads, each ending with the bytes in (pinned) host memory, ready for PIL:

  grid    the reference's sample grid: five fp32 [8, 3, 128, 128] tensors -> uint8 [640, 1024, 3], range from the data
  images  a translated batch: one bf16 NHWC8 buffer [128, 8, 128, 128] -> uint8 [128, 128, 128, 3], range (-1, 1)

Three routes:

  (a) hip     grid_u8 / image_to_u8, then a non-blocking copy of the bytes and an event wait (what utils.write_grid does)
  (b) torch   the same chain as torch device ops (cat / min / max / clamp / sub / div / mul / add / permute / to(uint8)), then the
              same copy and wait; the range costs it two host synchronisations on the grid workload
  (c) cpu     .cpu() of the fp32 tensors, then the chain on the CPU (torch's default thread count)

Per route and workload: ``wall_us``, host clock per call of calls that each wait until the bytes are on the host, and for (a) and
(b) ``device_us``, HIP-event time per call of ``--calls`` calls enqueued back to back (copies included).  The routes ALTERNATE inside
one process: ``--rounds`` windows each (round 0 warms up and is not counted); per figure the median and max - min over the rounds.
The three routes' bytes are compared once before anything is timed.

    python benchmarks/u8_out_overhead.py [--calls 30] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dwc-gan_amd"))
import torch  # noqa: E402


def to_bytes(t):
    """The byte conversion of save_image on a normalised fp32 [..., 3, H, W] tensor -> uint8 [..., H, W, 3]."""
    return t.mul(255).add_(0.5).clamp_(0, 255).movedim(-3, -1).to(torch.uint8).contiguous()


def chain_grid(tensors, n):
    """make_grid(nrow=n, padding=0, normalize=True) + to_bytes on whatever device the tensors are on; n images of each."""
    t = torch.cat([x[:n] for x in tensors])
    lo, hi = float(t.min()), float(t.max())
    t.clamp_(lo, hi).sub_(lo).div_(max(hi - lo, 1e-5))
    N, C, H, W = t.shape
    return to_bytes(t.view(N // n, n, C, H, W).permute(2, 0, 3, 1, 4).reshape(C, N // n * H, n * W))


def chain_images(x):
    """fp32 [B, 3, H, W] in (-1, 1) -> uint8 [B, H, W, 3]."""
    return to_bytes(x.clamp(-1.0, 1.0).sub_(-1.0).div_(2.0))


class Route:
    """``enqueue()`` puts one call's device work on the stream (and returns the host tensor it fills, or the finished bytes for the
    CPU route); ``finish()`` waits for that call's bytes."""

    def __init__(self, make_u8, shape, on_cpu=False):
        self.make_u8, self.on_cpu = make_u8, on_cpu
        self.host = torch.empty(shape, dtype=torch.uint8, pin_memory=True)
        self.done = torch.cuda.Event()

    def enqueue(self):
        if self.on_cpu:
            return self.make_u8()
        self.host.copy_(self.make_u8(), non_blocking=True)
        self.done.record()
        return self.host

    def finish(self):
        if not self.on_cpu:
            self.done.synchronize()

    def result(self):
        out = self.enqueue()
        self.finish()
        return out.clone()


def device_us(route, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        route.enqueue()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def wall_us(route, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        route.enqueue()
        route.finish()
    return 1e6 * (time.perf_counter() - t0) / calls


def run(what, routes, calls, rounds, extra):
    first = routes["hip"].result()
    for name, r in routes.items():
        differing = int((r.result() != first).sum())
        if differing:
            raise SystemExit("%s: route %s differs from hip in %d bytes" % (what, name, differing))
    times = {(name, kind): [] for name, r in routes.items() for kind in ("device_us", "wall_us") if not (r.on_cpu and kind == "device_us")}
    for r in range(rounds + 1):
        for kind, fn in (("device_us", device_us), ("wall_us", wall_us)):
            for name, route in routes.items():
                if (name, kind) in times:
                    t = fn(route, calls)
                    if r:
                        times[(name, kind)].append(t)
    res = dict(what=what, calls=calls, rounds=rounds, out_bytes=first.numel(), cpu_threads=torch.get_num_threads(), **extra)
    for (name, kind), v in times.items():
        res["%s_%s" % (name, kind)] = {"median": round(statistics.median(v), 1), "spread": round(max(v) - min(v), 1),
                                       "windows": [round(t, 1) for t in v]}
    for kind in ("device_us", "wall_us"):
        res["hip_minus_torch_%s" % kind] = round(res["hip_" + kind]["median"] - res["torch_" + kind]["median"], 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this benchmark needs the GPU: there is no CPU stand-in for the device routes")
    from hipdwc import ops, u8image
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    n, size = 8, 128
    outs = [(torch.randn(n, 3, size, size, generator=g) * 0.5).to(dev) for _ in range(5)]
    shape = (5 * size, n * size, 3)
    run("grid", {"hip": Route(lambda: u8image.grid_u8(outs, n), shape),
                 "torch": Route(lambda: chain_grid(outs, n), shape),
                 "cpu": Route(lambda: chain_grid([x.cpu() for x in outs], n), shape, on_cpu=True)},
        args.calls, args.rounds, {"in_bytes": sum(x.numel() * 4 for x in outs)})

    B = 128
    ops.set_precision("bf16")
    try:
        buf = ops.pack_image(torch.rand(B, 3, size, size, generator=g).mul_(2.4).sub_(1.2).to(dev))
        assert ops.is_image(buf) and buf.dtype == torch.bfloat16
        shape = (B, size, size, 3)
        run("images", {"hip": Route(lambda: u8image.image_to_u8(buf), shape),
                       "torch": Route(lambda: chain_images(buf[:, :3].float()), shape),
                       "cpu": Route(lambda: chain_images(buf[:, :3].float().cpu()), shape, on_cpu=True)},
            args.calls, args.rounds, {"in_bytes": buf.numel() * 2})
    finally:
        ops.set_precision("fp32")


if __name__ == "__main__":
    main()
