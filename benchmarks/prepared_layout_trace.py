#!/usr/bin/env python
"""Call trace and bits of everything hipdwc.ops keeps per parameter: prepared weight layouts, concatenated parameters, the LSTM's
transposed recurrent weights and bias sum, the float of a constant.

The check behind a refactor of those caches, by the scheme of benchmarks/conv_call_trace.py (whose Recorder this file uses): run it on
the tree before and on the tree after, then compare the two outputs as text.

    python benchmarks/prepared_layout_trace.py --out before.txt        (on the parent)
    python benchmarks/prepared_layout_trace.py --out after.txt         (on the branch)
    python benchmarks/prepared_layout_trace.py --compare before.txt after.txt
    python benchmarks/prepared_layout_trace.py --time 100000           (hit-path time of the four caches, one repeat, one JSON line)

It calls ops._prepped, ops.refresh_prepared, ops.cat_params, ops.lstm_bidir and ops.gmm_kl_sp only, and reads ops._REFRESH_TABLES (the
descriptor tables as the C side receives them) for the recipe fields.  Per layout case, four stages:
  build      first call                                          C calls, SHA-256 of the prepared tensor
  hit        second call                                         no C call, the same tensor object
  lazy       in-place update of the weight, then a call          C calls, SHA-256
  refreshed  in-place update, ops.refresh_prepared, then a call  C calls, layouts rebuilt, descriptor fields, same address, SHA-256
"""
import argparse
import hashlib
import json
import os
import sys
import timeit
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "dwc-gan_amd"), REPO, os.path.join(REPO, "benchmarks")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from conv_call_trace import Recorder, compare  # noqa: E402

IM2COL = [(k, h) for k in ("fwd", "dgrad", "dgrad_t") for h in (False, True)]
SPLIT = [(k, False) for k in ("x3_fwd", "x3_dgrad", "h2_fwd", "h2_dgrad")]


def layout_cases():
    """(filter shape, kind, cout_pad, cin_pad, stride, half) -- the shapes of tests/test_prepared_cache.py, then the layers of the
    c1 / c2 workload (128x128: 7x7 stem, two 4x4 stride-2 steps, 3x3 blocks at 256, 5x5 decoder, 7x7 heads, the style MLP as 1x1)."""
    for kind, half in IM2COL:
        cip = 8 if half else 4
        yield (8, 3, 3, 3), kind, 16, cip, 1, half
        if kind != "dgrad_t":
            yield (8, 3, 4, 4), kind, 16, cip, 2, half
    for kind, half in SPLIT:
        yield (16, 16, 3, 3), kind, 16, 16, 1, half
        yield (8, 8, 3, 3), kind, 16, 16, 1, half
    for half in (False, True):
        P = 8 if half else 4
        x3 = "" if half else "_x3"
        yield (64, 3, 7, 7), "stem_steps" + x3, 64, P, 1, half
        yield (P, 64, 7, 7), "stem_steps_dgrad" + x3, 64, P, 1, half
        yield (P, 64, 7, 7), "heads_wide", 32, 64, 1, half
        yield (P, 64, 7, 7), "heads_narrow" + x3, 32, 64, 1, half
        yield (64, 3, 7, 7), "dgrad_image", 64, P, 1, half
        yield (64, 3, 7, 7), "dgrad_image_narrow" + x3, 64, P, 1, half
    for co, ci, k, s in ((128, 64, 4, 2), (256, 128, 4, 2), (256, 256, 3, 1), (128, 256, 5, 1), (64, 128, 5, 1)):
        for kind, half in IM2COL:
            if kind != "dgrad_t" or s == 1:
                yield (co, ci, k, k), kind, co, ci, s, half
        if s == 1:
            for kind, half in SPLIT:
                yield (co, ci, k, k), kind, co, ci, 1, half
    for n, k in ((256, 8), (256, 256), (2048, 256)):
        yield (n, k, 1, 1), "fwd", n, k, 1, False


def _sha(t):
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _seeded(name, shape, scale=1.0):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(zlib.crc32(name.encode()))) * scale


def _step(p, name):
    """In-place update of a parameter, as an optimiser makes it (the version counter moves, the storage stays)."""
    import torch
    with torch.no_grad():
        p.add_(_seeded(name, tuple(p.shape), 0.05).to(p.device))


def _refresh_fields(ops):
    """Descriptor rows of the refresh tables built since the last call (all fields but the two addresses), then forgotten."""
    rows = []
    for table in ops._REFRESH_TABLES.values():
        for d in table[0].cpu().numpy().view(ops._REFRESH_DT):
            rows.append(" ".join("%s=%d" % (f, int(d[f])) for f in ops._REFRESH_DT.names if f not in ("src", "dst")))
    ops._REFRESH_TABLES.clear()
    return rows


def record(out_path):
    import torch
    from hipdwc import _lib, ops
    rec = Recorder(_lib.load(), _lib.SIGNATURES)
    _lib._lib = rec
    assert _lib.load() is rec
    dev = torch.device("cuda:0")
    lines = []

    def stage(tag, *words):
        torch.cuda.synchronize()
        lines.append("  %s %s" % (tag, " ".join(str(w) for w in words)))
        lines.extend("    " + s for s in rec.drain())

    for shape, kind, cop, cip, stride, half in layout_cases():
        name = "%s %s cop%d cip%d s%d %s" % ("x".join(map(str, shape)), kind, cop, cip, stride, "bf16" if half else "fp32")
        for owned in ("self", "pair"):
            # "pair": the filter is a fresh tensor made from two parameters (a stacked or reshaped weight), the cache lives on them
            if owned == "pair" and kind not in ("fwd", "heads_wide", "heads_narrow", "heads_narrow_x3"):
                continue
            lines.append("CASE %s %s" % (name, owned))
            w = torch.nn.Parameter(_seeded(name, shape, (shape[1] * shape[2] * shape[3]) ** -0.5).to(dev))
            if owned == "pair":
                halves = [torch.nn.Parameter(w.detach()[: shape[0] // 2].clone()), torch.nn.Parameter(w.detach()[shape[0] // 2:].clone())]
                call = lambda: ops._prepped(torch.cat([h.detach() for h in halves], 0), kind, cop, cip, stride, tuple(halves), half)
                params = halves
            else:
                call = lambda: ops._prepped(w, kind, cop, cip, stride, None, half)
                params = [w]
            ops._REFRESH_TABLES.clear()
            t = call()
            stage("build", _sha(t), tuple(t.shape), t.dtype)
            t2 = call()
            stage("hit", "same" if t2 is t else "OTHER")
            _step(params[-1], name + " lazy")
            t3 = call()
            stage("lazy", _sha(t3), "same" if t3 is t else "new")
            _step(params[-1], name + " refreshed")
            ptr = t3.data_ptr()
            n = ops.refresh_prepared(params)
            stage("refresh", n)
            lines.extend("    D " + r for r in _refresh_fields(ops))
            t4 = call()
            stage("refreshed", _sha(t4), "same" if t4 is t3 else "new", "address kept" if t4.data_ptr() == ptr else "address moved")
            del call, params, w, t, t2, t3, t4

    # concatenated / stacked parameters: without and with a graph, across one step of the last parameter
    for stack in (False, True):
        lines.append("CASE cat_params stack=%d" % stack)
        ps = [torch.nn.Parameter(_seeded("cat %d %d" % (stack, i), (6, 5)).to(dev)) for i in range(3)]
        for when in ("first", "second", "stepped"):
            if when == "stepped":
                _step(ps[-1], "cat step")
            with torch.no_grad():
                a = ops.cat_params(ps, stack)
            b = ops.cat_params(ps, stack)
            stage(when, _sha(a), _sha(b), tuple(a.shape), "grad" if b.requires_grad else "nograd")
        b.sum().backward()
        stage("backward", " ".join(_sha(p.grad) for p in ps))

    # one bidirectional LSTM layer the way networks_v2.TxtEncoder calls it; the tensors ops._lstm_derived hands out are hashed as they
    # pass (the wrapper keeps the function's signature, which both trees share)
    lines.append("CASE lstm_bidir")
    inner = ops._lstm_derived

    def logged(kind, owners, stamp, build):
        out = inner(kind, owners, stamp, build)
        lines.append("    derived %s %s" % (kind, _sha(out)))
        return out
    ops._lstm_derived = logged
    T, B, I, H = 4, 3, 32, 32
    names = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
    par = {n: [torch.nn.Parameter(_seeded("lstm %s %d" % (n, d), (4 * H, I if n == "weight_ih" else H) if n[0] == "w" else (4 * H,),
                                          0.2).to(dev)) for d in range(2)] for n in names}
    x = _seeded("lstm x", (T, B, I)).to(dev)
    lens = torch.tensor([4, 3, 1], dtype=torch.int32, device=dev)

    def layer():
        st = {n: ops.cat_params(par[n], stack=True) for n in names}
        return ops.lstm_bidir(x, lens, st["weight_ih"], st["weight_hh"], st["bias_ih"], st["bias_hh"], owners=tuple(par["weight_ih"]),
                              owners_hh=tuple(par["weight_hh"]), owners_b=tuple(par["bias_ih"] + par["bias_hh"]))
    out, c = layer()
    stage("forward", _sha(out), _sha(c))
    out2, _ = layer()
    stage("forward again", _sha(out2))
    for n in names:                              # the step falls between a forward and its backward: the backward reads the old values
        _step(par[n][1], "lstm step " + n)
    out3, c3 = layer()
    stage("forward stepped", _sha(out3), _sha(c3))
    (out.sum() + c.sum()).backward()
    stage("backward of the first forward", " ".join(_sha(p.grad) for n in names for p in par[n]))
    (out3.sum() + c3.sum()).backward()
    stage("backward of the stepped forward", " ".join(_sha(p.grad) for n in names for p in par[n]))
    ops._lstm_derived = inner

    lines.append("CASE gmm_kl_sp")
    sigma = torch.tensor(0.3, device=dev)
    mu, lv = (_seeded("gmm %d" % i, (4, 3, 8)).to(dev) for i in range(2))
    centre = _seeded("gmm centre", (4, 3)).to(dev)
    for when in ("first", "second", "changed"):
        if when == "changed":
            sigma.fill_(0.5)
        stage(when, _sha(ops.gmm_kl_sp(mu, lv, centre, sigma)))

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases, %d lines -> %s" % (sum(1 for s in lines if s.startswith("CASE ")), len(lines), out_path))
    return 0


def hit_time(calls):
    """One repeat: microseconds per call on the hit path of each cache."""
    import torch
    from hipdwc import ops
    dev = torch.device("cuda:0")
    w = torch.nn.Parameter(torch.randn(64, 64, 3, 3, device=dev))
    a, b = (torch.nn.Parameter(torch.randn(32, 64, 1, 1, device=dev)) for _ in range(2))
    w2 = torch.cat([a.detach(), b.detach()], 0)
    ps = [torch.nn.Parameter(torch.randn(6, 5, device=dev)) for _ in range(4)]
    sigma = torch.tensor(0.3, device=dev)
    runs = {"prepped_one_owner": lambda: ops._prepped(w, "fwd", 64, 64, 1, None, False),
            "prepped_owner_pair": lambda: ops._prepped(w2, "fwd", 64, 64, 1, (a, b), False),
            "cat_params_no_grad": lambda: ops.cat_params(ps),
            "scalar_value": lambda: ops._scalar_value(sigma)}
    out = {}
    with torch.no_grad():
        for name, fn in runs.items():
            fn()
            torch.cuda.synchronize()
            out[name] = round(timeit.timeit(fn, number=calls) / calls * 1e6, 4)
    print(json.dumps({"hit_us": out, "calls": calls}))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="run the table and write the trace here")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two traces")
    ap.add_argument("--time", type=int, default=0, metavar="CALLS", help="time the hit paths over this many calls")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.time:
        sys.exit(hit_time(args.time))
    if not args.out:
        ap.error("--out FILE, --compare BEFORE AFTER or --time CALLS")
    sys.exit(record(args.out))
