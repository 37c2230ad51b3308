#!/usr/bin/env python
"""Call trace and result bits of the convolution autograd nodes (hipdwc.ops: conv2d, conv2d_padded, conv2d_heads, conv2d_zeropad).

The check behind a refactor of those nodes: run this file on the tree before and on the tree after, then compare the two outputs.

    python benchmarks/conv_call_trace.py --out before.txt          (on the parent)
    python benchmarks/conv_call_trace.py --out after.txt           (on the branch)
    python benchmarks/conv_call_trace.py --compare before.txt after.txt

What is recorded, per case of the table below (seeded forward + backward through the public API only, inputs generated on the CPU):
  * every call into libdwcgan_hip.so, through a proxy in front of what ``_lib.load()`` returns: the entry name, the arguments its
    ``_lib.SIGNATURES`` row declares as ``c_int``, and for pointer arguments only whether they were null.  ``size_t`` arguments are
    left out (arena sizes follow the workspace's growth history).
      - ``L`` lines: entries that take a pointer (they launch, or write device memory), in call order;
      - ``Q`` lines: entries that take none (``*_ok``, ``*_ws_bytes``, ``*_elems``: host-side questions with no side effect), SORTED
        within the case -- the nodes ask for an arena size and for a prepared weight layout in whichever order their text happens to
        have them, and that order is nothing a caller or a kernel can see;
  * every KernelTimer span: tag, flops, executed flops, detail (``S`` lines);
  * the SHA-256 of the bytes of y, dx, dw, db (``H`` lines; ``-`` where the case has no such tensor).

The comparison is equality as text, after one rewrite: ``dwc_bf16_conv2d_same_halo(x, w, b, y, ...)`` on one side reads as
``dwc_bf16_conv2d_same_halo_add(x, w, b, null, y, ...)`` (the C function IS that call).

The table is kept honest by ENTRIES: every ``lib.dwc_*`` / ``_fn(lib, ...)`` name the three nodes and their helpers can call.  The run
fails if one of them was never called and is not listed in UNREACHABLE with its reason.
"""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "dwc-gan_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# every C entry named between ops._x3_use and ops.conv2d_zeropad (both precisions' forms of the _fn() names, both pad rules' forms of
# the "+ z" names), sorted
ENTRIES = """
dwc_act_bwd_bias dwc_act_bwd_bias_amax dwc_act_bwd_bias_ws_bytes dwc_bf16_act_bwd_bias dwc_bf16_conv2d_bwd_data dwc_bf16_conv2d_bwd_data_crop
dwc_bf16_conv2d_bwd_data_crop_ws_bytes dwc_bf16_conv2d_bwd_data_fold dwc_bf16_conv2d_bwd_data_image dwc_bf16_conv2d_bwd_data_image_narrow
dwc_bf16_conv2d_bwd_data_image_ws_bytes dwc_bf16_conv2d_bwd_data_ring dwc_bf16_conv2d_bwd_data_s2_ring dwc_bf16_conv2d_bwd_data_same
dwc_bf16_conv2d_bwd_data_same_fused dwc_bf16_conv2d_bwd_data_same_fused_ok dwc_bf16_conv2d_bwd_data_same_ws_bytes dwc_bf16_conv2d_bwd_data_ws_bytes
dwc_bf16_conv2d_bwd_data_zeropad dwc_bf16_conv2d_bwd_data_zeropad_ws_bytes dwc_bf16_conv2d_bwd_weight dwc_bf16_conv2d_bwd_weight_ex
dwc_bf16_conv2d_bwd_weight_ex_ws_bytes dwc_bf16_conv2d_bwd_weight_ws_bytes dwc_bf16_conv2d_bwd_weight_zeropad dwc_bf16_conv2d_fwd
dwc_bf16_conv2d_fwd_ex dwc_bf16_conv2d_fwd_ws_bytes dwc_bf16_conv2d_fwd_zeropad dwc_bf16_conv2d_narrow dwc_bf16_conv2d_narrow_ok
dwc_bf16_conv2d_s2_halo dwc_bf16_conv2d_s2_halo_bwd_data dwc_bf16_conv2d_s2_halo_bwd_data_fused dwc_bf16_conv2d_s2_halo_bwd_data_ok
dwc_bf16_conv2d_s2_halo_ok dwc_bf16_conv2d_s2_halo_zeropad dwc_bf16_conv2d_same_halo dwc_bf16_conv2d_same_halo_add dwc_bf16_conv2d_same_halo_ok
dwc_bf16_conv2d_stem dwc_bf16_conv2d_stem_crop dwc_bf16_conv2d_stem_ok dwc_bf16_conv2d_wgrad_halo dwc_bf16_conv2d_wgrad_halo_ws_bytes
dwc_bf16_conv2d_wgrad_halo_zeropad dwc_bf16_conv7_smallk_wgrad dwc_bf16_conv7_smallk_wgrad_ws_bytes dwc_bf16_reflect_pad_adjoint
dwc_bf16_reflect_pad_adjoint_band dwc_conv2d_bwd_data dwc_conv2d_bwd_data_crop dwc_conv2d_bwd_data_crop_ws_bytes dwc_conv2d_bwd_data_fold
dwc_conv2d_bwd_data_image dwc_conv2d_bwd_data_image_ws_bytes dwc_conv2d_bwd_data_ring dwc_conv2d_bwd_data_s2_ring dwc_conv2d_bwd_data_same
dwc_conv2d_bwd_data_same_ws_bytes dwc_conv2d_bwd_data_ws_bytes dwc_conv2d_bwd_data_zeropad dwc_conv2d_bwd_data_zeropad_ws_bytes dwc_conv2d_bwd_weight
dwc_conv2d_bwd_weight_ex dwc_conv2d_bwd_weight_ex_ws_bytes dwc_conv2d_bwd_weight_ws_bytes dwc_conv2d_bwd_weight_zeropad dwc_conv2d_fwd
dwc_conv2d_fwd_ex dwc_conv2d_fwd_ws_bytes dwc_conv2d_fwd_zeropad dwc_h2_conv2d_bwd_data_same_fused dwc_h2_conv2d_s2_bwd_data
dwc_h2_conv2d_s2_bwd_data_fused dwc_h2_conv2d_s2_ws dwc_h2_conv2d_s2_ws_zeropad dwc_h2_conv2d_same_add_ws dwc_h2_conv2d_wgrad
dwc_h2_conv2d_wgrad_zeropad dwc_reflect_pad_adjoint dwc_reflect_pad_adjoint_band dwc_reflect_pad_adjoint_pitch dwc_x3_conv2d_ksplit_ticket_words
dwc_x3_conv2d_ksplit_ws_bytes dwc_x3_conv2d_narrow dwc_x3_conv2d_narrow_ok dwc_x3_conv2d_s2_bwd_data dwc_x3_conv2d_s2_bwd_data_ok dwc_x3_conv2d_s2_ok
dwc_x3_conv2d_s2_ws dwc_x3_conv2d_s2_ws_zeropad dwc_x3_conv2d_same_add_ws dwc_x3_conv2d_same_ok dwc_x3_conv2d_stem_amax dwc_x3_conv2d_stem_crop
dwc_x3_conv2d_stem_ok dwc_x3_conv2d_wgrad dwc_x3_conv2d_wgrad_ws_bytes dwc_x3_conv2d_wgrad_zeropad dwc_x3_conv7_smallk_wgrad
dwc_x3_conv7_smallk_wgrad_ws_bytes
""".split()

# entries of ENTRIES no case can reach, with the reason.  (The other branch nothing here reaches -- an fp32 operand of 2 GiB or more
# with X3_PLANES = 2, which h2_fits sends to the three-plane launches -- names no entry of its own: X3_PLANES = 3 calls the same ones.)
UNREACHABLE = {
    "dwc_bf16_conv2d_same_halo": "after the refactor every bf16 halo launch goes through dwc_bf16_conv2d_same_halo_add (it is that "
                                 "call with add = null); the parent calls it, the comparison rewrites it",
}

SWITCH_SETS = [{}, {"X3_PLANES": 3}, {"RING_FUSED": 0}, {"DGRAD_FOLD": 0}, {"NARROW": 0}, {"HALO": 0}, {"HALO": 0, "RING_FUSED": 0}]
P = "P"      # "as many channels as an image buffer has planes" (4 fp32, 8 bf16), filter over 3 of them

# (api, B, Cin, Cout, H, W, K, stride, pad, act, extra switches, "full": the whole product below / "lean": default switches only)
SHAPES = [
    # stride-1 halo routes (tests/test_zero_pad.py HALO_S1_CASES; the last: contraction split), 48x48: the fused fp32 ring
    ("conv2d", 2, 64, 64, 16, 16, 3, 1, 1, "relu", {}, "full"),
    ("conv2d", 1, 64, 64, 32, 32, 3, 1, 1, "none", {}, "full"),
    ("conv2d", 1, 64, 64, 16, 16, 5, 1, 2, "lrelu", {}, "full"),
    ("conv2d", 1, 64, 64, 48, 48, 3, 1, 1, "relu", {}, "full"),
    ("conv2d", 2, 256, 256, 16, 16, 3, 1, 1, "none", {}, "full"),
    ("conv2d", 2, 64, 128, 32, 32, 3, 1, 1, "relu", {}, "full"),
    # the bf16 fused-ring gate: K = 3, Cin a multiple of 128 above 128, at least 512 workgroups
    ("conv2d", 2, 256, 256, 128, 128, 3, 1, 1, "none", {}, "lean"),
    # stride-2 routes (tests/test_zero_pad.py test_stride2_routes_under_zero) with the size rule of the data gradient lifted
    ("conv2d", 1, 64, 64, 32, 32, 4, 2, 1, "none", {"S2DGRAD_MIN_WGS": 0}, "full"),
    ("conv2d", 2, 64, 128, 64, 32, 4, 2, 1, "relu", {"S2DGRAD_MIN_WGS": 0}, "full"),
    ("conv2d", 1, 64, 64, 64, 64, 4, 2, 1, "none", {"S2DGRAD_MIN_WGS": 0}, "lean"),
    ("conv2d", 1, 64, 64, 96, 96, 4, 2, 1, "none", {"S2DGRAD_MIN_WGS": 0}, "lean"),
    ("conv2d", 2, 64, 128, 32, 32, 4, 2, 1, "relu", {}, "lean"),              # (under the size rule: the im2col data gradient)
    # the stride-2 forward's 160-workgroup gate (tests/test_amax_contract.py H2_S2)
    ("conv2d", 10, 16, 256, 64, 64, 4, 2, 1, "lrelu", {}, "lean"),
    ("conv2d", 40, 64, 256, 32, 32, 4, 2, 1, "none", {}, "lean"),
    ("conv2d", 40, 64, 256, 32, 32, 4, 2, 1, "none", {"X3_PLANES": 3, "S2DGRAD_MIN_WGS": 0}, "lean"),
    # 7x7 stem on an image buffer
    ("conv2d", 2, P, 64, 16, 16, 7, 1, 3, "relu", {}, "full"),
    ("conv2d", 1, P, 64, 20, 36, 7, 1, 3, "none", {}, "full"),
    # im2col routes: stride 2 on a small grid, fewer than 32 output channels, 1x1 without padding, a grid too small to fold, a padded
    # output buffer, fp32 channels the split products do not take
    ("conv2d", 1, 16, 32, 6, 6, 4, 2, 1, "tanh", {}, "full"),
    ("conv2d", 2, 32, 16, 12, 12, 3, 1, 1, "lrelu", {}, "full"),
    ("conv2d", 2, 32, 64, 8, 8, 1, 1, 0, "none", {}, "full"),
    ("conv2d", 1, 64, 64, 3, 3, 3, 1, 1, "relu", {}, "full"),
    ("conv2d_padded", 1, 16, 3, 8, 8, 3, 1, 1, "tanh", {}, "full"),
    ("conv2d", 1, 8, 32, 8, 8, 3, 1, 1, "relu", {}, "full"),
    ("conv2d", 1, P, 32, 16, 16, 5, 1, 2, "lrelu", {}, "full"),               # (an image's data gradient the narrow kernels leave)
    # image heads: width divisible by 32 // P and not, 64 channels (the narrow kernels) and not
    ("conv2d_heads", 1, 64, P, 16, 16, 7, 1, 3, "heads", {}, "full"),
    ("conv2d_heads", 2, 64, P, 20, 32, 7, 1, 3, "heads", {}, "full"),
    ("conv2d_heads", 1, 64, P, 16, 18, 7, 1, 3, "heads", {}, "full"),
    ("conv2d_heads", 1, 32, P, 16, 16, 7, 1, 3, "heads", {}, "full"),
    # VGG (frozen weights): first layer (image planes to 64, im2col), 64 to 64, contraction split, a larger grid, 5x5 without relu
    ("conv2d_zeropad", 1, P, 64, 16, 16, 3, 1, 1, "relu", {}, "full"),
    ("conv2d_zeropad", 1, 64, 64, 16, 16, 3, 1, 1, "relu", {}, "full"),
    ("conv2d_zeropad", 2, 256, 256, 16, 16, 3, 1, 1, "relu", {}, "full"),
    ("conv2d_zeropad", 1, 64, 64, 48, 48, 3, 1, 1, "none", {}, "full"),
    ("conv2d_zeropad", 1, 64, 64, 16, 16, 5, 1, 2, "none", {}, "full"),
]


def cases():
    """(name, api, prec, geometry, pad_mode, token, bias, bias_grad, frozen, switches) of every case, in a fixed order."""
    for api, B, ci, co, H, W, K, stride, pad, act, extra, breadth in SHAPES:
        geom = (B, ci, co, H, W, K, stride, pad, act)
        for prec, zero in itertools.product(("fp32", "bf16"), (False, True)):
            if api == "conv2d_zeropad" and not zero:
                continue
            variants = []     # (token, bias, bias_grad, frozen)
            if api == "conv2d":
                variants = [(t, True, g, False) for t in (False, True) for g in (True, False)] + [(False, False, True, False),
                                                                                                 (True, True, True, True)]
            elif api == "conv2d_zeropad":
                variants = [(False, True, True, True), (False, False, True, True)]
            else:
                variants = [(False, True, True, False), (False, True, True, True)]
            for sw in (SWITCH_SETS if breadth == "full" else [{}]):
                sw = dict(sw, **extra)
                for token, bias, bias_grad, frozen in variants:
                    name = "%s %s %s B%d %s>%s %dx%d k%d s%d p%d %s%s%s%s%s %s" % (
                        api, prec, "zero" if zero else "reflect", B, ci, co, H, W, K, stride, pad, act, " token" if token else "",
                        "" if bias else " nobias", "" if bias_grad else " nobiasgrad", " frozen" if frozen else "",
                        ",".join("%s=%d" % kv for kv in sorted(sw.items())) or "default")
                    yield name, api, prec, geom, zero, token, bias, bias_grad, frozen, sw


class Recorder:
    """Stands in front of the loaded library: attribute access hands out the real entry wrapped in a logging call."""

    def __init__(self, lib, signatures):
        self._lib, self._sig, self._wrapped = lib, signatures, {}
        self.launches, self.queries, self.seen = [], [], set()

    def __getattr__(self, name):
        fn = self._wrapped.get(name)
        if fn is None:
            fn = self._wrap(name, getattr(self._lib, name))
            self._wrapped[name] = fn
        return fn

    def _wrap(self, name, real):
        argtypes = self._sig[name][1] if name in self._sig else None
        if argtypes is None:
            return real
        kinds = ["i" if t is ctypes.c_int else "p" if t is ctypes.c_void_p else "" for t in argtypes]
        sink = self.launches if "p" in kinds else self.queries

        def call(*args):
            words = [name]
            for k, a in zip(kinds, args):
                if k == "i":
                    words.append(str(int(a)))
                elif k == "p":
                    words.append("null" if a is None or a == 0 else "ptr")
            sink.append(" ".join(words))
            self.seen.add(name)
            return real(*args)
        return call

    def drain(self):
        out = ["L " + s for s in self.launches] + ["Q " + s for s in sorted(self.queries)]
        del self.launches[:], self.queries[:]
        return out


def _sha(t):
    if t is None:
        return "-"
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def record(out_path):
    import torch
    from hipdwc import _lib, ops
    real = _lib.load()
    rec = Recorder(real, _lib.SIGNATURES)
    _lib._lib = rec                          # what _lib.load() returns from here on
    assert _lib.load() is rec
    timer = ops.KernelTimer()
    ops.TIMER = timer
    dev = torch.device("cuda:0")
    lines, n_cases, refused = [], 0, []
    for name, api, prec, geom, zero, token, bias, bias_grad, frozen, sw in cases():
        B, ci, co, H, W, K, stride, pad, act = geom
        saved = {k: getattr(ops, k) for k in sw}
        for k, v in sw.items():
            setattr(ops, k, v)
        ops.set_precision(prec)
        try:
            dt = ops.act_dtype()
            planes = ops.image_planes(dt)
            cx, wci = (planes, 3) if ci == P else (ci, ci)
            cw = planes if co == P else co
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            x = torch.randn(B, cx, H, W, generator=g)
            w = torch.randn(cw, wci, K, K, generator=g) * (1.0 / (wci * K * K) ** 0.5)
            b = torch.randn(cw, generator=g) if bias else None
            if co == P:
                w[4:] = 0.0                  # (bf16 heads: planes 4..7 are zero planes)
                b[4:] = 0.0
            res = torch.randn(B, cx, H, W, generator=g) if token else None
            xd = x.to(dev).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            as_param = prec == "bf16" and not frozen          # (a Parameter bias takes the zero-gradient flag, a plain tensor the zeros)
            wd = w.to(dev)
            bd = b.to(dev) if bias else None
            if as_param:
                wd = torch.nn.Parameter(wd)
                bd = torch.nn.Parameter(bd) if bias else None
            elif not frozen:
                wd.requires_grad_(True)
                if bias:
                    bd.requires_grad_(True)
            tok = ops.ResGradToken() if token else None
            mode = "zero" if zero else "reflect"
            if api == "conv2d":
                y = ops.conv2d(xd, wd, bd, stride, pad, act, bias_grad=bias_grad, token=tok, pad_mode=mode)
            elif api == "conv2d_padded":
                y = ops.conv2d_padded(xd, wd, bd, stride, pad, act, pad_mode=mode)
            elif api == "conv2d_heads":
                y = ops.conv2d_heads(xd, wd, bd, pad_mode=mode)
            else:
                y = ops.conv2d_zeropad(xd, wd, bd, pad, act)
            gy = torch.randn(y.shape, generator=g).to(dev).to(y.dtype)
            if token:
                tok.g = res.to(dev).to(dt)
            y.backward(gy)
            torch.cuda.synchronize()
            hashes = "H y %s dx %s dw %s db %s" % (_sha(y), _sha(xd.grad), _sha(wd.grad), _sha(bd.grad if bias else None))
        except _lib.HipKernelError as e:
            # an entry point refused its arguments (a host-side answer, nothing was launched): part of the record like any other result
            hashes = "E %s" % e
            refused.append(name)
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
        lines.append("CASE " + name)
        lines += rec.drain()
        for (tag, flops, _a, _b), ex, det in zip(timer.spans, timer.executed, timer.details):
            lines.append("S %s %r %r %s" % (tag, float(flops), float(ex), det))
        del timer.spans[:], timer.executed[:], timer.details[:]
        lines.append(hashes)
        n_cases += 1
    ops.TIMER = None
    ops.set_precision("fp32")
    missing = sorted(set(ENTRIES) - rec.seen - set(UNREACHABLE))
    lines.append("ENTRIES %d called %d unreachable %d never called %d" % (
        len(ENTRIES), len(set(ENTRIES) & rec.seen), len(set(UNREACHABLE) - rec.seen), len(missing)))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d cases, %d lines -> %s" % (n_cases, len(lines), out_path))
    for name in refused:
        print("refused: " + name)
    if missing:
        print("never called: " + " ".join(missing))
        return 1
    return 0


def _normalised(path):
    out = []
    for line in open(path):
        words = line.split()
        if len(words) > 1 and words[0] == "L" and words[1] == "dwc_bf16_conv2d_same_halo":
            words = words[:1] + ["dwc_bf16_conv2d_same_halo_add"] + words[2:5] + ["null"] + words[5:]
            line = " ".join(words) + "\n"
        if words and words[0] == "ENTRIES":
            continue          # (the parent calls the alias itself: its tally differs by that one name)
        out.append(line)
    return out


def compare(a_path, b_path):
    a, b = _normalised(a_path), _normalised(b_path)
    count = lambda ls, c: sum(1 for s in ls if s.startswith(c + " "))
    print("cases %d / %d, calls %d / %d, spans %d / %d, hash lines %d / %d" % (
        count(a, "CASE"), count(b, "CASE"), count(a, "L") + count(a, "Q"), count(b, "L") + count(b, "Q"), count(a, "S"), count(b, "S"),
        count(a, "H"), count(b, "H")))
    diffs = [(i, s, t) for i, (s, t) in enumerate(zip(a, b)) if s != t]
    if len(a) != len(b) or diffs:
        print("DIFFERENT: %d / %d lines, %d differing" % (len(a), len(b), len(diffs)))
        case = ""
        shown = 0
        for i, s in enumerate(a[:len(b)]):
            if s.startswith("CASE "):
                case = s
            if s != b[i] and shown < 20:
                print("  in %s  - %s  + %s" % (case, s, b[i]), end="")
                shown += 1
        return 1
    print("EQUAL")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="run the table and write the trace here")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two traces")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out FILE or --compare BEFORE AFTER")
    sys.exit(record(args.out))
