"""Synchronised batch norm (hipdwc.syncbn; ``batch_norm(..., sync=)``, ``Solver.enable_data_parallel(sync_bn=True)``).

CPU: the new C-ABI symbols agree between header, ctypes table and library and none contains ``batchnorm``; dwc_syncbn_finalise
refuses bad arguments before any launch; the stock-op form on R = 2, 3 virtual ranks (threads that meet in a barrier) in float64
against nn.BatchNorm2d on the concatenated batch.  GPU: R virtual ranks on the one device, WITHOUT threads (autograd runs every
backward node on the one device thread, a barrier inside a gather would deadlock): the other ranks' contributions are computed first
with the public phase helpers and each rank gets a ``sync`` whose all_gather returns "mine at ``rank``, theirs precomputed".  The
reference is float64 on the concatenated batch (test_batch_norm._case on the global shape), at the tolerances test_bn_kernels_vs_float64
holds the plain kernels to.  Shapes are (R; S, Bs, C, H): R ranks with Bs samples of each of the S segments."""
import ctypes
import os
import re
import threading
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as ga
from hipdwc import _lib, batchnorm, host, ops, syncbn
from test_batch_norm import ACTS, BF, DEV, TOL, _assert_tag, _buffers, _case, _dev, _running64, close

SYNC_SYMBOLS = {"dwc_syncbn_ws_bytes", "dwc_syncbn_moments", "dwc_bf16_syncbn_moments", "dwc_syncbn_finalise", "dwc_syncbn_apply",
                "dwc_syncbn_apply_amax", "dwc_bf16_syncbn_apply", "dwc_syncbn_bwd_sums", "dwc_bf16_syncbn_bwd_sums",
                "dwc_syncbn_bwd_apply", "dwc_syncbn_bwd_apply_amax", "dwc_bf16_syncbn_bwd_apply"}


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_syncbn_symbols_header_table_library():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "dwcgan_hip.h")).read()
    declared = {n for n in re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header) if "syncbn" in n}
    assert declared == SYNC_SYMBOLS
    assert {n for n in _lib.SIGNATURES if "syncbn" in n} == SYNC_SYMBOLS
    assert not any("batchnorm" in n for n in SYNC_SYMBOLS)
    assert int(re.search(r"#define\s+DWC_ABI_VERSION\s+(\d+)\b", header).group(1)) == _lib.ABI_VERSION == 11      # additive
    lib = _lib.load()
    for n in SYNC_SYMBOLS:
        assert hasattr(lib, n), n
        # the argument list of the header and of the ctypes table have the same length
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n
    assert lib.dwc_syncbn_ws_bytes(3, 3, 64, 16) == lib.dwc_batchnorm_ws_bytes(3, 3, 64, 16)
    assert lib.dwc_syncbn_ws_bytes(2, 1, 1, 8) >= (2 * 2 * 8) * 4          # one value per (sample, channel) is a legal local part


def test_syncbn_finalise_refuses_bad_arguments_before_any_launch():
    """No device is touched: the pointers are dummies and every call must return DWC_EINVAL from the host-side checks."""
    lib = _lib.load()
    p = 4096

    def fin(R=2, S=2, C=8, order=(0, 1), n=None, rm=p, rv=p, m=p):
        o = _lib.BnOrder(len(order) if n is None else n, (ctypes.c_int * 8)(*(list(order) + [0] * 8)[:8]))
        return lib.dwc_syncbn_finalise(m, R, p, p, rm, rv, S, C, 1e-5, 0.1, o, None)
    assert fin(R=0) == fin(R=-1) == _lib.EINVAL
    assert fin(order=(0, 2)) == fin(order=(-1,)) == fin(n=9) == fin(n=-1) == _lib.EINVAL
    assert fin(S=0) == fin(S=9) == fin(C=0) == fin(m=None) == _lib.EINVAL
    assert fin(rm=None) == fin(rv=None) == _lib.EINVAL                    # the buffers come together


class BarrierSync:
    """R threads of one process as ranks: all_gather meets in a barrier.  (CPU only.)"""

    def __init__(self, world, rank, shared):
        self.world, self.rank, self.force, self.shared = world, rank, False, shared

    def all_gather(self, t):
        slots, barrier = self.shared
        slots[self.rank] = t.detach().clone()
        barrier.wait()
        out = torch.stack(list(slots))
        barrier.wait()
        return out


def _split(t, S, parts):
    """The ranks' local tensors of a global batch of S segments: rank r holds parts[r] samples of every segment."""
    ts = t.reshape(S, sum(parts), *t.shape[1:])
    out, o = [], 0
    for n in parts:
        out.append(ts[:, o:o + n].reshape(S * n, *t.shape[1:]))
        o += n
    return out


def _join(locs, S, parts):
    return torch.cat([l.reshape(S, n, *l.shape[1:]) for l, n in zip(locs, parts)], 1).reshape(S * sum(parts), *locs[0].shape[1:])


@pytest.mark.parametrize("R", [2, 3])
def test_syncbn_stock_op_form_on_cpu_vs_concatenated_batch(monkeypatch, R):
    """The stock-op form, float64, R virtual ranks, three segments with order (0, 2, 1, 2): every rank's y / dx are its slice of four
    calls of nn.BatchNorm2d on the concatenated segments x0, x2, x1, x2; dgamma (summed over the ranks) and dbeta likewise; the
    running buffers of every rank are the module's.  Tolerances of test_bn_stock_op_path_on_cpu_vs_single_calls."""
    import networks.networks as nets
    monkeypatch.setattr(batchnorm, "BN_HIP", 0)
    g = torch.Generator().manual_seed(11 + R)
    C, Bs, S = 6, 2, 3
    parts = [Bs] * R
    xs = [(torch.randn(R * Bs, C, 5, 4, generator=g, dtype=torch.float64) * (1 + j) + j +
           5.0 * torch.arange(R * Bs, dtype=torch.float64)[:, None, None, None]).requires_grad_(True) for j in range(S)]
    gys = [torch.randn(R * Bs, C, 5, 4, generator=g, dtype=torch.float64) for _ in range(S)]
    ref = torch.nn.BatchNorm2d(C).double()
    mods = [nets.SegmentedBatchNorm2d(C).double() for _ in range(R)]
    with torch.no_grad():
        for m in [ref] + mods:
            m.weight.copy_(torch.linspace(-1.0, 1.5, C))
            m.bias.copy_(torch.linspace(0.3, -0.2, C))
    want = {}
    for j in (0, 2, 1, 2):
        want[j] = F.leaky_relu(ref(xs[j]), 0.1)
    sum((want[j] * gys[j]).sum() for j in range(S)).backward()
    x_loc = [t.detach().clone().requires_grad_(True) for t in _split(torch.cat([x.detach() for x in xs]), S, parts)]
    gy_loc = _split(torch.cat(gys), S, parts)
    shared = ([None] * R, threading.Barrier(R))
    ys, errs = [None] * R, []

    def rank(r):
        try:
            mods[r].sync = BarrierSync(R, r, shared)
            ys[r] = mods[r](x_loc[r], act="lrelu", segments=S, stat_order=(0, 2, 1, 2))
            (ys[r] * gy_loc[r]).sum().backward()
        except Exception as e:      # a dead rank must not leave the others in the barrier
            errs.append(e)
            shared[1].abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(R)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not errs, errs
    close(_join(ys, S, parts), torch.cat([want[j] for j in range(S)]), rel=1e-12, atol=1e-12, msg="y")
    close(_join([x.grad for x in x_loc], S, parts), torch.cat([x.grad for x in xs]), rel=1e-10, atol=1e-12, msg="dx")
    close(sum(m.weight.grad for m in mods), ref.weight.grad, rel=1e-10, atol=1e-12, msg="dgamma")
    close(sum(m.bias.grad for m in mods), ref.bias.grad, rel=1e-10, atol=1e-12, msg="dbeta")
    for m in mods:
        close(m.running_mean, ref.running_mean, rel=1e-12, atol=1e-14, msg="running_mean")
        close(m.running_var, ref.running_var, rel=1e-12, atol=1e-14, msg="running_var")
        assert torch.equal(m.running_mean, mods[0].running_mean) and torch.equal(m.running_var, mods[0].running_var)
        assert int(m.num_batches_tracked) == int(ref.num_batches_tracked) == 4
    # eval mode exchanges nothing (a gather would wait for the other ranks for ever); one rank without force is the plain path
    mods[0].eval()
    ref.eval()
    close(mods[0](x_loc[0].detach(), act="relu"), torch.relu(ref(x_loc[0].detach())), rel=1e-12, atol=1e-12, msg="eval y")
    mods[0].train()
    mods[0].sync = BarrierSync(1, 0, None)
    mods[0](x_loc[0].detach(), segments=S)


def test_syncbn_count_is_checked_over_all_ranks(monkeypatch):
    monkeypatch.setattr(batchnorm, "BN_HIP", 0)
    x, w, b = torch.randn(1, 4, 1, 1, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)

    class One:
        world, rank, force = 1, 0, True

        def all_gather(self, t):
            return t[None].clone()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        batchnorm.batch_norm(x, w, b, None, None, sync=One())              # one value in the whole "global" batch
    two = One()
    two.segment_batch = 2                                                  # another rank holds the second value
    with pytest.raises(ValueError, match="all_gather returned"):           # ... and this gather does not deliver it
        two.world = 2
        batchnorm.batch_norm(x, w, b, None, None, sync=two)


def test_group_sync_is_shared_by_deepcopy():
    import copy

    class Stub(syncbn.GroupSync):
        def __init__(self):
            self.group, self.world, self.rank, self.force = object(), 2, 0, False
    import networks.networks as nets
    m = nets.SegmentedBatchNorm2d(4)
    assert m.sync is None and "sync" not in m.state_dict()
    m.sync = Stub()
    c = copy.deepcopy(m)
    assert c.sync is m.sync and c.weight is not m.weight


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: virtual ranks on one device
# ---------------------------------------------------------------------------------------------------------------------------------
class QueueSync:
    """The ``sync`` of one virtual rank: the k-th all_gather returns the k-th precomputed [R, ...] array with this rank's own
    contribution at ``rank`` (first call: the forward's moments, second: the backward's sums)."""

    def __init__(self, world, rank, segment_batch=None, alloc=None):
        self.world, self.rank, self.force, self.segment_batch, self.alloc = world, rank, True, segment_batch, alloc
        self.queue, self.seen = [], []

    def all_gather(self, t):
        out = self.queue.pop(0).clone() if self.queue else t[None].clone()
        assert out.shape[0] == self.world and out.shape[1:] == t.shape
        self.seen.append(t)
        out[self.rank] = t
        return self.alloc.guarded_input(out, channels_last=False) if self.alloc is not None else out


def _virtual_ranks(S, parts, act, x, ga_, be, gy, half, order=None, alloc=None):
    """Forward and backward of every virtual rank.  -> per rank (y, dx, dgamma, dbeta, running_mean, running_var, mean, rstd)."""
    R, C = len(parts), x.shape[1]
    order = tuple(range(S)) if order is None else order
    put = (lambda t: alloc.guarded_input(t.to(BF) if half and t.dim() == 4 else t, device=DEV)) if alloc else (lambda t: _dev(t, half))
    xs = [put(t).requires_grad_(True) for t in _split(x, S, parts)]
    gys = [put(t) for t in _split(gy, S, parts)]
    moments = torch.stack([syncbn.sync_moments(t.detach(), S) for t in xs])
    mean, rstd = syncbn.sync_finalise(moments, None, None, (), 0.1, 1e-5)
    sums = torch.stack([syncbn.sync_bwd_sums(g_, t.detach(), mean, rstd, ga_.to(DEV), be.to(DEV), S, act)[0] for g_, t in zip(gys, xs)])
    if alloc:
        alloc.verify()
    out = []
    for r in range(R):
        sync = QueueSync(R, r, sum(parts), alloc)
        sync.queue = [moments, sums]
        gd, bd = put(ga_).requires_grad_(True), put(be).requires_grad_(True)
        rm, rv = put(torch.zeros(C)), put(torch.ones(C))
        y = batchnorm.batch_norm(xs[r], gd, bd, rm, rv, segments=S, order=order, act=act, sync=sync)
        assert y.dtype == (BF if half else torch.float32) and y.is_contiguous(memory_format=torch.channels_last)
        assert type(y.grad_fn).__name__.startswith("_SyncBatchNorm") and not type(y.grad_fn).__name__.startswith("_SyncBatchNormTorch")
        mu, rs = y.grad_fn.saved_tensors[1:3]
        if alloc:
            alloc.verify()
            y.backward(gys[r])
            alloc.verify()
        else:
            (y.float() * gys[r].float()).sum().backward()
        assert not sync.queue and len(sync.seen) == 2
        assert torch.equal(sync.seen[0], moments[r]) and torch.equal(sync.seen[1], sums[r])      # the helpers ARE the phases
        out.append((y.detach(), xs[r].grad, gd.grad, bd.grad, rm, rv, mu, rs))
    return out


def _check_vs_float64(R_parts, shape, act, offsets, half, alloc=None):
    S, _, C, H = shape
    parts = list(R_parts)
    x, ga_, be, gy, yr, dxr, dgr, dbr = _case((S, sum(parts), C, H), act, offsets, half)
    a = _virtual_ranks(S, parts, act, x, ga_, be, gy, half, alloc=alloc)
    ty, tdx, tp = TOL[half]
    close(_join([o[0] for o in a], S, parts), yr, ty, msg="y")
    close(_join([o[1] for o in a], S, parts), dxr, tdx, msg="dx")
    close(sum(o[2].double() for o in a), dgr, tp, msg="dgamma")
    close(sum(o[3].double() for o in a), dbr, tp, msg="dbeta")
    wm, wv = _running64(x, S, range(S), torch.zeros(C), torch.ones(C))
    for o in a:
        close(o[4], wm, 1e-5, atol=0, msg="running_mean")
        close(o[5], wv, 1e-5, atol=0, msg="running_var")
        for k, name in ((4, "running_mean"), (5, "running_var"), (6, "mean"), (7, "rstd")):
            assert torch.equal(o[k], a[0][k]), name + " differs between the ranks"
    return a, (x, ga_, be, gy)


# (R; S, Bs, C, H)
RANK_SHAPES = [
    (2, (1, 1, 8, 1)),          # local count 1, global 2: M2 / (cnt - 1)
    (2, (1, 1, 8, 2)),          # smallest ordinary case
    (3, (3, 2, 16, 2)),         # odd R, HW < row groups
    (2, (4, 1, 64, 16)),        # 4 chunks
    (4, (3, 1, 128, 9)),        # ragged chunk
    (2, (2, 1, 1024, 3)),       # one row group
    (2, (1, 2, 24, 6)),         # idle row groups
    (8, (1, 1, 8, 2)),          # a node's rank count
]


def _rid(v):
    return "R%d-%s" % (v[0], "x".join(str(n) for n in v[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets", [False, True], ids=["plain", "offsets"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", RANK_SHAPES, ids=_rid)
def test_syncbn_virtual_ranks_vs_float64(case, act, offsets, half):
    R, shape = case
    S = shape[0]
    parts = [shape[1]] * R
    a, (x, ga_, be, gy) = _check_vs_float64(parts, shape, act, offsets, half)
    b = _virtual_ranks(S, parts, act, x, ga_, be, gy, half)
    for u, v in zip(a, b):
        for s, t, name in zip(u, v, ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "mean", "rstd")):
            assert torch.equal(s, t), name + ": the second run differs"


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("offsets", [False, True], ids=["plain", "offsets"])
@pytest.mark.parametrize("act", ACTS)
def test_syncbn_unequal_rank_counts(act, offsets, half):
    """Two ranks with 1 and 2 samples of each segment: legal for the kernels (the merge weighs by the counts)."""
    _check_vs_float64([1, 2], (2, None, 16, 3), act, offsets, half)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_syncbn_running_statistics_in_order(half):
    """Order (0, 2, 1, 2) from non-trivial buffers on 3 ranks (test_bn_running_statistics_in_order's check, statistics over ranks)."""
    S, parts, C, H = 3, [2, 2, 2], 16, 2
    x, ga_, be, gy = _case((S, 6, C, H), "lrelu", True, half)[:4]
    g = torch.Generator().manual_seed(3)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    order = (0, 2, 1, 2)
    xs = _split(x, S, parts)
    moments = torch.stack([syncbn.sync_moments(_dev(t, half), S) for t in xs])
    wm, wv = _running64(x, S, order, rm0, rv0)
    got = []
    for r in range(3):
        sync = QueueSync(3, r)
        sync.queue = [moments]
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        v0 = rm._version
        batchnorm.batch_norm(_dev(xs[r], half), ga_.to(DEV), be.to(DEV), rm, rv, segments=S, order=order, act="lrelu", sync=sync)
        assert rm._version > v0 and rv._version > 0
        close(rm, wm, 1e-5, atol=0, msg="running_mean")
        close(rv, wv, 1e-5, atol=0, msg="running_var")
        got.append((rm, rv))
    assert all(torch.equal(got[0][0], m) and torch.equal(got[0][1], v) for m, v in got)


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2, 128, 9), (2, 5, 256, 32)], ids=lambda s: "x".join(str(v) for v in s))
def test_syncbn_one_rank_is_bit_equal_to_the_plain_path(shape, half):
    """R = 1: moments -> finalise -> apply and sums -> apply reproduce the plain three-launch chains bit for bit."""
    S, Bs, C, H = shape
    x, ga_, be, gy = _case(shape, "relu", False, half)[:4]
    res = []
    for sync in (None, QueueSync(1, 0)):
        xd, gd, bd = _dev(x, half, True), _dev(ga_, grad=True), _dev(be, grad=True)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y = batchnorm.batch_norm(xd, gd, bd, rm, rv, segments=S, order=(0, 1, 0), act="relu", sync=sync)
        assert type(y.grad_fn).__name__.startswith("_SyncBatchNorm" if sync else "_BatchNorm")
        (y.float() * gy.to(DEV)).sum().backward()
        res.append((y.detach(), xd.grad, gd.grad, bd.grad, rm, rv))
    for u, v, name in zip(res[0], res[1], ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var")):
        assert torch.equal(u, v), name
    # without force a one-rank sync IS the plain path
    lazy = QueueSync(1, 0)
    lazy.force = False
    y = batchnorm.batch_norm(_dev(x, half, True), ga_.to(DEV), be.to(DEV), None, None, segments=S, act="relu", sync=lazy)
    assert type(y.grad_fn).__name__.startswith("_BatchNorm") and not lazy.seen


@pytest.fixture
def guards(monkeypatch):
    """tests/guarded_alloc.py applied to hipdwc.syncbn: scratch of exactly the size asked for, every output, statistics array and
    gathered array between guards and poisoned."""
    alloc = ga.GuardedAllocator()
    monkeypatch.setattr(ops, "workspace", alloc.workspace)
    monkeypatch.setattr(ops, "empty_cl", alloc.empty_cl)
    monkeypatch.setattr(syncbn, "torch", ga.TorchProxy(alloc))
    yield alloc
    alloc.forget()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(2, (1, 1, 8, 1)), (2, (3, 2, 128, 9))], ids=_rid)
def test_syncbn_memory_contract(guards, case, half):
    """Every new entry point on guarded, poisoned buffers: moments, gathered arrays, sums, y / dx, parameter gradients and scratch.
    No guard byte changes and no NaN is left in a result (an element nobody wrote, or one computed from scratch nobody wrote)."""
    R, shape = case
    a, _ = _check_vs_float64([shape[1]] * R, shape, "lrelu", False, half, alloc=guards)
    assert guards.handed.get("workspace", 0) == 2 * R + 2 * R and guards.handed.get("empty_cl", 0) == 2 * R
    for o in a:
        for t, name in zip(o, ("y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "mean", "rstd")):
            assert not torch.isnan(t.float()).any(), name


@pytest.fixture
def slots(monkeypatch):
    recs = []
    real = ops.set_amax

    def set_amax(t, slot, ep):
        recs.append((t, slot, ep))
        return real(t, slot, ep)
    monkeypatch.setattr(ops, "set_amax", set_amax)
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", [(1, 2, 8, 6), (3, 2, 128, 9), (1, 2, 12, 6)], ids=lambda s: "x".join(str(v) for v in s))
def test_syncbn_absmax_slots(slots, shape, where):
    """The _amax forms: the tag of y and of dx of each of two ranks equals max|t| bit for bit, with a peak planted in the first / the
    last pixel of the last sample of rank 1 (test_bn_absmax_slots, statistics over both ranks)."""
    assert ops.X3_PLANES == 2
    S, Bs, C, H = shape
    parts = [Bs, Bs]
    B = S * 2 * Bs
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, H, generator=g)
    gy = torch.randn(B, C, H, H, generator=g)
    n, c = B - 1, C - 1
    h = w = 0 if where == "first" else H - 1
    x[n, c, h, w] = 60.0
    gy[n, c, h, w] = 500.0
    ga_, be = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    ga_[c] = 1.5
    a = _virtual_ranks(S, parts, "lrelu", x, ga_, be, gy, False)
    assert len(slots) == 4                                   # y and dx of rank 0, then of rank 1
    for r in range(2):
        (ty, sy, ey), (tdx, sdx, edx) = slots[2 * r], slots[2 * r + 1]
        assert ty.data_ptr() == a[r][0].data_ptr() and torch.equal(tdx, a[r][1])
        _assert_tag(ty, sy, ey, "y of rank %d" % r)
        _assert_tag(tdx, sdx, edx, "dx of rank %d" % r)
    y1 = a[1][0]
    am = y1.abs().reshape(-1).argmax()
    assert tuple(int(v) for v in np.unravel_index(int(am), tuple(y1.shape))) == (S * Bs - 1, c, h, w)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the tiny 'bn' Solver, one rank over real RCCL
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_iterations(dev, cfg, batch, dp_kwargs=None):
    host.set_noise(host.HostNoise())
    torch.manual_seed(1234)
    from solver import Solver
    trainer = Solver(cfg, dev, None).to(dev)
    trainer.copy_nets()
    if dp_kwargs is not None:
        trainer.enable_data_parallel(**dp_kwargs)
    calls = {id(m): 0 for m in trainer.dis.bn_layers()}
    for m in trainer.dis.bn_layers():
        m.register_forward_hook(lambda mod, i, o: calls.__setitem__(id(mod), calls[id(mod)] + int(mod.training and torch.is_grad_enabled())))
    grads = {}
    for it in range(2):
        torch.manual_seed(99 + it)
        a = (batch["x_real"], batch["c_src"], batch["c_trg"], batch["txt"], batch["txt_lens"], batch["label_src"],
             batch["label_trg"], cfg, it)
        trainer.dis_update(*a)
        grads["dis%d" % it] = {k: p.grad.detach().clone() for k, p in trainer.dis.named_parameters() if p.grad is not None}
        trainer.gen_update(*a)
        grads["gen%d" % it] = {k: p.grad.detach().clone() for k, p in trainer.gen.named_parameters() if p.grad is not None}
        trainer.smooth_moving()
        trainer.update_learning_rate()
        trainer.update_attention_status(it)
    torch.cuda.synchronize()
    return trainer, grads, calls


@pytest.mark.gpu
def test_one_rank_rccl_sync_bn_equals_plain_trainer(tmp_path, monkeypatch):
    """dis.norm 'bn', enable_data_parallel(sync_bn=True) with DWC_FORCE_DP=1 on a world_size-1 RCCL group, in this process (file
    rendezvous): the phase path with R = 1 and real all-gathers.  Two iterations reproduce the plain trainer's gradients, parameters
    and BN buffers exactly; every BN layer issued two all-gathers per taped training-mode call (one per pass); no warning."""
    import torch.distributed as dist
    from hipdwc import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = synth.make_config(image_size=32, tiny=True, lstm_dropout=0.0)
    cfg["dis"]["norm"] = "bn"
    batch = {k: v.to(dev) for k, v in synth.make_batch(3, 32, seed=5).items()}
    monkeypatch.setenv("DWC_FORCE_DP", "1")
    dist.init_process_group("nccl", device_id=dev, init_method="file://" + str(tmp_path / "rdv"), rank=0, world_size=1)
    try:
        plain, g_plain, _ = _two_iterations(dev, cfg, batch)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            dp_, g_dp, calls = _two_iterations(dev, cfg, batch, dict(bucket_bytes=64 << 10, sync_bn=True))
    finally:
        host.set_noise(host.DeviceNoise())
        dist.destroy_process_group()
    assert not [w for w in caught if "bn" in str(w.message)], [str(w.message) for w in caught]
    layers = dp_.dis.bn_layers()
    assert len(layers) == 4 and all(isinstance(m.sync, syncbn.GroupSync) and m.sync.force for m in layers)
    assert all(m.sync is None for m in plain.dis.bn_layers())
    assert all(c.sync is m.sync for c, m in zip(dp_.dis_copy.bn_layers(), layers)) or all(c.sync is None for c in dp_.dis_copy.bn_layers())
    for m in layers:
        print("bn layer: %d taped training calls, %d all-gathers, %d bytes" % (calls[id(m)], m.sync.calls, m.sync.bytes))
        assert calls[id(m)] == 4                             # a D and a G step per iteration, one D pass each
        assert m.sync.calls == 2 * calls[id(m)]              # the forward's moments and the backward's sums
    for step in g_plain:
        assert set(g_plain[step]) == set(g_dp[step]), step
        for k in g_plain[step]:
            assert torch.equal(g_plain[step][k], g_dp[step][k]), (step, k)
    for (k, p), (_, q) in zip(list(plain.gen.named_parameters()) + list(plain.dis.named_parameters()),
                              list(dp_.gen.named_parameters()) + list(dp_.dis.named_parameters())):
        assert torch.equal(p, q), k
    bp, bd = _buffers(plain), _buffers(dp_)
    assert bp.keys() == bd.keys() and len(bp) == 12
    for k in bp:
        assert torch.equal(bp[k], bd[k]), k
