"""``hipdwc.txt.regroup``: over which samples the text encoder's feature rows are formed (csrc/txt_glue.hip ``dwc_txt_regroup_*``,
DESIGN.md 27).  No GPU: the stock-op form in float64 against the reference expression

    torch.cat([final_h, final_c], dim=1).view(batch, -1)            (reference networks_v2.py:249)

applied per group of G samples, and on the concatenated batch for W virtual ranks (threads that meet in a barrier); its adjoint; the
four exports in header, ctypes table and library, and their refusals before any launch; the error and identity paths.  Everything is
movement: ``torch.equal``.  The fixture tests/golden/txt_group.npz (tests/golden/make_golden_txt_group.py) is consistent with itself.
"""
import os
import re
import threading

import numpy as np
import pytest
import torch

from hipdwc import _lib, txt

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = {"dwc_txt_regroup_fwd", "dwc_txt_regroup_bwd", "dwc_txt_regroup_rank_fwd", "dwc_txt_regroup_rank_bwd"}
FIXTURE = os.path.join(HERE, "golden", "txt_group.npz")
LAYERS = [1, 2, 3]
WIDTHS = [6, 8]                                      # 2H
GROUPS = [(1, 1), (4, 4), (6, 1), (6, 2), (6, 3), (10, 5)]
RANKS = [(1, 4), (2, 3), (3, 2), (3, 5)]


def ref_feat(h, c):
    """The reference's feature rows of final states h, c: [L, B, 2H] each (caller order)."""
    return torch.cat([h, c], dim=1).view(h.shape[1], -1)


def states(L, B, width, seed, grad=False):
    g = torch.Generator().manual_seed(seed)
    h, c = torch.randn(L, B, width, generator=g, dtype=torch.float64), torch.randn(L, B, width, generator=g, dtype=torch.float64)
    return (h.requires_grad_(True), c.requires_grad_(True)) if grad else (h, c)


class BarrierSync:
    """W threads of one process as ranks: all_gather meets in a barrier."""

    def __init__(self, world, rank, shared):
        self.world, self.rank, self.force, self.shared = world, rank, False, shared

    def all_gather(self, t):
        slots, barrier = self.shared
        slots[self.rank] = t.detach().clone()
        barrier.wait()
        out = torch.stack(list(slots))
        barrier.wait()
        return out


def on_ranks(W, fn):
    """fn(rank, sync) on W threads -> the list of results."""
    shared = ([None] * W, threading.Barrier(W))
    out, errs = [None] * W, []

    def rank(r):
        try:
            out[r] = fn(r, BarrierSync(W, r, shared))
        except Exception as e:      # a dead rank must not leave the others in the barrier
            errs.append(e)
            shared[1].abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(W)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not errs, errs
    return out


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("B,G", GROUPS)
def test_groups_are_the_reference_expression_per_group(B, G, L, width):
    h, c = states(L, B, width, 100 * B + 10 * G + L, grad=True)
    feat = ref_feat(h, c)
    got = txt.regroup(feat, group=G, layers=L)
    want = torch.cat([ref_feat(h[:, a:a + G], c[:, a:a + G]) for a in range(0, B, G)])
    assert got.dtype == torch.float64 and torch.equal(got, want)
    assert (got is feat) == (G == B)
    # the adjoint, against autograd through the reference expression itself
    ct = torch.randn(got.shape, generator=torch.Generator().manual_seed(B + G), dtype=torch.float64)
    gh, gc = torch.autograd.grad(got, (h, c), ct, retain_graph=True)
    wh, wc = torch.autograd.grad(want, (h, c), ct, retain_graph=True)
    assert torch.equal(gh, wh) and torch.equal(gc, wc)
    # ... and as the inverse permutation: regrouping the gradient gives the cotangent back
    d_feat, = torch.autograd.grad(got, feat, ct) if G != B else (ct,)
    assert torch.equal(txt.regroup(d_feat, group=G, layers=L), ct)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("W,Bl", RANKS)
def test_ranks_are_the_reference_expression_on_the_concatenated_batch(W, Bl, L, width):
    h, c = states(L, W * Bl, width, 100 * W + 10 * Bl + L)
    want = ref_feat(h, c)
    ct = torch.randn(want.shape, generator=torch.Generator().manual_seed(W + Bl), dtype=torch.float64)
    local = [ref_feat(h[:, r * Bl:(r + 1) * Bl], c[:, r * Bl:(r + 1) * Bl]).requires_grad_(True) for r in range(W)]

    def rank(r, sync):
        sync.force = True                                        # (W = 1: the rank form all the same)
        out = txt.regroup(local[r], sync=sync, layers=L)
        d, = torch.autograd.grad(out, local[r], ct[r * Bl:(r + 1) * Bl])
        return out.detach(), d
    res = on_ranks(W, rank)
    assert torch.equal(torch.cat([o for o, _ in res]), want)
    # the adjoint: the ranks' gradients, regrouped once more, are the cotangents (the global map is a permutation) ...
    grads = [d for _, d in res]
    back = on_ranks(W, lambda r, sync: (setattr(sync, "force", True), txt.regroup(grads[r], sync=sync, layers=L))[1])
    assert torch.equal(torch.cat(back), ct)
    # ... and they are autograd's through the reference expressions
    hg, cg = h.clone().requires_grad_(True), c.clone().requires_grad_(True)
    wh, wc = torch.autograd.grad(ref_feat(hg, cg), (hg, cg), ct)
    for r in range(W):
        hl, cl = hg[:, r * Bl:(r + 1) * Bl], cg[:, r * Bl:(r + 1) * Bl]
        gh, gc = torch.autograd.grad(ref_feat(hl, cl), (hl, cl), grads[r])
        assert torch.equal(gh, wh[:, r * Bl:(r + 1) * Bl]) and torch.equal(gc, wc[:, r * Bl:(r + 1) * Bl])


def test_one_rank_without_force_is_the_plain_path():
    feat = torch.randn(4, 16)
    assert txt.regroup(feat, sync=BarrierSync(1, 0, None), layers=2) is feat


def test_identity_and_error_paths():
    feat = torch.randn(6, 24)
    assert txt.regroup(feat) is feat and txt.regroup(feat, group=None, layers=3) is feat and txt.regroup(feat, group=6) is feat
    for g in (4, 5, 7, 12, -1):
        with pytest.raises(ValueError, match="does not divide the batch"):
            txt.regroup(feat, group=g, layers=1)
    sync = BarrierSync(2, 0, None)
    with pytest.raises(ValueError, match="exclude each other"):
        txt.regroup(feat, group=2, sync=sync, layers=1)
    with pytest.raises(ValueError, match="layers"):
        txt.regroup(feat, group=2, layers=5)                     # 24 is no multiple of 4 * 5
    with pytest.raises(ValueError, match="layers"):
        txt.regroup(feat, group=2)


def test_regroup_symbols_header_table_library():
    header = open(os.path.join(os.path.dirname(HERE), "include", "dwcgan_hip.h")).read()
    declared = set(re.findall(r"\b(dwc_[a-z0-9_]+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SIGNATURES)
    assert int(re.search(r"#define\s+DWC_ABI_VERSION\s+(\d+)\b", header).group(1)) == _lib.ABI_VERSION == 11      # additive
    lib = _lib.load()
    assert lib.dwc_version() == 11
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n


def test_regroup_exports_refuse_bad_arguments_before_any_launch():
    """No device is touched: the pointers are dummies and every call must return DWC_EINVAL from the host-side checks."""
    lib = _lib.load()
    p = 4096

    def group(fn, src=p, dst=p, L=2, B=6, H=4, G=2):
        return fn(src, dst, L, B, H, G, None)

    def rank(fn, src=p, dst=p, L=2, W=2, Bl=3, H=4, r=1):
        return fn(src, dst, L, W, Bl, H, r, None)

    sizes = [dict(L=4, B=1 << 28, G=1),                          # 2^31 rows
             dict(L=1, B=1 << 20, H=1 << 20, G=1 << 20),         # 2^21 rows of 2^21 floats: 2^40 16-byte words
             dict(L=1, B=1 << 30, H=1 << 30, G=1)]
    bad_group = [dict(src=None), dict(dst=None), dict(L=0), dict(L=-1), dict(L=_lib.TXT_MAX_LAYERS + 1), dict(B=0), dict(B=-6),
                 dict(H=0), dict(H=-4), dict(G=0), dict(G=-2), dict(G=4), dict(G=5), dict(G=12)] + sizes
    for fn in (lib.dwc_txt_regroup_fwd, lib.dwc_txt_regroup_bwd):
        for kw in bad_group:
            assert group(fn, **kw) == _lib.EINVAL, kw
    sizes = [dict(L=4, W=1 << 14, Bl=1 << 14, r=0), dict(L=1, W=1 << 16, Bl=1 << 16), dict(L=1, W=1 << 30, Bl=1 << 30),
             dict(L=1, W=2, Bl=1 << 19, H=1 << 20)]
    bad_rank = [dict(src=None), dict(dst=None), dict(L=0), dict(L=_lib.TXT_MAX_LAYERS + 1), dict(W=0), dict(W=-2), dict(Bl=0),
                dict(Bl=-3), dict(H=0), dict(r=-1), dict(r=2), dict(r=7)] + sizes
    for fn in (lib.dwc_txt_regroup_rank_fwd, lib.dwc_txt_regroup_rank_bwd):
        for kw in bad_rank:
            assert rank(fn, **kw) == _lib.EINVAL, kw


def test_fixture_is_self_consistent():
    fx = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(HERE, "golden", "tiny_bn_step.npz"))
    lens = fx["lengths"].tolist()
    assert len(lens) == 6 and len(set(lens)) == 6
    n = sum(fx[k].size for k in fx.files if k.startswith("state/")) + fx["style"].size
    for G in (1, 2, 3):
        assert fx["g%d/g64" % G].shape == (n,) and fx["g%d/g64" % G].dtype == np.float64
        for k in ("mu", "lv"):
            a, b = fx["g%d/%s" % (G, k)], fx["g%d/%s64" % (G, k)]
            assert a.shape == (6, 12) and np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
    assert not np.array_equal(fx["g1/mu"], fx["g2/mu"]) and not np.array_equal(fx["g2/mu"], fx["g3/mu"])
