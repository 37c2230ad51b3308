"""ops._prepped / ops.refresh_prepared over every layout builder of ops._LAYOUTS, at the smallest shapes that reach each: a hit is
the same tensor, a changed parameter is never served from the cache (lazily rebuilt or refreshed in one launch, the same bits as a
build from a fresh clone either way), a composite layout leaves no slot behind for its temporary bank, a dead parameter leaves none."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from hipdwc import ops          # noqa: E402

DEV = "cuda:0"


def _cases():
    """(filter shape, kind, cout_pad, cin_pad, stride, half, refreshable: dwc_weight_refresh_multi has a recipe for it)"""
    out = []
    for half in (False, True):
        cip = 8 if half else 4
        for kind in ("fwd", "dgrad", "dgrad_t"):
            out.append(((8, 3, 3, 3), kind, 16, cip, 1, half, True))
            out.append(((8, 3, 4, 4), kind, 16, cip, 2, half, True))
    for kind in ("x3_fwd", "x3_dgrad", "h2_fwd", "h2_dgrad"):
        out.append(((16, 16, 3, 3), kind, 16, 16, 1, False, True))
        out.append(((8, 8, 3, 3), kind, 16, 16, 1, False, False))        # zero-padded through torch: rebuilt lazily
    for half, P, x3 in ((False, 4, "_x3"), (True, 8, "")):
        out.append(((64, 3, 7, 7), "stem_steps" + x3, 64, P, 1, half, False))
        out.append(((P, 64, 7, 7), "stem_steps_dgrad" + x3, 64, P, 1, half, False))
        out.append(((P, 64, 7, 7), "heads_wide", 32, 64, 1, half, False))
        out.append(((P, 64, 7, 7), "heads_narrow" + x3, 32, 64, 1, half, False))
        out.append(((64, 3, 7, 7), "dgrad_image", 64, P, 1, half, False))
        out.append(((64, 3, 7, 7), "dgrad_image_narrow" + x3, 64, P, 1, half, False))
    return out


CASES = _cases()


def test_every_builder_has_a_case():
    assert {c[1] for c in CASES} == set(ops._LAYOUTS)


def _bits(t, kind):
    t = t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t
    return t[:-4] if kind.startswith("h2") else t      # (h2: the last 8 bytes are the fused refresh's own absmax slot)


def _param(shape, seed):
    w = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * (shape[1] * shape[2] * shape[3]) ** -0.5
    return torch.nn.Parameter(w.to(DEV))


@pytest.mark.parametrize("shape,kind,cop,cip,stride,half,refreshable", CASES,
                         ids=["%s-%s-s%d-%s" % ("x".join(map(str, c[0])), c[1], c[4], "bf16" if c[5] else "fp32") for c in CASES])
def test_layout_follows_its_parameter(shape, kind, cop, cip, stride, half, refreshable):
    gc.collect()
    anchors = len(ops._WCACHE)
    w = _param(shape, 5)
    prep = lambda p: ops._prepped(p, kind, cop, cip, stride, None, half)
    fresh = lambda: _bits(prep(torch.nn.Parameter(w.detach().clone())), kind)
    delta = torch.randn(shape, generator=torch.Generator().manual_seed(6)).to(DEV) * 0.05

    first = prep(w)
    assert prep(w) is first
    # one slot, the parameter's: none for the wide bank a composite layout is made from
    assert len(ops._WCACHE) == anchors + 1 and id(w) in ops._WCACHE.slots
    assert torch.equal(_bits(first, kind), fresh())
    gc.collect()
    assert len(ops._WCACHE) == anchors + 1

    # a writer that goes through .data and bumps the version itself (dp.broadcast_module, host.moving_average): rebuilt at the next use
    w.data.add_(delta)
    torch._C._increment_version(w)
    lazy = prep(w)
    assert lazy is not first and prep(w) is lazy
    assert torch.equal(_bits(lazy, kind), fresh()) and not torch.equal(_bits(lazy, kind), _bits(first, kind))

    # an optimiser step, then the refresh FusedAdam.step ends with: one launch into the same tensor where there is a recipe
    with torch.no_grad():
        w.add_(delta)
    ptr, launches = lazy.data_ptr(), ops.REFRESH_STATS["launches"]
    assert ops.refresh_prepared([w]) == int(refreshable)
    assert ops.REFRESH_STATS["launches"] == launches + int(refreshable)
    got = prep(w)
    if refreshable:
        assert got is lazy and got.data_ptr() == ptr
    assert ops.refresh_prepared([w]) == 0
    assert torch.equal(_bits(got, kind), fresh()) and not torch.equal(_bits(got, kind), _bits(first, kind))

    wid = id(w)
    del w, prep, fresh
    gc.collect()
    assert wid not in ops._WCACHE.slots and len(ops._WCACHE) == anchors


def test_layout_of_a_derived_filter_lives_on_its_owners():
    """The filter is a fresh tensor at every call (stacked image heads): one slot, on the first owner; either owner's change misses."""
    gc.collect()
    anchors = len(ops._WCACHE)
    a, b = _param((2, 64, 7, 7), 7), _param((2, 64, 7, 7), 8)
    prep = lambda kind: ops._prepped(torch.cat([a.detach(), b.detach()], 0), kind, 32, 64, 1, (a, b), False)
    for kind in ("heads_wide", "heads_narrow_x3", "fwd"):
        first = prep(kind)
        assert prep(kind) is first
        assert len(ops._WCACHE) == anchors + 1 and id(a) in ops._WCACHE.slots and id(b) not in ops._WCACHE.slots
        for p in (a, b):
            with torch.no_grad():
                p.mul_(1.5)
            assert ops.refresh_prepared([a, b]) == 0
            again = prep(kind)
            assert again is not first and not torch.equal(_bits(again, kind), _bits(first, kind))
            w4 = torch.nn.Parameter(torch.cat([a.detach(), b.detach()], 0))
            assert torch.equal(_bits(again, kind), _bits(ops._prepped(w4, kind, 32, 64, 1, None, False), kind))
            first = again
            del w4
    del a, prep
    gc.collect()
    assert len(ops._WCACHE) == anchors
