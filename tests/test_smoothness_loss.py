"""mh_smoothness_loss: the reference's edge-aware smoothness(x, y) (Losses/loss_factory.py:183-220) with its gradient w.r.t. the disparity.

Oracles: (a) tests/golden/ref_smoothness.npz, minted by executing the reference's own function (tests/golden/make_ref_smoothness_golden.py); (b)
smoothness_oracle.restate, the definition of include/madnet_hip.h in float64.  Bounds of both, those tests/test_label_loss.py holds the label losses to: value
within 2e-6 relative, gradient within 1e-5 max|g|, every gradient element finite.  They are safe here: the per-pixel term is two 8-term stencils of values <= 1
(each a few float32 roundings, 6e-8 relative), one exp that is accurate to an ulp, and a fixed-order sum of non-negative terms (<= 5e-7 relative), the rest is
float64; a float32 torch evaluation of the same formula sits at <= 5e-8 and <= 4e-7 max|g| on these shapes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import footprint as FP
import smoothness_oracle as SO
from madnet_hip import _ffi, ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_smoothness.npz")
MH_ERR_ARG = -1
T_H, T_W = _ffi.SMOOTH_TILE
SHAPES = [(1, 1, 1), (1, 3, 3), (1, 7, 9), (2, 37, 53), (1, T_H + 1, 2 * T_W + 1), (2, 2 * T_H - 1, T_W - 1)]
_ids = lambda s: "%dx%dx%d" % s
_data = {}


def _case(shape, C_):
    """seeded inputs and their float64 oracle, made once, read-only"""
    if (shape, C_) not in _data:
        disp, image = SO.case(*shape, C=C_)
        _data[(shape, C_)] = (disp, image) + SO.restate(disp, image)
    return _data[(shape, C_)]


def test_the_tile_constants_are_the_kernel_s(backend):
    lib = backend.lib
    assert lib.smoothness_ws_floats(1, T_H, T_W) == 1 and lib.smoothness_ws_floats(1, T_H + 1, T_W) == 2 and lib.smoothness_ws_floats(1, T_H, T_W + 1) == 2
    assert lib.smoothness_ws_floats(3, 2 * T_H + 1, 3 * T_W) == 27


def _run(backend, disp, image, weight=1.0, grad_scale=1.0, accumulate=False, with_grad=True, poison=float("nan"), prefill=None, phases=(0,)):
    """-> (result [4], ddisp [B,H,W] or None) on the CPU; ws of exactly mh_smoothness_ws_floats floats, result and ddisp in guarded allocations, poisoned (or
    prefilled: (result, ddisp)), guards checked"""
    lib, dev = backend.lib, backend.device
    B, H, W = disp.shape
    ws = FP.Guarded(lib.smoothness_ws_floats(B, H, W), torch.float32, dev)
    res = FP.Guarded(4, torch.float32, dev)
    dd = FP.Guarded(B * H * W, torch.float32, dev) if with_grad else None
    for g in (ws, res, dd):
        if g is not None:
            g.t.fill_(poison)
    if prefill is not None:
        res.t.copy_(prefill[0].to(dev))
        if with_grad:
            dd.t.copy_(prefill[1].reshape(-1).to(dev))
    for ph in phases:
        ops.smoothness_loss(lib, disp.to(dev), image.to(dev), ws.t, res.t, dd.t.view(B, H, W) if with_grad else None, weight=weight, grad_scale=grad_scale,
                            accumulate=accumulate, phase=ph)
    backend.sync()
    what = "smoothness_loss %s" % ((B, H, W),)
    ws.assert_guards(what); res.assert_guards(what)
    if with_grad:
        dd.assert_guards(what)
    return res.t.cpu().clone(), (dd.t.cpu().view(B, H, W).clone() if with_grad else None)


def _check(res, dd, ref, gref, what):
    ref = float(ref)
    gmax = gref.abs().max().item()
    print("%s: S %.9g (oracle %.9g, rel %.3g)  max|g err| %.3g  max|g| %.3g" % (what, res[0].item(), ref, abs(res[0].item() - ref) / max(abs(ref), 1e-30),
                                                                             (dd.double() - gref).abs().max().item(), gmax))
    assert abs(res[0].item() - ref) <= 2e-6 * abs(ref), what
    assert res[3].item() == res[0].item(), what
    assert torch.isnan(res[1:3]).all(), what                # result[1], result[2]: untouched poison
    assert torch.isfinite(dd).all(), what                   # every element written
    assert (dd.double() - gref).abs().max().item() <= 1e-5 * gmax, what
    assert (dd[gref == 0] == 0).all(), what


# ---- a. the reference's own function ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c3", "c1"])
def test_smoothness_equals_the_reference(backend, tag):
    z = np.load(GOLD)
    disp = torch.from_numpy(z["disp"][..., 0])
    image = torch.from_numpy(z["image" + tag[1]])
    res, dd = _run(backend, disp, image)
    _check(res, dd, z["loss_" + tag], torch.from_numpy(z["grad_" + tag][..., 0]).double(), "reference " + tag)
    s, g, _ = SO.restate(disp, image)                       # and the restatement IS the reference (which ran in float32: the bounds above)
    assert abs(s.item() - float(z["loss_" + tag])) <= 2e-6 * s.item() and (g - torch.from_numpy(z["grad_" + tag][..., 0]).double()).abs().max().item() <= 1e-5 * g.abs().max().item()


# ---- b. float64 restatement, shapes around the tile -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [3, 1], ids=["C3", "C1"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_smoothness_equals_the_float64_restatement(backend, shape, C_):
    disp, image, s, g, gmin = _case(shape, C_)
    for weight, gs in ((1.0, 1.0), (0.37, 0.5)):
        res, dd = _run(backend, disp, image, weight=weight, grad_scale=gs)
        if shape == (1, 1, 1):
            assert res[0].item() == 0.0 and res[3].item() == 0.0 and dd.item() == 0.0 and s.item() == 0.0
            continue
        assert gmin >= 1e-3
        _check(res, dd, weight * s, weight * gs * g, "%s C %d weight %g" % (shape, C_, weight))
        assert (g != 0).any()


def test_constant_regions_have_exactly_zero_gradient(backend):
    """a map with regions of constant disparity 0 and 40: where the restatement's gradient is exactly zero (inside the zero region: gx = gy = 0, sign(0) = 0) ours is"""
    B, H, W = 2, 37, 53
    disp, image, _, _, _ = _case((B, H, W), 3)
    disp = disp.clone()
    disp[:, 4:20, 6:30] = 0.0
    disp[:, 22:34, 28:50] = 40.0
    s, g, _ = SO.restate(disp, image)
    assert (g[:, 6:18, 8:28] == 0).all() and (g[:, 24:32, 30:48] != 0).any()        # (the second region is not zero: Ky sums to -2, the reference's literal)
    res, dd = _run(backend, disp, image)
    assert abs(res[0].item() - s.item()) <= 2e-6 * s.item()
    assert (dd[g == 0] == 0).all() and (dd.double() - g).abs().max().item() <= 1e-5 * g.abs().max().item()


# ---- c. accumulate, phases, determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, T_H + 1, 2 * T_W + 1)], ids=_ids)
def test_accumulate_adds_to_result_0_and_to_the_gradient(backend, shape):
    disp, image, s, g, _ = _case(shape, 3)
    gen = torch.Generator().manual_seed(5)
    gref = 0.37 * 0.5 * g
    gmax = gref.abs().max().item()
    known = ((torch.rand(shape, generator=gen) - 0.5) * gmax).float()        # a map of the gradient's own scale: the sum's rounding (<= 1.2e-7 gmax) stays inside the bound
    pre = torch.tensor([0.625, -3.0, 7.5, float("nan")])
    res, dd = _run(backend, disp, image, weight=0.37, grad_scale=0.5, accumulate=True, prefill=(pre, known))
    ws = 0.37 * s.item()
    assert abs(res[3].item() - ws) <= 2e-6 * ws
    assert res[0].item() == (torch.tensor(0.625) + res[3]).item()            # one float32 addition to what was there
    assert res[1].item() == -3.0 and res[2].item() == 7.5
    assert torch.isfinite(dd).all() and (dd.double() - known.double() - gref).abs().max().item() <= 1e-5 * gmax
    only, donly = _run(backend, disp, image, weight=0.37, grad_scale=0.5)
    assert FP.bits(only[3:4]).item() == FP.bits(res[3:4]).item() and only[0].item() == only[3].item()
    none, dnone = _run(backend, disp, image, weight=0.37, accumulate=True, prefill=(pre, known), with_grad=False)
    assert dnone is None and torch.equal(FP.bits(none[:3]), FP.bits(res[:3])) and none[3].item() == res[3].item()


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, T_H + 1, 2 * T_W + 1)], ids=_ids)
def test_phases_and_repeated_calls_give_the_same_bits(backend, shape):
    disp, image, _, _, _ = _case(shape, 3)
    r0, g0 = _run(backend, disp, image, weight=0.37)
    r12, g12 = _run(backend, disp, image, weight=0.37, phases=(1, 2))
    r1, g1 = _run(backend, disp, image, weight=0.37, poison=1.0e30)
    for r, g in ((r12, g12), (r1, g1)):
        assert torch.equal(FP.bits(r0[[0, 3]]), FP.bits(r[[0, 3]])) and torch.equal(FP.bits(g0), FP.bits(g))
    assert torch.isfinite(r0[[0, 3]]).all() and torch.isfinite(g0).all()
    # phase 1 alone leaves the result alone
    ronly, _ = _run(backend, disp, image, weight=0.37, phases=(1,))
    assert torch.isnan(ronly).all()


# ---- d. argument errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(backend):
    lib, dev = backend.lib, backend.device
    B, H, W = 1, 7, 9
    disp, image = (t.to(dev) for t in _case((B, H, W), 3)[:2])
    ws = torch.full((lib.smoothness_ws_floats(B, H, W),), -7.0, device=dev)
    res = torch.full((4,), -7.0, device=dev)
    dd = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(disp=p(disp), image=p(image), ws=p(ws), result=p(res), ddisp=p(dd), weight=1.0, grad_scale=1.0, accumulate=0, B=B, H=H, W=W, C=3, phase=0, stream=None)
    bad = [dict(C=0), dict(C=2), dict(C=4), dict(C=-1), dict(disp=None), dict(image=None), dict(ws=None), dict(result=None), dict(B=0), dict(H=0), dict(W=0),
           dict(B=-1), dict(H=-7), dict(W=-9), dict(phase=-1), dict(phase=3), dict(B=2, H=32768, W=32768), dict(B=1, H=65536, W=32768)]
    for change in bad:
        assert lib._raw_mh_smoothness_loss(*dict(good, **change).values()) == MH_ERR_ARG, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_smoothness_loss: ") and len(msg) > len("mh_smoothness_loss: "), (change, msg)
    backend.sync()
    for t in (ws, res, dd):
        assert bool((t == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_smoothness_loss(*good.values()) == 0 and lib._raw_mh_smoothness_loss(*dict(good, ddisp=None).values()) == 0
    backend.sync()
    assert bool((res[[0, 3]] != -7.0).all()) and bool((res[1:3] == -7.0).all()) and bool((dd != -7.0).all()) and bool((ws != -7.0).all())
