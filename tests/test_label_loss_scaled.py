"""mh_label_loss_scaled: the six label losses on a MAD block's prediction and the proxy labels at 1/s scale (--reprojectionScale), defined as mh_proxy_loss_scaled
is: p = R(pred), q = R(label) / s, valid = !(q <= 0 | q >= 192), the gradient R^T of the per-pixel one on the full grid.

Cases, data and the ambiguity check are those of tests/test_proxy_scaled.py; the oracle is composed the same way -- T.resize_bilinear -> / s -> the formula of
tests/test_label_loss.py -> autograd -- and held to the same bounds."""
import ctypes as C

import pytest
import torch

import footprint as FP
from madnet_hip import _ffi, ops
from test_label_loss import NAMES, formula
from test_proxy_scaled import CASES, _assert_unambiguous, _op_data, _scaled

_ref = {}


def _case(case, seed):
    """(pred, labels, valid) of a case, made and checked once"""
    if case not in _ref:
        B, H, W, s = case
        pred, px = _op_data(B, H, W, s, seed)
        _ref[case] = (pred, px, _assert_unambiguous(pred, px, s))
    return _ref[case]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case,seed", CASES, ids=["%dx%dx%d_s%d" % c for c, _ in CASES])
def test_label_loss_scaled_vs_composed_oracle(backend, case, seed, name):
    B, H, W, s = case
    lib, dev = backend.lib, backend.device
    pred, px, valid = _case(case, seed)
    weight = 0.1
    pc = pred.clone().requires_grad_(True)
    p, q = _scaled(pc, px, s)
    assert p.shape[1:3] == (H // s, W // s)
    ref = formula(name, p.double(), q.double(), valid.double(), weight, npix=B * (H // s) * (W // s))        # mean_huber divides by B (H // s) (W // s)
    (gref,) = torch.autograd.grad(ref, [pc])
    pd, xd = pred.to(dev), px.to(dev)
    outs = []
    for poison in (float("nan"), 1.0e30):
        ws = FP.Guarded(lib.proxy_scaled_ws_floats(B, H, W, s), torch.float32, dev)
        res = FP.Guarded(2, torch.float32, dev)
        dp = FP.Guarded(B * H * W, torch.float32, dev)
        for g in (ws, res, dp):
            g.t.fill_(poison)
        ops.proxy_loss_scaled(lib, pd, xd, ws.t, res.t, s, dp.t.view(B, H, W), weight=weight, grad_scale=1.0, loss=name)
        backend.sync()
        for g in (ws, res, dp):
            g.assert_guards("label_loss_scaled %s %s" % (name, case))
        outs.append((res.t.cpu().clone(), dp.t.cpu().view(B, H, W).clone()))
    res, dp = outs[0]
    print("%s: loss %.9g (oracle %.9g)  valid %d (oracle %d)  max|g err| %.3g  max|g| %.3g"
          % (name, res[0].item(), ref.item(), int(res[1].item()), int(valid.sum()), (dp - gref).abs().max().item(), gref.abs().max().item()))
    assert abs(res[0].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert res[1].item() == float(valid.sum().item())
    assert torch.isfinite(dp).all()                                              # every element written
    assert (dp - gref).abs().max().item() <= 1e-5 * gref.abs().max().item()
    assert (dp[gref == 0] == 0).all()
    assert (gref == 0).any() and (gref > 0).any() and (gref < 0).any()
    if (H % s, W % s, s) == (0, 0, 2):
        assert (dp[:, 1::2, :] == 0).all() and (dp[:, :, 1::2] == 0).all()       # exact ratio 2: odd rows / columns receive nothing
    assert torch.equal(FP.bits(outs[0][0]), FP.bits(outs[1][0])) and torch.equal(FP.bits(outs[0][1]), FP.bits(outs[1][1]))      # two runs, two poisons: the same bits


def test_mean_huber_scaled_divides_by_the_reduced_grid(backend):
    """constant maps, exact ratio: every output pixel has d = -3 (4.5 each), so the mean over B (H // s) (W // s) outputs is 4.5 whatever the full size"""
    lib, dev = backend.lib, backend.device
    B, H, W, s = 2, 8, 12, 2
    pred = torch.full((B, H, W), 7.0, device=dev)
    label = torch.full((B, H, W), 20.0, device=dev)
    ws = torch.zeros(lib.proxy_scaled_ws_floats(B, H, W, s), device=dev)
    res = torch.zeros(2, device=dev)
    ops.proxy_loss_scaled(lib, pred, label, ws, res, s, None, weight=1.0, loss="mean_huber")
    backend.sync()
    assert res.tolist() == [4.5, float(B * (H // s) * (W // s))]
    ops.proxy_loss_scaled(lib, pred, label, ws, res, s, None, weight=1.0, loss="sum_huber")
    backend.sync()
    assert res.tolist() == [4.5 * B * (H // s) * (W // s), float(B * (H // s) * (W // s))]


@pytest.mark.parametrize("case,seed", CASES, ids=["%dx%dx%d_s%d" % c for c, _ in CASES])
def test_mean_l1_scaled_equals_proxy_loss_scaled_on_bits(backend, case, seed):
    B, H, W, s = case
    lib, dev = backend.lib, backend.device
    pred, px, _ = _case(case, seed)
    pd, xd = pred.to(dev), px.to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    outs = []
    for new in (False, True):
        ws = torch.zeros(lib.proxy_scaled_ws_floats(B, H, W, s), device=dev)
        res = torch.full((2,), 7.0, device=dev)
        dp = torch.full((B, H, W), float("nan"), device=dev)
        if new:
            lib.label_loss_scaled(p(pd), p(xd), p(ws), p(res), p(dp), _ffi.LABEL_LOSS["mean_l1"], 0.1, 0.5, s, B, H, W, None)
        else:
            ops.proxy_loss_scaled(lib, pd, xd, ws, res, s, dp, weight=0.1, grad_scale=0.5)
        backend.sync()
        outs.append((FP.bits(res), FP.bits(dp), FP.bits(ws)))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
