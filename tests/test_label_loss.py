"""mh_label_loss: the reference's six scalar (x, y, mask) losses -- mean_l1, sum_l1, mean_l2, sum_l2, mean_huber, sum_huber (Losses/loss_factory.py:28-108) --
with their gradients under the two validity rules of get_proxy_loss (rule 0) and get_supervised_loss (rule 1).

Oracles: (a) tests/golden/ref_label_losses.npz, minted by executing the reference's own builders (tests/golden/make_ref_label_losses_golden.py); (b) `restate`
below, the table of include/madnet_hip.h in float64.  Bounds of both: result[0] within 2e-6 relative, result[1] exact, gradient within 1e-5 max|g| -- the bounds
tests/test_proxy_scaled.py holds mean_l1 to.  They hold for every loss here by the same argument: a float32 difference of two values <= 200 is off by at most
half an ulp(200) = 7.6e-6, every per-pixel term and gradient is one or two float32 roundings of it (6e-8 relative each), the sum of 256 non-negative terms in a
fixed tree adds at most 8 more roundings (5e-7 relative), the rest is float64."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import footprint as FP
from madnet_hip import _ffi, ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_label_losses.npz")
NAMES = ("mean_l1", "sum_l1", "mean_l2", "sum_l2", "mean_huber", "sum_huber")
MH_ERR_ARG = -1


def restate(name, pred, label, rule, hi, weight, npix=None):
    """float64: (weight * sum(v phi) / n, sum(v), weight * v phi' / n); pred, label: float64 tensors of one shape; npix: mean_huber's divisor (default: all)"""
    v = ~(((label == 0) if rule == 1 else (label <= 0)) | (label >= hi))
    d = pred - label
    fam = name.split("_")[1]
    if fam == "l1":
        phi, dphi = d.abs(), torch.sign(d)
    elif fam == "l2":
        phi, dphi = d * d, 2.0 * d
    else:           # the test is on the SIGNED difference and d == 1 is quadratic
        phi = torch.where(d > 1.0, 0.5 + (d.abs() - 1.0), 0.5 * d * d)
        dphi = torch.where(d > 1.0, torch.ones_like(d), d)
    vf = v.to(torch.float64)
    nvalid = vf.sum()
    if name in ("mean_l1", "mean_l2"):
        n = nvalid
    elif name == "mean_huber":
        n = float(d.numel() if npix is None else npix)
    else:
        n = 1.0
    return weight * (vf * phi).sum() / n, nvalid, weight * vf * dphi / n


def formula(name, pred, label, valid, weight, npix=None):
    """the same losses as one differentiable expression (autograd supplies the gradient, as TF does in the reference): weight * loss(pred, label, valid);
    valid: a 0 / 1 tensor of pred's type"""
    d = pred - label
    fam = name.split("_")[1]
    phi = d.abs() if fam == "l1" else (d * d if fam == "l2" else torch.where(d > 1.0, 0.5 + (d.abs() - 1.0), 0.5 * d * d))
    n = valid.sum() if name in ("mean_l1", "mean_l2") else (float(d.numel() if npix is None else npix) if name == "mean_huber" else 1.0)
    return weight * (valid * phi).sum() / n


def test_restatement_names_the_ffi_numbers():
    assert tuple(_ffi.LABEL_LOSS) == NAMES and [_ffi.LABEL_LOSS[n] for n in NAMES] == list(range(6))


def _run(backend, name, rule, hi, pred, label, weight=1.0, grad_scale=1.0, with_grad=True, poison=float("nan")):
    """-> (result [2], dpred [B,H,W] or None) on the CPU; ws / result / dpred in guarded allocations of the stated sizes, poisoned, guards checked"""
    lib, dev = backend.lib, backend.device
    B, H, W = pred.shape
    ws = FP.Guarded(lib.proxy_ws_floats(B, H, W), torch.float32, dev)
    res = FP.Guarded(2, torch.float32, dev)
    dp = FP.Guarded(B * H * W, torch.float32, dev) if with_grad else None
    for g in (ws, res, dp):
        if g is not None:
            g.t.fill_(poison)
    ops.label_loss(lib, pred.to(dev), label.to(dev), ws.t, res.t, name, rule, hi, dpred=dp.t.view(B, H, W) if with_grad else None, weight=weight, grad_scale=grad_scale)
    backend.sync()
    what = "label_loss %s rule %d %s" % (name, rule, (B, H, W))
    ws.assert_guards(what); res.assert_guards(what)
    if with_grad:
        dp.assert_guards(what)
    return res.t.cpu().clone(), (dp.t.cpu().view(B, H, W).clone() if with_grad else None)


def _check(res, dp, ref, nvalid, gref, what):
    ref, nvalid = float(ref), float(nvalid)
    gmax = gref.abs().max().item()
    print("%s: loss %.9g (oracle %.9g)  valid %d (oracle %d)  max|g err| %.3g  max|g| %.3g" % (what, res[0].item(), ref, int(res[1].item()), int(nvalid),
                                                                                               (dp.double() - gref).abs().max().item(), gmax))
    assert abs(res[0].item() - ref) <= 2e-6 * max(1.0, abs(ref)), what
    assert res[1].item() == nvalid, what
    assert torch.isfinite(dp).all(), what                   # every element written
    assert (dp.double() - gref).abs().max().item() <= 1e-5 * gmax, what
    assert (dp[gref == 0] == 0).all(), what


# ---- a. the reference's own builders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_label_loss_equals_the_reference_builders(backend, name):
    z = np.load(GOLD)
    pred = torch.from_numpy(z["pred"][..., 0])
    for tag, labels, rule, weight in (("sup", z["target"], 1, 1.0), ("proxy", z["proxy"], 0, 0.01)):
        label = torch.from_numpy(labels[..., 0])
        res, dp = _run(backend, name, rule, 192.0, pred, label, weight=weight)
        gref = torch.from_numpy(z["%s_grad_%s" % (tag, name)][..., 0]).double()
        nvalid = restate(name, pred.double(), label.double(), rule, 192.0, weight)[1]
        _check(res, dp, z["%s_loss_%s" % (tag, name)], nvalid, gref, "%s %s" % (tag, name))


# ---- b. float64 restatement, shapes around the 256-pixel workgroup ----------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 7, 9), (2, 37, 53), (1, 64, 128), (1, 160, 416)]
_data = {}


def _case(shape):
    """seeded predictions in (0, 160) and labels in (1, 150) with holes at 0, negative labels and labels at and above 192; the first seed at which no valid
    pixel of either rule has |d| < 1e-4 (the sign of l1's gradient is then the same in any arithmetic).  Pixel 0 is always valid.  Made once, read-only."""
    if shape not in _data:
        for seed in range(1, 40):
            g = torch.Generator().manual_seed(1000 * seed + sum(shape))
            pred = torch.rand(shape, generator=g) * 160.0
            label = 1.0 + torch.rand(shape, generator=g) * 149.0
            u = torch.rand(shape, generator=g)
            label[u < 0.2] = 0.0
            label[(u >= 0.2) & (u < 0.25)] = -3.0
            label[(u >= 0.25) & (u < 0.3)] = 192.0
            label[(u >= 0.3) & (u < 0.33)] = 230.0
            label.view(-1)[0], pred.view(-1)[0] = 37.25, 40.5
            d = (pred.double() - label.double()).abs()
            if all(d[~(bad | (label >= 192.0))].min().item() >= 1e-4 for bad in (label <= 0, label == 0)):
                break
        else:
            raise AssertionError("no unambiguous seed")
        _data[shape] = (pred, label)
    return _data[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("name", NAMES)
def test_label_loss_equals_the_float64_restatement(backend, name, shape):
    pred, label = _case(shape)
    for rule, hi, weight, gs in ((0, 192.0, 0.01, 1.0), (1, 200.0, 0.7, 0.5)):          # (rule 1 with hi = 200: the labels at 192 are valid, those at 230 not)
        ref, nvalid, gref = restate(name, pred.double(), label.double(), rule, hi, weight)
        res, dp = _run(backend, name, rule, hi, pred, label, weight=weight, grad_scale=gs)
        _check(res, dp, ref, nvalid, gs * gref, "%s rule %d %s" % (name, rule, shape))
        if pred.numel() > 1:
            assert (gref == 0).any() and (gref != 0).any()


# ---- c. MH_LOSS_MEAN_L1 is the three existing entry points, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 160, 416)], ids=lambda s: "%dx%dx%d" % s)
def test_mean_l1_equals_the_existing_entry_points_on_bits(backend, shape):
    lib, dev = backend.lib, backend.device
    B, H, W = shape
    pred, label = _case(shape)
    pd, ld = pred.to(dev), label.to(dev)

    def call(fn):
        ws = torch.zeros(max(lib.proxy_ws_floats(B, H, W), lib.proxy_scaled_ws_floats(B, H, W, 2)), device=dev)
        res = torch.full((4,), 7.0, device=dev)
        dp = torch.full((B, H, W), float("nan"), device=dev)
        fn(ws, res, dp)
        backend.sync()
        return FP.bits(res[:2]), FP.bits(dp)

    pairs = [(lambda ws, res, dp: ops.proxy_loss(lib, pd, ld, ws, res, dp, weight=0.01, grad_scale=0.5),
              lambda ws, res, dp: ops.label_loss(lib, pd, ld, ws, res, "mean_l1", 0, 192.0, dpred=dp, weight=0.01, grad_scale=0.5)),
             (lambda ws, res, dp: ops.supervised_loss(lib, pd, ld, ws, res, dp, weight=0.8, grad_scale=1.0, max_disp=150.0),
              lambda ws, res, dp: ops.label_loss(lib, pd, ld, ws, res, "mean_l1", 1, 150.0, dpred=dp, weight=0.8, grad_scale=1.0)),
             (lambda ws, res, dp: ops.proxy_loss_scaled(lib, pd, ld, ws, res, 2, dp, weight=0.1, grad_scale=1.0),
              lambda ws, res, dp: lib.label_loss_scaled(C.c_void_p(pd.data_ptr()), C.c_void_p(ld.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(res.data_ptr()),
                                                        C.c_void_p(dp.data_ptr()), 0, 0.1, 1.0, 2, B, H, W, None))]
    for old, new in pairs:
        (r0, g0), (r1, g1) = call(old), call(new)
        assert torch.equal(r0, r1) and torch.equal(g0, g1)
        assert not torch.isnan(g0.view(torch.float32)).any()


# ---- d. Huber's asymmetry at hand-set pixels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,value,grad", [(-5.0, 12.5, -5.0), (5.0, 4.5, 1.0), (1.0, 0.5, 1.0)], ids=["d=-5", "d=+5", "d=1"])
def test_huber_tests_the_signed_difference(backend, d, value, grad):
    label = torch.full((1, 1, 1), 20.0)
    pred = label + d
    for name in ("sum_huber", "mean_huber"):                # (one pixel: the mean divides by 1)
        for rule in (0, 1):
            res, dp = _run(backend, name, rule, 192.0, pred, label)
            assert (res[0].item(), res[1].item(), dp.item()) == (value, 1.0, grad), (name, rule)


def test_mean_huber_divides_by_all_pixels(backend):
    """d = -5, +5, 1 and one invalid pixel: (12.5 + 4.5 + 0.5) / 4, the gradients / 4"""
    label = torch.tensor([10.0, 20.0, 30.0, 0.0]).view(1, 2, 2)
    pred = torch.tensor([5.0, 25.0, 31.0, 99.0]).view(1, 2, 2)
    res, dp = _run(backend, "mean_huber", 0, 192.0, pred, label)
    assert res.tolist() == [17.5 / 4, 3.0] and dp.view(-1).tolist() == [-1.25, 0.25, 0.25, 0.0]
    res, dp = _run(backend, "sum_huber", 0, 192.0, pred, label)
    assert res.tolist() == [17.5, 3.0] and dp.view(-1).tolist() == [-5.0, 1.0, 1.0, 0.0]


# ---- e. no valid pixel; no gradient asked for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_valid_pixel_and_no_gradient(backend, name):
    pred, _ = _case((1, 7, 9))
    res, dp = _run(backend, name, 0, 192.0, pred, torch.zeros(1, 7, 9))
    assert res[1].item() == 0.0
    if name in ("mean_l1", "mean_l2"):
        assert torch.isnan(res[0]).item()                   # 0 / 0, like the reference
    else:
        assert res[0].item() == 0.0 and (dp == 0).all()
    pred, label = _case((2, 37, 53))
    with_g, _ = _run(backend, name, 1, 192.0, pred, label, weight=0.3)
    without, none = _run(backend, name, 1, 192.0, pred, label, weight=0.3, with_grad=False)
    assert none is None and torch.equal(FP.bits(with_g), FP.bits(without))


# ---- f. two runs over two poisons -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_runs_over_poisoned_outputs_give_the_same_bits(backend, name):
    pred, label = _case((2, 37, 53))
    (r0, g0), (r1, g1) = (_run(backend, name, 0, 192.0, pred, label, weight=0.01, poison=p) for p in (float("nan"), 1.0e30))
    assert torch.equal(FP.bits(r0), FP.bits(r1)) and torch.equal(FP.bits(g0), FP.bits(g1))
    assert torch.isfinite(r0).all() and torch.isfinite(g0).all()


# ---- g. argument errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(backend):
    lib, dev = backend.lib, backend.device
    B, H, W = 1, 7, 9
    pred, label = (t.to(dev) for t in _case((B, H, W)))
    ws = torch.full((lib.proxy_ws_floats(B, H, W),), -7.0, device=dev)
    res = torch.full((2,), -7.0, device=dev)
    dp = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(pred=p(pred), label=p(label), ws=p(ws), result=p(res), dpred=p(dp), loss=5, rule=1, hi=192.0, weight=1.0, grad_scale=1.0, B=B, H=H, W=W, stream=None)
    bad = [dict(loss=-1), dict(loss=6), dict(rule=-1), dict(rule=2), dict(hi=0.0), dict(hi=-192.0), dict(hi=float("nan")), dict(pred=None), dict(label=None),
           dict(ws=None), dict(result=None), dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-7), dict(W=-9)]
    for change in bad:
        assert lib._raw_mh_label_loss(*dict(good, **change).values()) == MH_ERR_ARG, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_label_loss: ") and len(msg) > len("mh_label_loss: "), (change, msg)
    goods = dict(pred=p(pred), label=p(label), ws=p(ws), result=p(res), dpred=p(dp), loss=5, weight=1.0, grad_scale=1.0, scale=2, B=B, H=H, W=W, stream=None)
    bads = [dict(loss=-1), dict(loss=6), dict(pred=None), dict(label=None), dict(ws=None), dict(result=None), dict(B=0), dict(H=0), dict(W=0), dict(B=-1),
            dict(scale=0), dict(scale=-2), dict(scale=H + 1), dict(H=65536), dict(W=65536), dict(B=4, H=32768, W=16384)]
    for change in bads:
        assert lib._raw_mh_label_loss_scaled(*dict(goods, **change).values()) == MH_ERR_ARG, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_label_loss_scaled: ") and len(msg) > len("mh_label_loss_scaled: "), (change, msg)
    backend.sync()
    for t in (ws, res, dp):
        assert bool((t == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_label_loss(*good.values()) == 0 and lib._raw_mh_label_loss(*dict(good, dpred=None).values()) == 0
    assert lib._raw_mh_label_loss_scaled(*goods.values()) == 0
    backend.sync()
    assert bool((res != -7.0).all()) and bool((dp != -7.0).all())
    with pytest.raises(ValueError, match="unknown label loss"):
        ops.label_loss(lib, pred, label, ws, res, "ZNCC", 0, 192.0)
