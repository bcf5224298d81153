"""Reprojection loss past one tile, and the masked reductions past 256 partial sums (emulated build and, marked gpu, the MI355X).

loss_tile_kernel gives every workgroup a 16 x 32 pixel tile with a 2-pixel halo and one slot per partial sum in the workspace; loss_final_kernel sums the
slots in a loop strided by 256.  The shapes below are the smallest that reach: halo pixels owned by a neighbouring tile, edge tiles one pixel wide / high,
b > 0 with several tiles per frame, more tiles than ceil(B*H*W / 256) (the partial arrays once lay that far apart and overlapped), and 257 tiles (a second
pass of the final loop).  The workspace is a view of EXACTLY mh_loss_ws_floats() floats in front of a sentinel guard that no call may touch.

Reference: oracle/tf_ops.reprojection_loss in float64, gradient from autograd.  The per-pixel gradient bound is 8 * E32 + 1e-12, E32 = the largest
deviation of the float32 oracle's gradient from the float64 oracle's on the same inputs: kernel and float32 oracle do the same length of float32
arithmetic in another order and with other contraction (three bits of headroom), and one missing window coefficient -- about 1/9 of a pixel's SSIM
gradient, 1e-4 .. 1e-3 here -- stays three orders of magnitude above the bound.

Measured err / E32 (printed per shape by test_gradient_per_pixel), emulated build / MI355X:
    1x9x14 0.66 / 0.48   1x17x33 1.16 / 1.01   2x16x32 1.05 / 1.05   2x18x35 0.77 / 0.85   1x33x65 0.93 / 0.95   3x3x3 1.53 / 0.88
    1x3x70 0.78 / 0.83   1x40x3 1.27 / 1.27    100x3x3 1.16 / 1.23   1x3x8224 1.00 / 1.00  smooth 1.09 / 1.43        largest: 1.53 / 1.43
At (1,3,8224) E32 itself is large (4e-5, the gradients are <= 9e-5): near x = 8000 the float32 rounding of x - disp moves a few sampling positions across
an integer, the float32 oracle then reads other taps than the float64 one, and the kernel reads the float32 oracle's (ratio 1.00).  That shape is there for
the 257 partial sums of the loss values, not for the gradient.

The second half runs mh_metrics, mh_metrics_kitti, mh_proxy_loss, mh_supervised_loss and mh_proxy_loss_scaled (scale 1) at (1,260,257): 66820 pixels =
262 partial blocks, so the `i += 256` loop of every final kernel takes a second, partial pass -- against float64 numpy restatements of the definitions in
include/madnet_hip.h, with the edge values of every mask planted and the same exact-size workspace + guard.
"""
import functools

import numpy as np
import pytest
import torch

from madnet_hip import ops
from oracle import tf_ops as T

SENTINEL = -123.0
GUARD = 4096          # floats behind the workspace.  A layout that spaces the partial arrays too closely overruns by fewer floats than there are tiles (<= 257 here)


def _guarded(n, dev):
    """(allocation, workspace): the workspace is the first n floats of the allocation, the GUARD floats behind it must keep the sentinel"""
    buf = torch.full((int(n) + GUARD,), SENTINEL, device=dev)
    return buf, buf[:int(n)]


def _guard_intact(buf, n):
    g = buf[int(n):].cpu().view(torch.int32)
    return bool((g == torch.tensor(SENTINEL).view(torch.int32)).all().item())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# reprojection loss
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 9, 14),        # one tile (control)
               (1, 17, 33),       # 2 x 2 tiles, edge tiles one pixel wide and high
               (2, 16, 32),       # exactly full tiles, b > 0
               (2, 18, 35),       # edge tiles 2 / 3 pixels wide and high, b > 0 with 4 tiles per frame
               (1, 33, 65),       # 3 x 3 tiles: every halo pixel of the centre tile is a real pixel of a neighbour
               (3, 3, 3),         # minimum image, one window per frame
               (1, 3, 70),        # minimum height
               (1, 40, 3),        # minimum width
               (100, 3, 3),       # many frames of one nearly empty tile
               (1, 3, 8224)]      # 257 tiles: a second pass of the final kernel's loop
SMOOTH = "smooth"                 # ramp images at (1, 18, 35): SSIM denominators near C1 / C2, the clip boundary
_ids = lambda s: s if isinstance(s, str) else "%dx%dx%d" % s


def _oracle(disp, left, right, dtype):
    """loss, mean SSIM term, mean L1 term, d loss / d disp of tf_ops.reprojection_loss in `dtype` (the two means restated from its pieces)"""
    d = disp.to(dtype).requires_grad_(True)
    loss = T.reprojection_loss(d[..., None], left, right)
    (g,) = torch.autograd.grad(loss, [d])
    with torch.no_grad():
        l, r = left.to(dtype) / 256.0, right.to(dtype) / 256.0
        rep = T.warp_image(r, T.resize_bilinear(d[..., None], l.shape[1], l.shape[2]) * 1.0)
        ms, ml = T.ssim_map(rep, l).mean(), (rep - l).abs().mean()
        assert abs((0.85 * ms + 0.15 * ml).item() - loss.item()) <= 1e-6 * abs(loss.item())
    return loss.item(), ms.item(), ml.item(), g.detach()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (CPU) and both oracles of one shape, computed once and never modified"""
    if shape == SMOOTH:
        B, H, W = 1, 18, 35
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        left = torch.stack([xx * 3 + 10, yy * 5 + 20, xx + yy], -1)[None].contiguous()
        right = torch.stack([xx * 3 + 16, yy * 5 + 20, xx + yy + 2], -1)[None].contiguous()
        disp = torch.full((B, H, W), 2.25)
    else:
        B, H, W = shape
        g = torch.Generator().manual_seed(5)
        left = torch.floor(torch.rand(B, H, W, 3, generator=g) * 256)
        right = torch.floor(torch.rand(B, H, W, 3, generator=g) * 256)
        disp = torch.rand(B, H, W, generator=g) * 6 - 1                # warps run off both image edges
        assert all(not torch.equal(left[b], left[0]) and not torch.equal(right[b], right[0]) for b in range(1, B))
        assert (torch.arange(W, dtype=torch.float32) - disp).min() < 0 and (disp[..., W - 3:] < 0).any()       # off the left edge; a right tap at or past the last column
    loss, ms, ml, g64 = _oracle(disp, left, right, torch.float64)
    _, _, _, g32 = _oracle(disp, left, right, torch.float32)
    e32 = (g32.double() - g64).abs().max().item()
    return dict(B=B, H=H, W=W, left=left, right=right, disp=disp, loss=loss, ms=ms, ml=ml, g64=g64, e32=e32)


def _call(backend, c, grad=True, grad_scale=1.0, phases=(0,), buf=None, refill=True):
    """one mh_reprojection_loss (or its phases in turn) into an exact-size workspace inside a sentinel-filled allocation -> (result, ddisp, allocation, #ws floats)"""
    dev, lib = backend.device, backend.lib
    B, H, W = c["B"], c["H"], c["W"]
    n = lib.loss_ws_floats(B, H, W)
    if buf is None:
        buf, _ = _guarded(n, dev)
    elif refill:
        buf.fill_(SENTINEL)
    ws = buf[:n]
    res = torch.full((4,), float("nan"), device=dev)
    dd = torch.full((B, H, W), float("nan"), device=dev) if grad else None
    left, right, disp = c["left"].to(dev), c["right"].to(dev), c["disp"].to(dev)
    for ph in phases:
        ops.reprojection_loss(lib, left, right, disp, ws, res, dd, grad_scale=grad_scale, phase=ph)
    backend.sync()
    return res.cpu(), (dd.cpu() if grad else None), buf, n


@pytest.mark.parametrize("shape", LOSS_SHAPES + [SMOOTH], ids=_ids)
def test_loss_values(backend, shape):
    """result[0] = loss, result[1] = mean SSIM term, result[2] = mean L1 term against the float64 oracle"""
    c = _case(shape)
    res, _, _, _ = _call(backend, c)
    got = [res[k].item() for k in range(3)]
    ref = [c["loss"], c["ms"], c["ml"]]
    print("%s: result %r, float64 oracle %r" % (_ids(shape), got, ref))
    if shape == SMOOTH:
        assert abs(got[0] - ref[0]) <= 5e-6
    for a, b in zip(got, ref):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (got, ref)


@pytest.mark.parametrize("shape", LOSS_SHAPES + [SMOOTH], ids=_ids)
def test_gradient_per_pixel(backend, shape):
    """every element of ddisp written (NaN canary) and within 8 * E32 + 1e-12 of the float64 oracle's gradient"""
    c = _case(shape)
    _, dd, _, _ = _call(backend, c)
    assert torch.isfinite(dd).all()
    err = (dd.double() - c["g64"]).abs().max().item()
    print("%s on %s: max|ddisp - g64| %.3g  E32 %.3g  err/E32 %.2f  max|g64| %.3g"
          % (_ids(shape), backend.name, err, c["e32"], err / c["e32"], c["g64"].abs().max().item()))
    assert err <= 8 * c["e32"] + 1e-12, (err, c["e32"])


@pytest.mark.parametrize("shape", LOSS_SHAPES + [SMOOTH], ids=_ids)
def test_workspace_guard_untouched(backend, shape):
    """no call writes behind mh_loss_ws_floats() floats, with and without the gradient"""
    c = _case(shape)
    for grad in (True, False):
        _, _, buf, n = _call(backend, c, grad=grad)
        assert _guard_intact(buf, n), "the kernel wrote behind its workspace of %d floats" % n


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_ids)
def test_grad_scale_is_one_multiply(backend, shape):
    """grad_scale = 0.25 (a power of two): ddisp is 0.25 x the grad_scale = 1 gradient bit for bit, the loss values do not move"""
    c = _case(shape)
    r1, d1, _, _ = _call(backend, c)
    r2, d2, _, _ = _call(backend, c, grad_scale=0.25)
    assert torch.equal(_bits(d2), _bits(d1 * 0.25)) and torch.equal(_bits(r1[:3]), _bits(r2[:3]))


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_ids)
def test_forward_only_gives_the_same_result(backend, shape):
    """ddisp = NULL: result is bit-identical to the call with a gradient"""
    c = _case(shape)
    r1, _, _, _ = _call(backend, c)
    r2, _, _, _ = _call(backend, c, grad=False)
    assert torch.equal(_bits(r1[:3]), _bits(r2[:3])), (r1, r2)


@pytest.mark.parametrize("shape", [(2, 18, 35), (1, 3, 8224)], ids=_ids)
def test_phase_1_then_2_equals_phase_0(backend, shape):
    """mh_reprojection_loss_phase: maps + gradient, then the final reduction = the single call, result and ddisp bit for bit; result is not written before phase 2"""
    c = _case(shape)
    r0, d0, _, _ = _call(backend, c)
    r1, d1, buf, n = _call(backend, c, phases=(1,))
    assert torch.isnan(r1).all() and torch.equal(_bits(d1), _bits(d0))
    r12, d12, buf, n = _call(backend, c, phases=(1, 2))
    assert _guard_intact(buf, n)
    assert torch.equal(_bits(r12[:3]), _bits(r0[:3])), (r12, r0)
    assert torch.equal(_bits(d12), _bits(d0))
    assert all(abs(r12[k].item() - ref) <= 2e-6 * max(1.0, abs(ref)) for k, ref in enumerate([c["loss"], c["ms"], c["ml"]])), r12


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=_ids)
def test_second_call_into_the_same_workspace(backend, shape):
    """the partial sums are written before they are read: a call into the workspace the previous call left behind gives the same bits"""
    c = _case(shape)
    r1, d1, buf, n = _call(backend, c)
    r2, d2, buf, n = _call(backend, c, buf=buf, refill=False)
    assert torch.equal(_bits(r1[:3]), _bits(r2[:3])) and torch.equal(_bits(d1), _bits(d2)) and _guard_intact(buf, n)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# masked reductions: 262 partial blocks
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
RSHAPE = (1, 260, 257)            # 66820 pixels = 261 full blocks of 256 + one of 4: not a multiple of 256 partial sums, a partial last block
_f32 = np.float32


@functools.lru_cache(maxsize=None)
def _reduction_data(hi):
    """(pred, target) float32 [1,260,257]: targets 2 .. 1.2 hi with holes (exactly 0) and negative entries, errors on both sides of 3 px and of 5 %, and the
    edge value of every mask planted: target 0 / -0 / hi / one ulp below hi / negative, |pred - target| exactly 3 (targets that are multiples of 0.25, so
    target +- 3 is exact) and one ulp above 3, pred == target.  No other pixel lies within 1e-3 of the 3 px or the 5 % threshold, so every decision is
    the same in float32 and float64."""
    B, H, W = RSHAPE
    g = np.random.default_rng(29)
    t = g.uniform(2.0, 1.2 * hi, (B, H, W)).astype(_f32)
    t[g.random((B, H, W)) < 0.3] = 0.0
    t[g.random((B, H, W)) < 0.1] *= _f32(-1.0)
    err = np.where(g.random((B, H, W)) < 0.5, g.normal(0.0, 1.0, (B, H, W)), g.normal(0.0, 6.0, (B, H, W))).astype(_f32)
    p = (t + err).astype(_f32)
    planted = np.zeros((B, H, W), bool)
    t[0, 0, :5] = [0.0, hi, np.nextafter(_f32(hi), _f32(0.0)), -5.0, -0.0]
    t[0, H - 1, W - 1] = np.nextafter(_f32(hi), _f32(0.0))            # the 4-pixel block at the end holds an edge value too
    t[0, 1, :6] = [10.25, 20.5, 30.75, 96.0, 10.25, 64.5]
    p[0, 1, :6] = [13.25, 17.5, 33.75, 99.0, np.nextafter(_f32(13.25), _f32(14.0)), 64.5]        # |error| = 3, 3, 3, 3, 3 + one ulp, 0
    planted[0, 1, :6] = True
    for _ in range(200):          # any other error within 1e-3 of a threshold is stretched by 1 % until it is not
        d = np.abs(p.astype(np.float64) - t)
        near = ((np.abs(d - 3.0) < 1e-3) | ((t != 0) & (np.abs(d / np.where(t != 0, np.abs(t), 1.0) - 0.05) < 1e-3)) | (d < 1e-3)) & ~planted
        if not near.any():
            break
        p[near] = (t[near] + (p[near] - t[near]) * _f32(1.01) + _f32(0.002)).astype(_f32)
    assert not near.any()
    assert (np.abs(p[0, 1, :4] - t[0, 1, :4]) == 3.0).all() and np.abs(p[0, 1, 4] - t[0, 1, 4]) > 3.0
    assert np.nextafter(_f32(hi), _f32(0.0)) < hi
    p.setflags(write=False); t.setflags(write=False)
    return p, t


def _dev(a, dev):
    return torch.from_numpy(a.copy()).to(dev)


def _run_reduction(backend, n_ws, call, grad):
    """call(ws, res, dpred) into an exact-size workspace in front of the guard -> (result, dpred); result and dpred start from NaN"""
    dev = backend.device
    buf, ws = _guarded(n_ws, dev)
    res = torch.full((4,), float("nan"), device=dev)
    dp = torch.full(RSHAPE, float("nan"), device=dev) if grad else None
    call(ws, res, dp)
    backend.sync()
    assert _guard_intact(buf, n_ws), "the kernel wrote behind its workspace of %d floats" % n_ws
    return res.cpu().numpy().astype(np.float64), (dp.cpu().numpy() if grad else None)


def test_metrics_262_blocks(backend):
    """mh_metrics: valid = gt != 0 (a negative gt is valid), EPE = sum(valid |disp - gt|) / #valid, bad = #(valid |disp - gt| > th) / #valid, strict"""
    p, t = _reduction_data(192.0)
    dev, lib = backend.device, backend.lib
    valid = t != 0
    d = np.abs(p.astype(np.float64) - t) * valid
    epe, bad, nv = d.sum() / valid.sum(), (d > 3.0).sum() / valid.sum(), int(valid.sum())
    assert (t[valid] < 0).any() and (d == 3.0).sum() == 4
    res, _ = _run_reduction(backend, lib.metrics_ws_floats(*RSHAPE),
                            lambda ws, r, _: ops.metrics(lib, _dev(p, dev), _dev(t, dev), ws, r, 3.0), False)
    print("metrics: EPE %.9g (float64 %.9g)  bad %.9g (%.9g)  valid %d (%d)" % (res[0], epe, res[1], bad, res[2], nv))
    assert res[2] == float(nv)
    assert abs(res[0] - epe) <= 1e-5 * epe
    assert abs(res[1] - bad) <= 1e-6 and round(res[1] * nv) == int((d > 3.0).sum())


def test_metrics_kitti_262_blocks(backend):
    """mh_metrics_kitti: val = gt > 0, diff = |gt - disp| on val, EPE = mean(diff), D1 = 100 mean(diff > 3 && diff / gt >= 0.05)"""
    p, t = _reduction_data(192.0)
    dev, lib = backend.device, backend.lib
    val = t > 0
    d = np.abs(t[val].astype(np.float64) - p[val])
    out = (d > 3.0) & (d / t[val] >= 0.05)
    epe, d1, nv, nout = d.mean(), out.mean() * 100.0, int(val.sum()), int(out.sum())
    assert 0 < nout < nv and (d == 3.0).sum() == 4 and ((d > 3) & (d / t[val] < 0.05)).any() and ((d <= 3) & (d / t[val] >= 0.05)).any()
    res, _ = _run_reduction(backend, lib.metrics_kitti_ws_floats(*RSHAPE),
                            lambda ws, r, _: ops.metrics_kitti(lib, _dev(p, dev), _dev(t, dev), ws, r), False)
    print("metrics_kitti: EPE %.9g (float64 %.9g)  D1 %.9g (%.9g)  valid %d (%d)" % (res[0], epe, res[1], d1, res[2], nv))
    assert res[2] == float(nv)
    assert round(res[1] * nv / 100.0) == nout and abs(res[1] - d1) <= 1e-6 * d1
    assert abs(res[0] - epe) <= 1e-6 * epe


def _masked_l1(p, t, valid, weight, gs):
    """float64: weight * sum(valid |p - t|) / #valid, its gradient gs * weight * valid * sign(p - t) / #valid, #valid"""
    d = p.astype(np.float64) - t
    nv = valid.sum()
    return weight * (np.abs(d) * valid).sum() / nv, gs * weight * valid * np.sign(d) / nv, int(nv)


def _check_masked_l1(name, res, dp, ref, gref, nv):
    """the bounds of test_proxy_loss_and_grad / test_supervised_loss_and_grad / test_proxy_loss_scaled_vs_composed_oracle; the gradient bound is the scaled test's
    1e-5 max|g| (the 1e-5 max(1, max|g|) of the other two would be wider than the gradient itself at this size)"""
    print("%s: loss %.9g (float64 %.9g)  valid %d (%d)  max|g err| %.3g  max|g| %.3g" % (name, res[0], ref, res[1], nv, np.abs(dp - gref).max(), np.abs(gref).max()))
    assert abs(res[0] - ref) <= 2e-6 * max(1.0, abs(ref))
    assert res[1] == float(nv)
    assert np.isfinite(dp).all()                                      # every element written
    assert np.abs(dp - gref).max() <= 1e-5 * np.abs(gref).max()
    assert (dp[gref == 0] == 0).all() and (gref == 0).any() and (gref > 0).any() and (gref < 0).any()


def test_proxy_loss_262_blocks(backend):
    """mh_proxy_loss: valid = !(proxy <= 0 || proxy >= 192)"""
    p, t = _reduction_data(192.0)
    dev, lib = backend.device, backend.lib
    valid = ~((t <= 0) | (t >= 192.0))
    assert not valid[0, 0, 0] and not valid[0, 0, 1] and valid[0, 0, 2] and not valid[0, 0, 3] and not valid[0, 0, 4] and valid[0, -1, -1]
    ref, gref, nv = _masked_l1(p, t, valid, 0.1, 0.5)
    res, dp = _run_reduction(backend, lib.proxy_ws_floats(*RSHAPE),
                             lambda ws, r, g: ops.proxy_loss(lib, _dev(p, dev), _dev(t, dev), ws, r, g, weight=0.1, grad_scale=0.5), True)
    _check_masked_l1("proxy_loss", res, dp, ref, gref, nv)


def test_supervised_loss_262_blocks(backend):
    """mh_supervised_loss: valid = !(target == 0 || target >= max_disp), max_disp = 150.5: a negative target stays valid"""
    hi = 150.5
    p, t = _reduction_data(hi)
    dev, lib = backend.device, backend.lib
    valid = ~((t == 0) | (t >= hi))
    assert not valid[0, 0, 0] and not valid[0, 0, 1] and valid[0, 0, 2] and valid[0, 0, 3] and not valid[0, 0, 4] and (t[valid] < 0).any() and (t[~valid] > hi).any()
    ref, gref, nv = _masked_l1(p, t, valid, 0.7, 1.0)
    res, dp = _run_reduction(backend, lib.proxy_ws_floats(*RSHAPE),
                             lambda ws, r, g: ops.supervised_loss(lib, _dev(p, dev), _dev(t, dev), ws, r, g, weight=0.7, grad_scale=1.0,
                                                                  max_disp=hi), True)
    _check_masked_l1("supervised_loss", res, dp, ref, gref, nv)


def test_proxy_loss_scaled_at_scale_1_262_blocks(backend):
    """mh_proxy_loss_scaled, scale = 1: both resizes are the identity (every lerp weight is exactly 0) and the labels are divided by 1 -- mh_proxy_loss's numbers"""
    p, t = _reduction_data(192.0)
    dev, lib = backend.device, backend.lib
    valid = ~((t <= 0) | (t >= 192.0))
    ref, gref, nv = _masked_l1(p, t, valid, 0.1, 1.0)
    res, dp = _run_reduction(backend, lib.proxy_scaled_ws_floats(RSHAPE[0], RSHAPE[1], RSHAPE[2], 1),
                             lambda ws, r, g: ops.proxy_loss_scaled(lib, _dev(p, dev), _dev(t, dev), ws, r, 1, g, weight=0.1, grad_scale=1.0),
                             True)
    _check_masked_l1("proxy_loss_scaled", res, dp, ref, gref, nv)


@pytest.mark.parametrize("op", ["proxy", "supervised"])
def test_l1_loss_without_a_valid_pixel_is_nan(backend, op):
    """no valid pixel: result[0] = 0/0 = NaN like the TF graph, result[1] = 0 (mh_proxy_loss_scaled: test_proxy_loss_scaled_all_invalid_is_nan)"""
    B, H, W = 1, 9, 11
    dev, lib = backend.device, backend.lib
    g = torch.Generator().manual_seed(3)
    pred = torch.rand(B, H, W, generator=g).to(dev)
    if op == "proxy":
        target = -torch.rand(B, H, W, generator=g)
        target[0, ::2] = 0.0
        target[0, 1] = 192.0
    else:
        target = torch.zeros(B, H, W)
        target[0, ::2] = 192.0
        target[0, 1, ::2] = -0.0
    n = lib.proxy_ws_floats(B, H, W)
    buf, ws = _guarded(n, dev)
    res = torch.zeros(4, device=dev)
    if op == "proxy":
        ops.proxy_loss(lib, pred, target.to(dev), ws, res, None, weight=0.1)
    else:
        ops.supervised_loss(lib, pred, target.to(dev), ws, res, None, weight=0.7, max_disp=192.0)
    backend.sync()
    assert torch.isnan(res[0]).item() and res[1].item() == 0.0 and _guard_intact(buf, n)
