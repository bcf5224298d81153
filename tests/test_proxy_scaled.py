"""The MAD blocks' proxy loss under --reprojectionScale s (Stereo_Continual_Adaptation.py:26-27,95-112): mh_proxy_loss_scaled resizes the block's full-size
prediction and the proxy labels to (H // s, W // s) on the fly, divides the labels by s and returns the masked mean L1 with its gradient on the full grid.

The oracle is composed from the existing oracle functions: resize_bilinear -> / s -> proxy_loss(., ., weight) -> autograd."""
import json
import os

import pytest
import torch

from madnet_hip import engine as E
from madnet_hip import ops
from madnet_hip import synthetic as S
from oracle import madnet as OM
from oracle import tf_ops as T
from test_engine_parity import _backend, _check, _proxy_from, _setup

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real-time-self-adaptive-deep-stereo_amd")


def _scaled(pred, proxy, s):
    """p = R(pred), q = R(proxy) / s on the (H // s, W // s) grid; pred / proxy: [B,H,W]"""
    B, H, W = pred.shape
    p = T.resize_bilinear(pred[..., None], H // s, W // s)
    q = T.resize_bilinear(proxy[..., None], H // s, W // s) / float(s)
    return p, q


def _assert_unambiguous(pred, proxy, s):
    """No resized label within 1e-3 of a threshold of the validity rule (0, 192) and no valid pixel with |p - q| < 1e-4: kernel and oracle then agree on
    every mask bit and every sign whatever their rounding.  A label that is EXACTLY 0 because every tap that carries weight is a hole (exactly 0) is no
    ambiguity -- 0 * w sums to 0 in any arithmetic -- and with an exact ratio (even sizes, s = 2: tx = ty = 0) 30 % of the labels are of that kind."""
    with torch.no_grad():
        p, q = _scaled(pred, proxy, s)
        all_holes = _scaled(pred, proxy.abs(), s)[1] == 0
        assert ((q.abs() >= 1e-3) | all_holes).all(), "a resized label within 1e-3 of 0"
        assert ((q - 192.0).abs() >= 1e-3).all(), "a resized label within 1e-3 of 192"
        valid = ~((q <= 0) | (q >= 192))
        assert ((p - q).abs()[valid] >= 1e-4).all(), "a valid pixel with |p - q| < 1e-4"
        return valid


def _op_data(B, H, W, s, seed):
    """dense ground truth + noise as labels, 30 % holes at exactly 0, a patch at 200 (and one at 200 s: still out of range after the division);
    the prediction lives at the labels' scale after the division, so that both signs of p - q occur"""
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0.0, 1.0, H).view(1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    gt = 6.0 + 80.0 * yy + 5.0 * torch.sin(xx / 7.0) + 3.0 * torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    px = gt + torch.randn(B, H, W, generator=g) * 1.5
    px[torch.rand(B, H, W, generator=g) < 0.3] = 0.0
    px[0, :2, :5] = 200.0
    px[B - 1, H - 3:, W - 4:] = 200.0 * s
    pred = gt / s + torch.randn(B, H, W, generator=g) * 2.0
    return pred.contiguous(), px.contiguous()


# seeds for which _assert_unambiguous holds at every pixel of the case
CASES = [((1, 64, 128, 2), 1),       # exact ratio: odd source pixels receive nothing
         ((2, 37, 53, 2), 1),        # fractional ratio, 18 x 26 = 468 outputs per image: a partial last workgroup, batch offset
         ((1, 37, 53, 3), 1),        # s = 3
         ((1, 9, 11, 4), 1),         # 2 x 2 outputs, the `hi` clamp on the last row / column
         ((1, 128, 256, 3), 1)]      # 128 -> 42 rows: fl(21 * fl(128 / 42)) is the integer 64, so the upper tap of output row 21 weighs EXACTLY 0 -- 11 labels of that
                                     # row have holes as lower taps and positive upper taps: 0 (invalid) only if the lerp weight is not left over from an fma


@pytest.mark.parametrize("case,seed", CASES, ids=["%dx%dx%d_s%d" % c for c, _ in CASES])
def test_proxy_loss_scaled_vs_composed_oracle(backend, case, seed):
    B, H, W, s = case
    dev = backend.device
    pred, px = _op_data(B, H, W, s, seed)
    valid = _assert_unambiguous(pred, px, s)
    weight = 0.1
    pc = pred.clone().requires_grad_(True)
    p, q = _scaled(pc, px, s)
    ref = T.proxy_loss(p, q, weight)
    (gref,) = torch.autograd.grad(ref, [pc])
    lib = backend.lib
    ws = torch.zeros(lib.proxy_scaled_ws_floats(B, H, W, s), device=dev)
    pd, xd = pred.to(dev), px.to(dev)
    outs = []
    for poison in (float("nan"), 1.0e30):
        res = torch.zeros(4, device=dev)
        dp = torch.full((B, H, W), poison, device=dev)
        ops.proxy_loss_scaled(lib, pd, xd, ws, res, s, dp, weight=weight, grad_scale=1.0)
        backend.sync()
        outs.append((res.cpu(), dp.cpu()))
    res, dp = outs[0]
    print("loss %.9g (oracle %.9g)  valid %d (oracle %d)  max|g err| %.3g  max|g| %.3g"
          % (res[0].item(), ref.item(), int(res[1].item()), int(valid.sum()), (dp - gref).abs().max().item(), gref.abs().max().item()))
    assert abs(res[0].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert res[1].item() == float(valid.sum().item())
    assert torch.isfinite(dp).all()                                              # every element written
    assert (dp - gref).abs().max().item() <= 1e-5 * gref.abs().max().item()
    assert (dp[gref == 0] == 0).all()
    assert (gref == 0).any() and (gref > 0).any() and (gref < 0).any()
    if (H % s, W % s, s) == (0, 0, 2):
        assert (dp[:, 1::2, :] == 0).all() and (dp[:, :, 1::2] == 0).all()       # exact ratio 2: odd rows / columns receive nothing
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])        # two runs, two poisons: the same bits


def test_proxy_loss_scaled_all_invalid_is_nan(backend):
    B, H, W, s = 1, 9, 11, 2
    dev = backend.device
    pred, _ = _op_data(B, H, W, s, 5)
    ws = torch.zeros(backend.lib.proxy_scaled_ws_floats(B, H, W, s), device=dev)
    res = torch.zeros(4, device=dev)
    ops.proxy_loss_scaled(backend.lib, pred.to(dev), torch.zeros(B, H, W, device=dev), ws, res, s, None, weight=0.1)
    backend.sync()
    assert torch.isnan(res[0]).item() and res[1].item() == 0.0


def test_proxy_loss_scaled_is_one_plan_op(backend):
    """the MAD proxy plan at scale s has no more plan ops than at scale 1, and no frame is resized"""
    from madnet_hip import _ffi
    eng, wn, wt, acc, (l, r, gt) = _setup(backend, 60, 100)
    eng.loss_kind = "proxy"
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    bv = sum([OM.layer_variables()[n] for n in blocks[4]], [])
    kinds = {}
    for s in (1, 2):
        eng.set_reprojection_scale(s)
        plan = eng.build_plan("MAD", lr=1e-2, block_vars=bv, block_level=E.LEVELS[4])
        kinds[s] = [plan.arr[k].kind for k in range(plan.n)]
    assert len(kinds[2]) <= len(kinds[1])
    assert _ffi.OP_RESIZE_IMAGE not in kinds[2]
    assert all(kinds[2].count(k) == kinds[1].count(k) for k in (_ffi.OP_RESIZE_FWD, _ffi.OP_RESIZE_BWD))        # no resize op stands in for the fused one
    assert kinds[2].count(_ffi.OP_PROXY_LOSS_SCALED) == 1 and kinds[2].count(_ffi.OP_PROXY_LOSS) == 1          # the block's loss / the full-resolution loss
    assert not hasattr(eng, "left_s") and not hasattr(eng, "p_s")               # only the workspace was allocated


def _oracle_mad_proxy_scaled(wt, acc, l, r, gt, px, bv, block, lr, s):
    """Stereo_Continual_Adaptation.py:75,95-112 + the momentum update: bulkhead forward, full-resolution proxy loss (0.01) + EPE / bad3, the block's proxy
    loss (0.1) on prediction and labels at 1/s scale, autograd over the block's variables"""
    for n in bv:
        wt[n].requires_grad_(True)
    disps = OM.forward(wt, l, r, bulkhead=True)
    full_loss = T.proxy_loss(disps[-1], px[..., None], 0.01)
    epe, bad3 = T.validation_metrics(disps[-1].detach(), gt)
    p = disps[block]
    assert p.shape[1] == l.shape[1]                       # the block's prediction is full-size: multiplier 1 (:107)
    Hs, Ws = l.shape[1] // s, l.shape[2] // s
    p_s = T.resize_bilinear(p, Hs, Ws)
    q = T.resize_bilinear(px[..., None], Hs, Ws) / float(s)
    loss_k = T.proxy_loss(p_s, q, 0.1)
    gl = torch.autograd.grad(loss_k, [wt[n] for n in bv], allow_unused=True)
    grads = {n: g.detach() for n, g in zip(bv, gl) if g is not None}
    for n in bv:
        wt[n].requires_grad_(False)
    OM.momentum_update(wt, acc, grads, lr)
    return {"loss": float(full_loss.detach()), "epe": float(epe), "bad3": float(bad3), "disparity": disps[-1].detach(), "grads": grads,
            "p_s": p_s.detach(), "q": q}


# the last entry: the seed of _proxy_from.  The labels of _proxy_from are noise around 0 wherever the sparse ground truth has a hole, so some resized label always
# comes close to 0; the seeds are the ones (of 3000 tried) that keep every mask / sign decision of the case furthest from its threshold.
MAD_CASES = [pytest.param("emul", (60, 100), 2, 4, 47, id="emul-60x100-s2-b4"),
             pytest.param("hip", (60, 100), 2, 4, 47, marks=pytest.mark.gpu, id="hip-60x100-s2-b4"),
             pytest.param("hip", (60, 100), 3, 1, 47, marks=pytest.mark.gpu, id="hip-60x100-s3-b1"),
             pytest.param("hip", (128, 256), 2, 4, 81, marks=pytest.mark.gpu, id="hip-128x256-s2-b4"),
             pytest.param("hip", (128, 256), 3, 1, 2282, marks=pytest.mark.gpu, id="hip-128x256-s3-b1")]
# a bilinear sample of labels <= 100 px rounds to within 3 ulp(100) = 2.3e-5 whatever the order of its three lerps; the engine's prediction is within ~1e-5 px of
# the oracle's (fp32 mode).  20 x that keeps both sides on the same side of every threshold.
MARGIN = 5e-4


@pytest.mark.parametrize("bname,size,scale,block,seed", MAD_CASES)
def test_mad_step_proxy_reprojection_scale(bname, size, scale, block, seed):
    """MAD step with loss_kind 'proxy' and reprojection scale s != 1 against the composed oracle with _check's criteria; the full-resolution loss and EPE / bad3
    equal the unscaled run's."""
    backend = _backend(bname)
    eng, wn, wt, acc, (l, r, gt) = _setup(backend, *size)
    px = _proxy_from(gt, seed)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    bv = sum([OM.layer_variables()[n] for n in blocks[block]], [])
    lr = 1e-2
    # the unscaled run on an engine of its own: its full-resolution numbers are the ones the scaled run must report
    eng1 = E.MadNetEngine(backend.lib, size[0], size[1], B=1, device=backend.device, weights=wn)
    eng1.loss_kind = "proxy"
    eng1.set_inputs(l, r, gt[..., 0], proxy=px)
    eng1.build_plan("MAD", lr=lr, block_vars=bv, block_level=E.LEVELS[block]).run(backend.lib, 0)
    backend.sync()
    full = (eng1.res_loss[0].item(), eng1.res_met[0].item(), eng1.res_met[1].item())
    eng.loss_kind = "proxy"
    eng.set_inputs(l, r, gt[..., 0], proxy=px)
    eng.set_reprojection_scale(scale)
    eng.build_plan("MAD", lr=lr, block_vars=bv, block_level=E.LEVELS[block]).run(backend.lib, 0)
    o = _oracle_mad_proxy_scaled(wt, acc, l, r, gt, px, bv, block, lr, scale)
    valid = ~((o["q"] <= 0) | (o["q"] >= 192))
    all_holes = T.resize_bilinear(px[..., None].abs(), o["q"].shape[1], o["q"].shape[2]) == 0
    margin = min(o["q"].abs()[~all_holes].min().item(), (o["q"] - 192.0).abs().min().item(), (o["p_s"] - o["q"]).abs()[valid].min().item())
    assert margin >= MARGIN, margin
    print("scale %d block %d: loss %.9g (oracle %.9g), smallest margin of a mask / sign decision %.3g" % (scale, block, eng.res_loss[0].item(), o["loss"], margin))
    _check(eng, wn, wt, o, backend)
    assert (eng.res_loss[0].item(), eng.res_met[0].item(), eng.res_met[1].item()) == full


@pytest.mark.gpu
def test_mad_proxy_scaled_graph_equals_eager_bit_for_bit(hip):
    """the criterion of test_captured_graph_replays_equal_the_eager_plan_bit_for_bit for the MAD proxy plan at scale 2, 60 x 100: four steps from the same weights,
    eager on streams vs the captured hipGraph, end with torch.equal weights, momentum, gradients and disparity"""
    H, W = 60, 100
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    bv = sum([OM.layer_variables()[n] for n in blocks[4]], [])
    pairs = [S.make_pair(H, W, frame=t) for t in range(4)]
    res = []
    for graph in (False, True):
        eng = E.MadNetEngine(hip.lib, H, W, B=1, device=hip.device, weights=wn, precision="mixed")
        eng.loss_kind = "proxy"
        eng.set_reprojection_scale(2)
        plan = eng.build_plan("MAD", lr=1e-3, block_vars=bv, block_level=E.LEVELS[4])
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            if graph:
                l, r, gt = pairs[0]
                eng.set_inputs(l, r, gt[..., 0], proxy=_proxy_from(torch.from_numpy(gt)))
                plan.capture(hip.lib, st.cuda_stream)
            for l, r, gt in pairs:
                eng.set_inputs(l, r, gt[..., 0], proxy=_proxy_from(torch.from_numpy(gt)))
                st.synchronize()
                plan.launch(hip.lib, st.cuda_stream)
                st.synchronize()
        res.append((eng.params.w.clone(), eng.params.m.clone(), eng.params.g.clone(), eng.pred.clone()))
        eng.close()
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a - b).abs().max().item()
    assert (res[0][1] != 0).any()
