"""KITTI D1-all and EPE inside the step (mh_metrics_kitti, Adapter(kitti_metrics=True)) against the numpy lines of the continual loop
(Stereo_Continual_Adaptation.py:245-249 of the reference):
    val = gt > 0; disp_diff = |gt[val] - disp[val]|; outliers = disp_diff > 3 and disp_diff / gt[val] >= 0.05; d1 = mean(outliers) * 100; epe = mean(disp_diff)"""
import json
import os

import numpy as np
import pytest
import torch

from madnet_hip import _ffi
from madnet_hip import dispnet_engine as DE
from madnet_hip import engine as E
from madnet_hip import ops
from madnet_hip.oplayout import lane_of
from madnet_hip import synthetic as S
from oracle import dispnet as OD
from oracle import madnet as OM

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real-time-self-adaptive-deep-stereo_amd")


def _reference(disp, gt):
    """the reference's lines on float32 arrays -> (epe, d1, #outliers, #valid)"""
    val = gt > 0
    disp_diff = np.abs(gt[val] - disp[val])
    outliers = np.logical_and(disp_diff > 3, (disp_diff / gt[val]) >= 0.05)
    return np.mean(disp_diff), np.mean(outliers) * 100., int(outliers.sum()), int(val.sum())


def _data(B, H, W, seed):
    """ground truth 2 .. 96 with holes (0) and negative entries (both invalid: val = gt > 0); errors on both sides of both thresholds"""
    g = np.random.default_rng(seed)
    gt = g.uniform(2.0, 96.0, (B, H, W)).astype(np.float32)
    gt[g.random((B, H, W)) < 0.3] = 0.0
    gt[g.random((B, H, W)) < 0.1] *= -1.0
    err = np.where(g.random((B, H, W)) < 0.5, g.normal(0.0, 1.0, (B, H, W)), g.normal(0.0, 6.0, (B, H, W))).astype(np.float32)
    disp = (gt + err).astype(np.float32)
    for _ in range(50):        # an error that lands within 2e-4 of a threshold (3 px, 5 %) is stretched by 1 % until it does not
        diff = np.abs(gt - disp)
        near = (gt > 0) & ((np.abs(diff - 3.0) < 2e-4) | (np.abs(diff / np.where(gt > 0, gt, 1.0) - 0.05) < 2e-4))
        if not near.any():
            break
        disp[near] = (gt[near] + (disp[near] - gt[near]) * np.float32(1.01)).astype(np.float32)
    return disp, gt


@pytest.mark.parametrize("shape,seed", [((1, 37, 53), 3), ((2, 64, 128), 3)], ids=["1x37x53", "2x64x128"])
def test_metrics_kitti_vs_reference_lines(backend, shape, seed):
    B, H, W = shape
    dev = backend.device
    disp, gt = _data(B, H, W, seed)
    val = gt > 0
    diff = np.abs(gt[val] - disp[val])
    # no pixel within 1e-4 of either threshold: every outlier decision is the same in any rounding
    assert (np.abs(diff - 3.0) >= 1e-4).all() and (np.abs(diff / gt[val] - 0.05) >= 1e-4).all()
    epe, d1, nout, nval = _reference(disp, gt)
    assert 0 < nout < nval and (gt < 0).any() and (gt == 0).any()
    assert ((diff > 3) & (diff / gt[val] < 0.05)).any() and ((diff <= 3) & (diff / gt[val] >= 0.05)).any()      # each clause of the rule decides somewhere
    lib = backend.lib
    ws = torch.zeros(lib.metrics_kitti_ws_floats(B, H, W), device=dev)
    res = torch.full((4,), -1.0, device=dev)
    ops.metrics_kitti(lib, torch.from_numpy(disp).to(dev), torch.from_numpy(gt).to(dev), ws, res)
    backend.sync()
    res = res.cpu().numpy()
    print("EPE %.9g (reference %.9g)  D1 %.9g (reference %.9g)  valid %d (reference %d)" % (res[0], epe, res[1], d1, res[2], nval))
    assert res[2] == float(nval)
    assert round(float(res[1]) * nval / 100.0) == nout and abs(float(res[1]) - d1) <= 1e-6 * d1
    assert abs(float(res[0]) - float(epe)) <= 1e-6 * float(epe)


def test_metrics_kitti_without_a_valid_pixel_is_nan(backend):
    B, H, W = 1, 9, 11
    dev = backend.device
    gt = -torch.rand(B, H, W); gt[0, ::2] = 0.0
    ws = torch.zeros(backend.lib.metrics_kitti_ws_floats(B, H, W), device=dev)
    res = torch.zeros(4, device=dev)
    ops.metrics_kitti(backend.lib, torch.rand(B, H, W).to(dev), gt.to(dev), ws, res)
    backend.sync()
    assert torch.isnan(res[0]).item() and torch.isnan(res[1]).item() and res[2].item() == 0.0


def _op_fields(plan):
    """kind, integer fields (geometry + scheduling word), float fields and count of every op; the pointer fields are left out: ops that reach their operands through
    a device table get a freshly built table with every recording"""
    return [(o.kind, tuple(o.i), tuple(o.f), o.n) for o in (plan.arr[k] for k in range(plan.n))]


@pytest.mark.parametrize("net", ["madnet", "dispnet"])
def test_default_plans_are_unchanged_and_the_report_is_one_more_op(backend, net):
    """kitti_metrics off: no plan holds the new op.  On: the same plan, op for op, with ONE mh_metrics_kitti right behind mh_metrics, on its lane."""
    H, W = 64, 128
    if net == "madnet":
        eng = E.MadNetEngine(backend.lib, H, W, B=1, device=backend.device, weights=S.calibrated_weights(OM.variable_shapes(), 1))
        blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
        bv = sum([OM.layer_variables()[n] for n in blocks[4]], [])
        builds = [lambda: eng.build_plan("NONE"), lambda: eng.build_plan("FULL", lr=1e-3),
                  lambda: eng.build_plan("MAD", lr=1e-3, block_vars=bv, block_level=E.LEVELS[4])]
    else:
        eng = DE.DispNetEngine(backend.lib, H, W, B=1, device=backend.device, weights=S.calibrated_weights(OD.variable_shapes(), 1))
        builds = [lambda: eng.build_plan("NONE"), lambda: eng.build_plan("FULL", lr=1e-3)]
    for build in builds:
        assert not eng.kitti_metrics
        off = _op_fields(build())
        eng.kitti_metrics = True
        plan = build()
        eng.kitti_metrics = False
        on = _op_fields(plan)
        kinds = [plan.arr[k].kind for k in range(plan.n)]
        assert _ffi.OP_METRICS_KITTI not in [f[0] for f in off]
        assert kinds.count(_ffi.OP_METRICS_KITTI) == 1
        at = kinds.index(_ffi.OP_METRICS_KITTI)
        assert kinds[at - 1] == _ffi.OP_METRICS and lane_of(plan.arr[at]) == lane_of(plan.arr[at - 1])
        assert on[:at] + on[at + 1:] == off


def _script_numbers(disp, gt):
    import Stereo_Continual_Adaptation as SCA
    return SCA.d1_and_epe(disp, gt)


@pytest.mark.gpu
@pytest.mark.parametrize("net,mode", [("MADNet", "MAD"), ("MADNet", "FULL"), ("Dispnet", "FULL")])
def test_adapter_returns_the_numbers_of_d1_and_epe(hip, net, mode):
    """Adapter(kitti_metrics=True).step: out['d1'] / out['epe_gt0'] are what the script's d1_and_epe computes from the returned disparity (captured graph, the report on
    the side lane in FULL mode); the keyword changes nothing else of the step"""
    import Nets
    from madnet_hip.adapter import Adapter
    H, W = 64, 128
    shapes = OM.variable_shapes() if net == "MADNet" else OD.variable_shapes()
    wn = S.calibrated_weights(shapes, 1)
    outs = {}
    for kitti in (False, True):
        frames = [S.make_pair(H, W, frame=t) for t in range(2)]
        l0, r0, _ = frames[0]
        nt = Nets.get_stereo_net(net, {"left_img": torch.from_numpy(l0).cuda(), "right_img": torch.from_numpy(r0).cuda(), "split_layers": [None], "sequence": True,
                                       "train_portion": "BEGIN", "bulkhead": mode == "MAD", "weights": wn, "precision": "mixed"})       # (the mode whose replays are bit-identical)
        cfg = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
        ad = Adapter(nt, mode=mode, block_config=cfg, lr=1e-3, sample_mode="SEQUENTIAL", ssim_th=1e9, kitti_metrics=kitti)
        res = []
        for l, r, gt in frames:
            tl, tr, tg = (torch.from_numpy(a).cuda() for a in (l, r, gt[..., 0]))
            out = ad.step(tl, tr, tg)
            if kitti:
                d1, epe = _script_numbers(out["disparity"][0], tg[0])
                print("%s %s: D1 %.6f (d1_and_epe %.6f)  EPE %.7f (%.7f)" % (net, mode, out["d1"], d1, out["epe_gt0"], epe))
                assert abs(out["d1"] - d1) <= 1e-4 * max(1.0, d1) and abs(out["epe_gt0"] - epe) <= 1e-6 * epe
                # the synthetic ground truth has no negative entry: EPE over gt > 0 is the step's own EPE over gt != 0
                assert abs(out["epe_gt0"] - out["epe"]) <= 1e-5 * out["epe"]
            else:
                assert "d1" not in out and "epe_gt0" not in out
            res.append((out["loss"], out["epe"], out["bad3"], out["disparity"].clone()))
        outs[kitti] = res
    for a, b in zip(outs[False], outs[True]):
        assert a[:3] == b[:3] and torch.equal(a[3], b[3])
