"""The continual loop with another label loss on the proxy labels: Adapter(loss='proxy', proxy_loss=...) -> the engines' three recording sites (MADNet full-resolution
loss, weight 0.01; MADNet block losses, scaled and unscaled, weight 0.1; DispNet full loss) -> Stereo_Continual_Adaptation.py --proxyLoss.

One step through the Adapter in the engines' exact-fp32 mode against the oracle step with oracle.tf_ops.proxy_loss swapped, for the duration of the oracle call, for
the formula of tests/test_label_loss.py.  Shapes, oracle composition and bounds are those the mean_l1 proxy step has at the same shape: test_engine_parity._check
(FULL / MAD at 60 x 100), test_proxy_scaled._oracle_mad_proxy_scaled (MAD at reprojection scale 2), test_dispnet_proxy._run (DispNet at 64 x 128)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import Nets
from madnet_hip import _ffi, oplayout
from madnet_hip import synthetic as S
from madnet_hip.adapter import Adapter
from oracle import dispnet as OD
from oracle import madnet as OM
from oracle import tf_ops as T
from test_dispnet_proxy import _oracle_step as _dispnet_oracle_step
from test_engine_parity import PKG, _backend, _check, _proxy_from
from test_label_loss import formula
from test_proxy_scaled import _oracle_mad_proxy_scaled

LOSS = "mean_huber"
BLOCK = 4


def _swapped(name):
    """oracle.tf_ops.proxy_loss's signature and validity rule with the loss `name` in place of mean_l1"""
    def proxy_loss(pred, proxy, weight=0.01):
        valid = torch.where((proxy <= 0) | (proxy >= 192), torch.zeros_like(proxy), torch.ones_like(proxy))
        return formula(name, pred, proxy, valid, weight)
    return proxy_loss


def _net(backend, model, H, W, wn, bulkhead):
    z = torch.zeros(1, H, W, 3, device=backend.device)
    return Nets.get_stereo_net(model, {"left_img": z, "right_img": z, "split_layers": [None], "sequence": True, "train_portion": "BEGIN", "bulkhead": bulkhead,
                                       "weights": wn, "precision": "fp32", "_lib": backend.lib, "_device": backend.device})


MAD_CASES = [pytest.param(b, mode, s, id="%s-%s%s" % (b, mode, "-s%d" % s if s != 1 else ""), marks=[pytest.mark.gpu] if b == "hip" else [])
             for b in ("emul", "hip") for mode, s in (("FULL", 1), ("MAD", 1), ("MAD", 2))]


@pytest.mark.parametrize("bname,mode,scale", MAD_CASES)
def test_madnet_step_with_mean_huber(bname, mode, scale, monkeypatch):
    backend = _backend(bname)
    H, W, lr = 60, 100, 1e-2
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a) for a in (l, r, gt))
    px = _proxy_from(tg, 47 if scale != 1 else 3)                  # (47: the seed test_proxy_scaled found for this shape at scale 2)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    net = _net(backend, "MADNet", H, W, wn, bulkhead=mode == "MAD")
    ad = Adapter(net, mode=mode, block_config=blocks if mode == "MAD" else None, lr=lr, sample_mode="FIXED", fixed_id=BLOCK, ssim_th=1e9, reprojection_scale=scale,
                 loss="proxy", proxy_loss=LOSS)
    eng = net.engine
    assert eng.loss_kind == "proxy" and eng.proxy_loss == LOSS
    out = ad.step(l, r, gt[..., 0], proxy=px.numpy())
    backend.sync()
    # every proxy-loss record of the step carries the loss in its slot
    plan = ad._plan("FULL" if mode == "FULL" else (BLOCK,))[0]
    recs = [plan.arr[k] for k in range(plan.n) if plan.arr[k].kind in (_ffi.OP_PROXY_LOSS, _ffi.OP_PROXY_LOSS_SCALED)]
    assert [oplayout.fields(o).loss for o in recs] == [_ffi.LABEL_LOSS[LOSS]] * (1 if mode == "FULL" else 2)
    assert [o.kind for o in recs].count(_ffi.OP_PROXY_LOSS_SCALED) == (1 if scale != 1 else 0)
    # the oracle step in float64
    wt = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    tl, tr, tg, px = tl.double(), tr.double(), tg.double(), px.double()
    monkeypatch.setattr(T, "proxy_loss", _swapped(LOSS))
    if mode == "FULL":
        o = OM.step(wt, acc, tl, tr, tg, mode="FULL", lr=lr, loss="proxy", proxy=px[..., None])
    else:
        bv = sum([OM.layer_variables()[n] for n in blocks[BLOCK]], [])
        if scale == 1:
            o = OM.step(wt, acc, tl, tr, tg, mode="MAD", block_vars=bv, block_index=BLOCK, lr=lr, loss="proxy", proxy=px[..., None])
        else:
            o = _oracle_mad_proxy_scaled(wt, acc, tl, tr, tg, px, bv, BLOCK, lr, scale)
    monkeypatch.undo()
    mean_l1 = T.proxy_loss(o["disparity"], px[..., None], 0.01).item()
    print("%s scale %d: %s %.9g (oracle %.9g; mean_l1 of the same prediction %.9g)" % (mode, scale, LOSS, out["loss"], o["loss"], mean_l1))
    assert abs(o["loss"] - mean_l1) > 1e-3 * abs(mean_l1)           # the step really ran another loss
    assert out["loss"] == eng.res_loss[0].item() and out["blocks"] == ([BLOCK] if mode == "MAD" else [])
    _check(eng, wn, wt, o, backend)


def _dispnet_step(backend, H, W):
    """test_dispnet_proxy._run's criteria for one FULL step through the Adapter"""
    lr = 1e-3
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a) for a in (l, r, gt))
    px = _proxy_from(tg)
    net = _net(backend, "Dispnet", H, W, wn, bulkhead=False)
    ad = Adapter(net, mode="FULL", lr=lr, ssim_th=1e9, loss="proxy", proxy_loss=LOSS)
    eng = net.engine
    out = ad.step(l, r, gt[..., 0], proxy=px.numpy())
    backend.sync()
    wt = {k: torch.from_numpy(v.copy()) for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    w64 = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    a64 = {k: torch.zeros_like(v) for k, v in w64.items()}
    old, T.proxy_loss = T.proxy_loss, _swapped(LOSS)
    try:
        o = _dispnet_oracle_step(wt, acc, tl, tr, tg, px[..., None], "FULL", lr)
        o64 = _dispnet_oracle_step(w64, a64, tl.double(), tr.double(), tg.double(), px[..., None].double(), "FULL", lr)
    finally:
        T.proxy_loss = old
    d = o["disparity"][..., 0]
    assert d.abs().mean().item() > 0.5
    assert (eng.pred.cpu() - d).abs().mean().item() <= 1e-3
    print("DispNet %s %dx%d: loss %.9g (oracle %.9g, float64 %.9g)" % (LOSS, H, W, out["loss"], o["loss"], o64["loss"]))
    assert abs(out["loss"] - o["loss"]) <= 2e-5 * max(1.0, abs(o["loss"]))
    assert eng.res_loss[1].item() == float(((px > 0) & (px < 192)).sum().item())
    assert abs(eng.res_met[0].item() - o["epe"]) <= 1e-4 * max(1.0, o["epe"])
    for n, g in o["grads"].items():
        ge = eng.params.tensor(n, "g").cpu()
        rel = (ge - g).norm().item() / max(g.norm().item(), 1e-30)
        if rel > 2e-3:          # (stragglers of the deep, cancellation-heavy layers: against float64 with the fp32 oracle's own error as yardstick)
            g64 = o64["grads"][n]
            ours = (ge.double() - g64).norm().item() / g64.norm().item()
            ref32 = (g.double() - g64).norm().item() / g64.norm().item()
            assert ours <= 3 * ref32 + 5e-4, (n, ours, ref32)
    for n in wt:
        assert (eng.params.tensor(n).cpu() - wt[n]).abs().max().item() <= 1e-5 * max(1.0, wt[n].abs().max().item()), n


@pytest.mark.slow
def test_dispnet_step_with_mean_huber_emulated():
    _dispnet_step(_backend("emul"), 40, 64)          # pads to 64 x 64, as test_dispnet_proxy's emulated step


@pytest.mark.gpu
def test_dispnet_step_with_mean_huber_gpu(hip):
    _dispnet_step(hip, 64, 128)


def test_adapter_refuses_bad_proxy_loss_arguments(backend):
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    net = _net(backend, "MADNet", 64, 64, wn, bulkhead=False)
    with pytest.raises(ValueError, match="proxy_loss must be one of"):
        Adapter(net, mode="FULL", loss="proxy", proxy_loss="ZNCC")
    with pytest.raises(ValueError, match="proxy_loss needs loss='proxy'"):
        Adapter(net, mode="FULL", proxy_loss="sum_huber")
    assert net.engine.proxy_loss == "mean_l1" and net.engine.loss_kind == "reprojection"       # a refused construction leaves the engine alone
    for name in _ffi.LABEL_LOSS:
        assert Adapter(net, mode="NONE", loss="proxy", proxy_loss=name, use_graph=False).eng.proxy_loss == name


def test_script_flag_and_factory_names():
    import Stereo_Continual_Adaptation as SCA
    from Losses import loss_factory as LF
    base = ["-l", "x", "-o", "y", "--weights", "z", "--blockConfig", "c"]
    assert SCA.build_parser().parse_args(base).proxyLoss == "mean_l1"
    for name in _ffi.LABEL_LOSS:
        assert SCA.build_parser().parse_args(base + ["--proxyLoss", name]).proxyLoss == name
    with pytest.raises(SystemExit):
        SCA.build_parser().parse_args(base + ["--proxyLoss", "ZNCC"])
    with pytest.raises(Exception, match="Unknown loss function selected"):
        LF.get_proxy_loss("ZNCC")


@pytest.mark.gpu
def test_continual_script_with_sum_huber_on_sgm_labels(hip, tmp_path):
    """Stereo_Continual_Adaptation.py --proxies sgm --proxyLoss sum_huber as a child process under its own time limit, on the list tests/test_continual_sgm_gpu.py
    writes: exits 0, the report and every row of the series are finite"""
    from test_continual_sgm_gpu import H, W, _make_list
    lst = _make_list(tmp_path, 3, proxy_column=False)
    out = tmp_path / "out"
    os.makedirs(out / "disparities"); os.makedirs(out / "weights")
    cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.join(PKG, "Stereo_Continual_Adaptation.py"), "-l", lst, "-o", str(out), "--weights", "calibrated:1",
           "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"), "--imageShape", str(H), str(W), "--SSIMTh", "1e9", "--mode", "MAD", "--modelName", "MADNet",
           "--sampleMode", "SEQUENTIAL", "--proxies", "sgm", "--proxyLoss", "sum_huber"]
    rc = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-3000:]
    overall = open(out / "overall.csv").read().split("\n")
    assert overall[0] == "EPE\tD1" and all(np.isfinite(float(v)) for v in overall[1].split("\t"))
    series = open(out / "series.csv").read().strip().split("\n")
    assert len(series) == 4 and all(np.isfinite(float(v)) for row in series[1:] for v in row.split(" & "))
