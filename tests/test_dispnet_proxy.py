"""DispNet under the continual-adaptation loss (Stereo_Continual_Adaptation.py:75, its default --modelName): full_proxy_loss = mean_l1 against the proxy labels,
weight 0.01, last prediction only -> the unchanged backward pass and momentum update.  Criteria of test_dispnet_parity._run; the oracle is
oracle.dispnet.forward -> proxy_loss(disps[-1], proxy, 0.01) -> autograd -> momentum_update."""
import numpy as np
import pytest
import torch

from madnet_hip import dispnet_engine as DE
from madnet_hip import synthetic as S
from oracle import dispnet as OD
from oracle import madnet as OM
from oracle import tf_ops as T
from test_engine_parity import _proxy_from


def _oracle_step(wt, acc, left, right, gt, proxy, mode, lr):
    names = list(wt.keys())
    for n in names:
        wt[n].requires_grad_(mode == "FULL")
    disps = OD.forward(wt, left, right)
    loss = T.proxy_loss(disps[-1], proxy, 0.01)
    epe, bad3 = T.validation_metrics(disps[-1].detach(), gt)
    grads = {}
    if mode == "FULL":
        gl = torch.autograd.grad(loss, [wt[n] for n in names], allow_unused=True)
        grads = {n: g.detach() for n, g in zip(names, gl) if g is not None}
    for n in names:
        wt[n].requires_grad_(False)
    if grads:
        OM.momentum_update(wt, acc, grads, lr)
    return {"loss": float(loss.detach()), "epe": float(epe), "bad3": float(bad3), "disparity": disps[-1].detach(), "grads": grads}


def _run(backend, H, W, mode):
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    px = _proxy_from(torch.from_numpy(gt))
    eng = DE.DispNetEngine(backend.lib, H, W, B=1, device=backend.device, weights=wn)
    eng.loss_kind = "proxy"
    eng.set_inputs(l, r, gt[..., 0], proxy=px)
    lr = 1e-3
    eng.build_plan(mode, lr=lr).run(backend.lib, 0)
    backend.sync()
    wt = {k: torch.from_numpy(v.copy()) for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    tl, tr, tg = torch.from_numpy(l), torch.from_numpy(r), torch.from_numpy(gt)
    o = _oracle_step(wt, acc, tl, tr, tg, px[..., None], mode, lr)
    d = o["disparity"][..., 0]
    assert d.abs().mean().item() > 0.5                       # non-degenerate prediction
    assert (eng.pred.cpu() - d).abs().mean().item() <= 1e-3
    print("DispNet proxy %s %dx%d: loss %.9g (oracle %.9g)" % (mode, H, W, eng.res_loss[0].item(), o["loss"]))
    assert abs(eng.res_loss[0].item() - o["loss"]) <= 2e-5 * max(1.0, abs(o["loss"]))
    assert eng.res_loss[1].item() == float(((px > 0) & (px < 192)).sum().item())
    assert abs(eng.res_met[0].item() - o["epe"]) <= 1e-4 * max(1.0, o["epe"])
    assert (mode == "FULL") == bool(o["grads"])
    bad = []
    for n, g in o["grads"].items():
        ge = eng.params.tensor(n, "g").cpu()
        rel = (ge - g).norm().item() / max(g.norm().item(), 1e-30)
        if rel > 2e-3:
            bad.append(n)
    if bad:      # (test_dispnet_parity._run: stragglers of the deep, cancellation-heavy layers are judged against fp64 with the fp32 oracle's own error as yardstick)
        w64 = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
        a64 = {k: torch.zeros_like(v) for k, v in w64.items()}
        o64 = _oracle_step(w64, a64, tl.double(), tr.double(), tg.double(), px[..., None].double(), mode, lr)
        for n in bad:
            g64 = o64["grads"][n]
            ours = (eng.params.tensor(n, "g").cpu().double() - g64).norm().item() / g64.norm().item()
            ref32 = (o["grads"][n].double() - g64).norm().item() / g64.norm().item()
            assert ours <= 3 * ref32 + 5e-4, (n, ours, ref32)
    for n in wt:
        assert (eng.params.tensor(n).cpu() - wt[n]).abs().max().item() <= 1e-5 * max(1.0, wt[n].abs().max().item()), n
    if mode == "NONE":
        assert all(torch.equal(eng.params.tensor(n).cpu(), torch.from_numpy(wn[n])) for n in wt)


@pytest.mark.slow
@pytest.mark.parametrize("mode", ["NONE", "FULL"])
def test_dispnet_proxy_step_emulated(mode):
    from conftest import _emul_backend
    _run(_emul_backend(), 40, 64, mode)          # pads to 64x64


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["NONE", "FULL"])
def test_dispnet_proxy_step_gpu(hip, mode):
    _run(hip, 64, 128, mode)


def test_dispnet_engine_rejects_an_unknown_loss_kind(backend):
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    eng = DE.DispNetEngine(backend.lib, 64, 64, B=1, device=backend.device, weights=wn)
    eng.loss_kind = "ssim"
    with pytest.raises(ValueError):
        eng.build_plan("NONE")


@pytest.mark.gpu
def test_dispnet_proxy_through_the_adapter(hip):
    """The public surface, as Stereo_Continual_Adaptation.py drives it with its default model: FULL, loss='proxy', dilation 2.  Frame 0 updates the weights;
    frame 1 is a NONE frame that still carries the proxy loss value and leaves the weights alone.  MAD keeps raising for DispNet."""
    import Nets
    from madnet_hip.adapter import Adapter
    H, W = 64, 128
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a).cuda() for a in (l, r, gt[..., 0]))
    px = _proxy_from(torch.from_numpy(gt)).cuda()
    net = Nets.get_stereo_net("Dispnet", {"left_img": tl, "right_img": tr, "split_layers": [None], "sequence": True,
                                          "train_portion": "BEGIN", "bulkhead": False, "weights": wn})
    ad = Adapter(net, mode="FULL", loss="proxy", dilation=2, lr=1e-3, ssim_th=1e9)
    eng = net.engine
    w0 = eng.params.w.clone()
    out0 = ad.step(tl, tr, tg, proxy=px)
    w1 = eng.params.w.clone()
    assert np.isfinite(out0["loss"]) and not torch.equal(w0, w1)
    # the loss IS the proxy loss of the returned disparity (pre-update weights), not the reprojection loss
    ref0 = T.proxy_loss(out0["disparity"].cpu()[..., None], px.cpu()[..., None], 0.01).item()
    assert abs(out0["loss"] - ref0) <= 2e-5 * max(1.0, abs(ref0))
    out1 = ad.step(tl, tr, tg, proxy=px)
    assert np.isfinite(out1["loss"]) and torch.equal(w1, eng.params.w)
    ref1 = T.proxy_loss(out1["disparity"].cpu()[..., None], px.cpu()[..., None], 0.01).item()
    assert abs(out1["loss"] - ref1) <= 2e-5 * max(1.0, abs(ref1))
    assert out1["loss"] != out0["loss"]                      # frame 1 ran on the updated weights
    with pytest.raises(ValueError):
        ad.step(tl, tr, tg)                                  # proxy labels are mandatory for loss='proxy'
    with pytest.raises(NotImplementedError):
        Adapter(net, mode="MAD", block_config=[[]] * 6, loss="proxy")
