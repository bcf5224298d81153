"""The edge-aware smoothness term inside the adaptation step: the LOSS record's float slot `smooth_weight` (filled from the recorder's state attribute
`smoothness` by ops.reprojection_loss(..., smoothness=)), the engines' recording sites, Adapter(smoothness=), the scripts' --smoothness and
Losses.loss_factory.smoothness.  There is no new op kind and no new Recorder method; at weight 0 -- the default -- every plan is the plan recorded before.

One step through the Adapter in the engines' exact-fp32 mode against the oracle step with oracle.tf_ops.reprojection_loss swapped, for the duration of the oracle
call, for reprojection + w * S(disp, left) (smoothness_oracle.smoothness): shapes, oracle composition and bounds of tests/test_continual_proxy_loss.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import Nets
import footprint as FP
import smoothness_oracle as SO
from madnet_hip import _ffi, oplayout, ops
from madnet_hip import plan as PL
from madnet_hip import synthetic as S
from madnet_hip.adapter import Adapter
from oracle import dispnet as OD
from oracle import madnet as OM
from oracle import tf_ops as T
from test_engine_parity import PKG, _backend, _check

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_smoothness.npz")
WEIGHT = 50.0           # large enough that the step's loss is another loss (asserted), small enough that the reset threshold of the tests (1e9) is far
BLOCK = 4


# ---- a. the record ------------------------------------------------------------------------------------------------------------------------------------------
RB, RH, RW, RWEIGHT, RGS = 2, 9, 14, 0.37, 0.75
_rec = {}


def _record_case():
    """seeded frames and a disparity in (-1, 5) whose smoothness signs are decided in any arithmetic, with the float64 / float32 oracles of both terms; made once"""
    if not _rec:
        for seed in range(1, 40):
            g = torch.Generator().manual_seed(1000 * seed + RB + RH + RW)
            disp = torch.rand((RB, RH, RW), generator=g) * 6.0 - 1.0
            ramp = 30.0 + 170.0 * torch.arange(RW, dtype=torch.float32) / (RW - 1)
            left = ramp.view(1, 1, RW, 1) + 40.0 * torch.rand((RB, RH, RW, 3), generator=g)
            right = ramp.view(1, 1, RW, 1) + 40.0 * torch.rand((RB, RH, RW, 3), generator=g)
            s, gs, gmin = SO.restate(disp, left)
            if gmin >= 1e-3:
                break
        else:
            raise AssertionError("no unambiguous seed")

        def reproj(dtype):
            d = disp.to(dtype).requires_grad_(True)
            loss = T.reprojection_loss(d[..., None], left.to(dtype), right.to(dtype))
            return loss.item(), torch.autograd.grad(loss, [d])[0].detach()
        l64, g64 = reproj(torch.float64)
        _, g32 = reproj(torch.float32)
        _rec.update(disp=disp, left=left, right=right, s=s.item(), gs=gs, l64=l64, g64=g64, e32=(g32.double() - g64).abs().max().item())
    return _rec


def _replay(backend, weight, phases):
    """LOSS records of the given phases, in turn, into a loss workspace of exactly mh_loss_ws_floats floats behind a guard -> (result [4], ddisp) on the CPU"""
    lib, dev = backend.lib, backend.device
    c = _record_case()
    ws = FP.Guarded(lib.loss_ws_floats(RB, RH, RW), torch.float32, dev)
    res = FP.Guarded(4, torch.float32, dev)
    dd = FP.Guarded(RB * RH * RW, torch.float32, dev)
    for g in (ws, res, dd):
        g.t.fill_(float("nan"))
    rec = PL.Recorder()
    for ph in phases:
        ops.reprojection_loss(rec, c["left"].to(dev), c["right"].to(dev), c["disp"].to(dev), ws.t, res.t, dd.t.view(RB, RH, RW) if ph != 2 else None,
                              grad_scale=RGS, phase=ph, smoothness=weight)
    assert rec.smoothness == 0.0 and len(rec.ops) == len(phases)                   # (the attribute is put back)
    for op, ph in zip(rec.ops, phases):
        f = oplayout.fields(op)
        assert op.kind == _ffi.OP_LOSS and f.phase == ph and f.smooth_weight == np.float32(weight) == op.f[1] and f.grad_scale == RGS
    rec.compile().run(lib, None)
    backend.sync()
    for g in (ws, res, dd):
        g.assert_guards("LOSS record, weight %g, phases %r" % (weight, phases))
    return res.t.cpu().clone(), dd.t.cpu().view(RB, RH, RW).clone(), (ws, res, dd)


@pytest.mark.parametrize("phases", [(0,), (1, 2)], ids=["phase0", "phase1+2"])
def test_loss_record_with_a_smoothness_weight(backend, phases):
    lib, dev = backend.lib, backend.device
    c = _record_case()
    r0, d0, _ = _replay(backend, 0.0, phases)
    assert torch.isnan(r0[3]).item()                                               # weight 0: nothing is launched, result[3] is not touched
    rw, dw, (ws, res, dd) = _replay(backend, RWEIGHT, phases)
    # values: float64 oracles of both terms
    ref_s = RWEIGHT * c["s"]
    print("LOSS record %r: loss %.9g (oracle %.9g + %.9g)  smoothness %.9g" % (phases, rw[0].item(), c["l64"], ref_s, rw[3].item()))
    assert abs(rw[3].item() - ref_s) <= 2e-6 * ref_s
    assert abs(rw[0].item() - (c["l64"] + ref_s)) <= 2e-6 * max(1.0, abs(c["l64"] + ref_s))
    assert rw[0].item() == (r0[0] + rw[3]).item()                                  # one float32 addition to the reprojection loss
    # the reprojection loss's own partial sums were not trampled
    assert torch.equal(FP.bits(rw[1:3]), FP.bits(r0[1:3])) and torch.isfinite(rw).all()
    # gradient: the sum of both, each within its own test's bound (tests/test_loss_tiles.py: 8 E32 + 1e-12; tests/test_smoothness_loss.py: 1e-5 max|g|)
    gsm = RGS * RWEIGHT * c["gs"]
    err = (dw.double() - RGS * c["g64"] - gsm).abs().max().item()
    print("   max|ddisp err| %.3g  (E32 %.3g, max|g smooth| %.3g, max|g reprojection| %.3g)" % (err, c["e32"], gsm.abs().max().item(), c["g64"].abs().max().item()))
    assert torch.isfinite(dw).all() and err <= RGS * (8 * c["e32"] + 1e-12) + 1e-5 * gsm.abs().max().item()
    assert (gsm.abs().max().item() > 100 * err) and not torch.equal(d0, dw)
    # ... and the reprojection loss's share of it is the weight-0 record's, on bits: the direct call on top of that record's gradient gives this record's
    g0 = FP.Guarded(RB * RH * RW, torch.float32, dev).set(d0)
    w2 = FP.Guarded(lib.smoothness_ws_floats(RB, RH, RW), torch.float32, dev)
    r2 = FP.Guarded(4, torch.float32, dev).set(r0)
    ops.smoothness_loss(lib, c["disp"].to(dev), c["left"].to(dev), w2.t, r2.t, g0.t.view(RB, RH, RW), weight=RWEIGHT, grad_scale=RGS, accumulate=True)
    backend.sync()
    assert torch.equal(g0.snapshot(), dd.snapshot()) and torch.equal(FP.bits(r2.t[[0, 3]]), FP.bits(rw[[0, 3]]))
    # the term's partial sums sit in the first floats of the loss workspace, the loss's own behind the retired maps
    n = lib.smoothness_ws_floats(RB, RH, RW)
    assert torch.equal(FP.bits(ws.t[:n]), FP.bits(w2.t)) and torch.isnan(ws.t[n:lib.loss_ws_floats(RB, RH, RW) - 2 * n]).all()


def test_a_record_made_without_the_attribute_has_zero_in_the_slot():
    rec = PL.Recorder()
    assert rec.smoothness == 0.0
    args = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0.5, 2, 9, 14)
    rec.reprojection_loss(*args, None)
    rec.reprojection_loss_phase(*args, 1, None)
    rec.smoothness = 0.37
    rec.reprojection_loss_phase(*args, 1, None)
    a, b, c = rec.ops
    assert a.f[1] == 0.0 and b.f[1] == 0.0 and oplayout.fields(b).smooth_weight == 0.0
    assert oplayout.fields(c).smooth_weight == np.float32(0.37) == c.f[1]
    assert bytes(b)[:] != bytes(c)[:] and list(b.i) == list(c.i) and list(b.p) == list(c.p) and b.f[0] == c.f[0] and list(b.f[2:]) == list(c.f[2:])     # nothing else moved
    assert oplayout.LAYOUT[_ffi.OP_LOSS].f == [(0, "grad_scale"), (1, "smooth_weight")]
    assert [nm for _, nm in oplayout.LAYOUT[_ffi.OP_LOSS].i] == ["B", "H", "W", "phase"] and len(oplayout.LAYOUT[_ffi.OP_LOSS].p) == 6


# ---- b. the default plans are the plans recorded before -------------------------------------------------------------------------------------------------------
def _net(backend, model, H, W, wn, bulkhead):
    z = torch.zeros(1, H, W, 3, device=backend.device)
    return Nets.get_stereo_net(model, {"left_img": z, "right_img": z, "split_layers": [None], "sequence": True, "train_portion": "BEGIN", "bulkhead": bulkhead,
                                       "weights": wn, "precision": "fp32", "_lib": backend.lib, "_device": backend.device})


def _rows(plan):
    """every record of a plan, pointers replaced by their rank of first appearance (two engines own different buffers)"""
    rank = {}
    rk = lambda q: -1 if not q else rank.setdefault(int(q), len(rank))
    return [(o.kind, tuple(o.i), tuple(FP.bits(torch.tensor(list(o.f))).tolist()), tuple(rk(q) for q in o.p), int(o.n)) for o in (plan.arr[k] for k in range(plan.n))]


@pytest.mark.parametrize("mode", ["FULL", "MAD"])
def test_default_plans_are_unchanged(mode):
    backend = _backend("emul")
    H, W = 60, 100
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    kw = dict(mode=mode, block_config=blocks if mode == "MAD" else None, sample_mode="FIXED", fixed_id=BLOCK, use_graph=False)
    key = "FULL" if mode == "FULL" else (BLOCK,)
    plans = [Adapter(_net(backend, "MADNet", H, W, wn, mode == "MAD"), **dict(kw, **extra))._plan(key)[0] for extra in ({}, {"smoothness": 0.0}, {"smoothness": 0.37})]
    r_default, r_zero, r_w = (_rows(p) for p in plans)
    assert r_default == r_zero
    loss_at = [k for k, row in enumerate(r_default) if row[0] == _ffi.OP_LOSS]
    assert len(loss_at) >= 2 and len(r_w) == len(r_default)
    for k, (a, b) in enumerate(zip(r_default, r_w)):
        if k in loss_at:
            assert a[2][1] == 0 and b[2][1] == FP.bits(torch.tensor([0.37])).item() and a[:2] == b[:2] and a[3:] == b[3:] and a[2][0] == b[2][0]
        else:
            assert a == b


# ---- c. one step through the Adapter against the oracle step ---------------------------------------------------------------------------------------------------
def _swapped(w):
    """oracle.tf_ops.reprojection_loss's signature with w * smoothness(disp, left) added"""
    plain = T.reprojection_loss

    def reprojection_loss(disp, left, right):
        return plain(disp, left, right) + w * SO.smoothness(disp[..., 0], left.to(disp.dtype))
    return reprojection_loss


def _loss_records(plan):
    return [plan.arr[k] for k in range(plan.n) if plan.arr[k].kind == _ffi.OP_LOSS]


MAD_CASES = [pytest.param(b, mode, s, id="%s-%s%s" % (b, mode, "-s%d" % s if s != 1 else ""), marks=[pytest.mark.gpu] if b == "hip" else [])
             for b in ("emul", "hip") for mode, s in (("FULL", 1), ("MAD", 1), ("MAD", 2))]


@pytest.mark.parametrize("bname,mode,scale", MAD_CASES)
def test_madnet_step_with_smoothness(bname, mode, scale, monkeypatch):
    backend = _backend(bname)
    H, W, lr = 60, 100, 1e-2
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a) for a in (l, r, gt))
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    net = _net(backend, "MADNet", H, W, wn, bulkhead=mode == "MAD")
    ad = Adapter(net, mode=mode, block_config=blocks if mode == "MAD" else None, lr=lr, sample_mode="FIXED", fixed_id=BLOCK, ssim_th=1e9, reprojection_scale=scale,
                 smoothness=WEIGHT)
    eng = net.engine
    assert eng.smoothness == WEIGHT and eng.loss_kind == "reprojection"
    out = ad.step(l, r, gt[..., 0])
    backend.sync()
    # every LOSS record of the step carries the weight
    recs = _loss_records(ad._plan("FULL" if mode == "FULL" else (BLOCK,))[0])
    assert len(recs) >= (1 if mode == "FULL" else 2) and [oplayout.fields(o).smooth_weight for o in recs] == [WEIGHT] * len(recs)
    # the oracle step in float64
    wt = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    tl, tr, tg = tl.double(), tr.double(), tg.double()
    monkeypatch.setattr(T, "reprojection_loss", _swapped(WEIGHT))
    if mode == "FULL":
        o = OM.step(wt, acc, tl, tr, tg, mode="FULL", lr=lr)
    else:
        bv = sum([OM.layer_variables()[n] for n in blocks[BLOCK]], [])
        o = OM.step(wt, acc, tl, tr, tg, mode="MAD", block_vars=bv, block_index=BLOCK, lr=lr, reprojection_scale=scale)
    monkeypatch.undo()
    plain = T.reprojection_loss(o["disparity"], tl, tr).item()
    smooth = WEIGHT * SO.smoothness(o["disparity"][..., 0], tl).item()
    print("%s scale %d: loss %.9g (oracle %.9g = reprojection %.9g + smoothness %.9g); out['smoothness'] %.9g" % (mode, scale, out["loss"], o["loss"], plain, smooth, out["smoothness"]))
    assert abs(o["loss"] - plain) > 1e-3 * abs(plain)               # the step really ran another loss
    assert out["loss"] == eng.res_loss[0].item() and out["smoothness"] == eng.res_loss[3].item() and out["blocks"] == ([BLOCK] if mode == "MAD" else [])
    assert abs(out["smoothness"] - smooth) <= 2e-5 * max(1.0, smooth)
    _check(eng, wn, wt, o, backend)


def _dispnet_step(backend, H, W):
    """test_dispnet_parity._run's criteria for one FULL step through the Adapter"""
    lr = 1e-3
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a) for a in (l, r, gt))
    net = _net(backend, "Dispnet", H, W, wn, bulkhead=False)
    ad = Adapter(net, mode="FULL", lr=lr, ssim_th=1e9, smoothness=WEIGHT)
    eng = net.engine
    out = ad.step(l, r, gt[..., 0])
    backend.sync()
    recs = _loss_records(ad._plan("FULL")[0])
    assert len(recs) >= 1 and [oplayout.fields(o).smooth_weight for o in recs] == [WEIGHT] * len(recs)
    wt = {k: torch.from_numpy(v.copy()) for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    w64 = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    a64 = {k: torch.zeros_like(v) for k, v in w64.items()}
    old, T.reprojection_loss = T.reprojection_loss, _swapped(WEIGHT)
    try:
        o = OD.step(wt, acc, tl, tr, tg, mode="FULL", lr=lr)
        o64 = OD.step(w64, a64, tl.double(), tr.double(), tg.double(), mode="FULL", lr=lr)
    finally:
        T.reprojection_loss = old
    d = o["disparity"][..., 0]
    plain = T.reprojection_loss(o["disparity"], tl, tr).item()
    print("DispNet %dx%d: loss %.9g (oracle %.9g, float64 %.9g; reprojection alone %.9g); out['smoothness'] %.9g" % (H, W, out["loss"], o["loss"], o64["loss"], plain, out["smoothness"]))
    assert abs(o["loss"] - plain) > 1e-3 * abs(plain)
    assert d.abs().mean().item() > 0.5
    assert (eng.pred.cpu() - d).abs().mean().item() <= 1e-3
    assert abs(out["loss"] - o["loss"]) <= 2e-5 * max(1.0, abs(o["loss"]))
    assert out["smoothness"] == eng.res_loss[3].item() and abs(out["smoothness"] - (o["loss"] - plain)) <= 2e-5 * max(1.0, abs(o["loss"]))
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
def test_dispnet_step_with_smoothness_emulated():
    _dispnet_step(_backend("emul"), 40, 64)          # pads to 64 x 64, as test_dispnet_proxy's emulated step


@pytest.mark.gpu
def test_dispnet_step_with_smoothness_gpu(hip):
    _dispnet_step(hip, 64, 128)


def test_adapter_refuses_smoothness_on_proxy_labels(backend):
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    net = _net(backend, "MADNet", 64, 64, wn, bulkhead=False)
    with pytest.raises(ValueError, match="smoothness needs loss='reprojection'"):
        Adapter(net, mode="FULL", loss="proxy", smoothness=0.5)
    assert net.engine.smoothness == 0.0 and net.engine.loss_kind == "reprojection"          # a refused construction leaves the engine alone
    assert Adapter(net, mode="NONE", loss="proxy", smoothness=0.0, use_graph=False).eng.smoothness == 0.0
    net = _net(backend, "MADNet", 64, 64, wn, bulkhead=False)
    assert Adapter(net, mode="NONE", smoothness=0.25, use_graph=False).eng.smoothness == 0.25


# ---- d. CPU only: the factory function and the scripts' flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c3", "c1"])
def test_loss_factory_smoothness_equals_the_reference(tag, monkeypatch):
    from Losses import loss_factory as LF
    monkeypatch.setattr(LF, "_lib", lambda: _backend("emul").lib)
    z = np.load(GOLD)
    x = torch.from_numpy(z["disp"]).requires_grad_(True)
    loss = LF.smoothness(x, torch.from_numpy(z["image" + tag[1]]))
    (g,) = torch.autograd.grad(3.0 * loss, [x])
    gref = torch.from_numpy(z["grad_" + tag]).double()
    assert loss.dim() == 0 and g.shape == x.shape
    assert abs(loss.item() - float(z["loss_" + tag])) <= 2e-6 * float(z["loss_" + tag])
    assert (g.double() / 3.0 - gref).abs().max().item() <= 1e-5 * gref.abs().max().item()
    with pytest.raises(Exception, match="Unknown loss function selected"):          # the builders' tables stay as they are
        LF.get_reprojection_loss("smoothness")


class _Reached(Exception):
    pass


def test_online_script_flag_reaches_the_adapter(monkeypatch, tmp_path):
    import Stereo_Online_Adaptation as SOA
    from madnet_hip import adapter as A
    base = ["-l", "x", "-o", str(tmp_path), "--weights", "calibrated:1", "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"), "--modelName", "MADNet"]
    assert SOA.build_parser().parse_args(base).smoothness == 0.0
    args = SOA.build_parser().parse_args(base + ["--smoothness", "0.125"])
    assert args.smoothness == 0.125
    seen = {}

    class Net(object):
        engine = None

        def get_disparities(self):
            return []

    def adapter(net, **kw):
        seen.update(kw)
        raise _Reached()
    monkeypatch.setattr(SOA.data_reader, "dataset", lambda *a, **k: None)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: None)
    monkeypatch.setattr(SOA, "load_weights", lambda *a, **k: None)
    monkeypatch.setattr(SOA.Nets, "get_stereo_net", lambda name, a: Net())
    monkeypatch.setattr(A, "Adapter", adapter)
    with pytest.raises(_Reached):
        SOA.main(args)
    assert seen["smoothness"] == 0.125 and seen["mode"] == "MAD"


def test_live_demo_flag_reaches_the_adapter(monkeypatch):
    import queue
    import sys
    sys.path.insert(0, os.path.join(PKG, "Demo"))
    import Live_Adaptation_Demo as LD
    import demo_model
    assert LD.build_parser().parse_args([]).smoothness == 0.0
    args = LD.build_parser().parse_args(["--smoothness", "0.125", "--mode", "FULL"])
    seen = {}

    def stereo(q, **kw):
        seen.update(kw)
        raise _Reached()
    monkeypatch.setattr(demo_model, "RealTimeStereo", stereo)
    with pytest.raises(_Reached):
        LD.main(args)
    assert seen["smoothness"] == 0.125
    monkeypatch.undo()
    # ... and from the demo's model to the Adapter
    seen.clear()

    def adapter(net, **kw):
        seen.update(kw)
        raise _Reached()
    monkeypatch.setattr(demo_model.RealTimeStereo, "_initial_weights", lambda self: None)
    monkeypatch.setattr(demo_model.Nets, "get_stereo_net", lambda name, a: object())
    monkeypatch.setattr(demo_model, "Adapter", adapter)
    dd = demo_model.RealTimeStereo(queue.Queue(1), image_shape=[-1], crop_shape=[-1], mode="FULL", device="cpu", smoothness=0.125)
    with pytest.raises(_Reached):
        dd._setup_graph((64, 64))
    assert seen["smoothness"] == 0.125
