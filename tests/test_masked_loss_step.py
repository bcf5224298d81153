"""The masked reprojection loss inside the adaptation step: the MH_LOSS_MASKED bit in the `phase` slot of the LOSS record (filled from the recorder's state
attribute `loss_masked` by ops.reprojection_loss(..., valid=)), the masks in the record's own workspace (ops.loss_set_valid), the engines' set_valid_masks,
Adapter(valid_masks=) / set_valid_masks and the live demo's --maskInvalid.  There is no new op kind, slot or Recorder method; without masks every plan is the
plan recorded before.

One step through the Adapter in the engines' exact-fp32 mode against the oracle step with oracle.tf_ops.reprojection_loss swapped, for the duration of the oracle
call, for masked_loss_oracle.step_loss: shapes, composition and bounds of tests/test_smoothness_step.py (test_engine_parity._check)."""
import json
import os
import sys

import pytest
import torch

import Nets
import footprint as FP
import masked_loss_oracle as MO
from madnet_hip import _ffi, oplayout, ops
from madnet_hip import plan as PL
from madnet_hip import synthetic as S
from madnet_hip.adapter import Adapter
from oracle import dispnet as OD
from oracle import madnet as OM
from oracle import tf_ops as T
from test_engine_parity import PKG, _backend, _check

BLOCK = 4


def _masks(H, W, rect=0, B=1):
    """a 4-pixel border band in both views plus one rectangle (rect picks where: two different mask pairs for the re-masking test)"""
    vl = torch.zeros(B, H, W, dtype=torch.uint8)
    vr = torch.zeros(B, H, W, dtype=torch.uint8)
    vl[:, 4:H - 4, 4:W - 4] = 1
    vr[:, 4:H - 4, 4:W - 4] = 1
    if rect == 0:
        vl[:, H // 3:H // 3 + H // 6, W // 2:W // 2 + W // 5] = 0
    else:
        vr[:, H // 2:H // 2 + H // 5, W // 4:W // 4 + W // 4] = 0
    return vl, vr


# ---- a. the record ------------------------------------------------------------------------------------------------------------------------------------------
RB, RH, RW, RGS = 2, 19, 37, 0.75


def _record_inputs():
    g = torch.Generator().manual_seed(11)
    left = torch.floor(torch.rand(RB, RH, RW, 3, generator=g) * 256)
    right = torch.floor(torch.rand(RB, RH, RW, 3, generator=g) * 256)
    disp = torch.rand(RB, RH, RW, generator=g) * 6 - 1
    return left, right, disp, _masks(RH, RW, 0, RB)


def test_recorder_attribute_puts_the_flag_into_the_phase_slot():
    rec = PL.Recorder()
    assert rec.loss_masked is False and oplayout.LOSS_MASKED == 4
    args = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0.5, 2, 9, 14)
    rec.reprojection_loss(*args, None)
    rec.reprojection_loss_phase(*args, 1, None)
    rec.loss_masked = True
    rec.reprojection_loss(*args, None)
    rec.reprojection_loss_phase(*args, 1, None)
    rec.reprojection_loss_phase(*args, 2, None)
    a0, a1, b0, b1, b2 = rec.ops
    assert [oplayout.fields(o).phase for o in rec.ops] == [0, 1, 4, 5, 6] and all(o.kind == _ffi.OP_LOSS for o in rec.ops)
    for a, b in ((a0, b0), (a1, b1)):           # all other words are as without it
        ia, ib = list(a.i), list(b.i)
        assert ia[:3] == ib[:3] and ia[4:] == ib[4:] and ib[3] == ia[3] | 4 and list(a.f) == list(b.f) and list(a.p) == list(b.p) and a.n == b.n
    assert [nm for _, nm in oplayout.LAYOUT[_ffi.OP_LOSS].i] == ["B", "H", "W", "phase"] and len(oplayout.LAYOUT[_ffi.OP_LOSS].p) == 6


@pytest.mark.parametrize("phases", [(0,), (1, 2)], ids=["phase0", "phase1+2"])
def test_replayed_record_gives_the_direct_call_s_bits(backend, phases):
    lib, dev = backend.lib, backend.device
    left, right, disp, (vl, vr) = _record_inputs()
    left, right, disp, vl, vr = (t.to(dev) for t in (left, right, disp, vl, vr))

    def bufs():
        ws = FP.Guarded(lib.loss_ws_floats(RB, RH, RW), torch.float32, dev)
        res = FP.Guarded(4, torch.float32, dev)
        dd = FP.Guarded(RB * RH * RW, torch.float32, dev)
        for g in (ws, res, dd):
            g.t.fill_(float("nan"))
        return ws, res, dd
    ws, res, dd = bufs()
    for ph in phases:
        ops.reprojection_loss(lib, left, right, disp, ws.t, res.t, dd.t.view(RB, RH, RW) if ph != 2 else None, grad_scale=RGS, phase=ph, valid=(vl, vr))
    ws2, res2, dd2 = bufs()
    ops.loss_set_valid(lib, ws2.t, vl, vr)
    rec = PL.Recorder()
    for ph in phases:
        ops.reprojection_loss(rec, left, right, disp, ws2.t, res2.t, dd2.t.view(RB, RH, RW) if ph != 2 else None, grad_scale=RGS, phase=ph, valid=(vl, vr))
    assert rec.loss_masked is False and [oplayout.fields(o).phase for o in rec.ops] == [ph | 4 for ph in phases]          # (the attribute is put back)
    rec.compile().run(lib, None)
    backend.sync()
    for g in (ws, res, dd, ws2, res2, dd2):
        g.assert_guards("masked LOSS record %r" % (phases,))
    assert torch.equal(FP.bits(res.t), FP.bits(res2.t)) and torch.equal(FP.bits(dd.t), FP.bits(dd2.t))
    assert torch.isfinite(res.t[:3]).all() and torch.isfinite(dd.t).all() and torch.isnan(res.t[3]).item()
    o = MO.evaluate(disp.cpu(), left.cpu(), right.cpu(), vl.cpu(), vr.cpu(), torch.float64)
    assert abs(res2.t[0].item() - o["loss"]) <= 2e-6 * max(1.0, abs(o["loss"])) and 0 < o["n1"] < RB * RH * RW
    # other bytes at the offset are another mask: the replay reads them, not the tensors the recording saw
    ops.loss_set_valid(lib, ws2.t, torch.ones_like(vl), torch.ones_like(vr))
    rec.compile().run(lib, None)
    backend.sync()
    ws3, res3, dd3 = bufs()
    for ph in phases:
        ops.reprojection_loss(lib, left, right, disp, ws3.t, res3.t, dd3.t.view(RB, RH, RW) if ph != 2 else None, grad_scale=RGS, phase=ph)
    backend.sync()
    assert torch.equal(FP.bits(res3.t[:3]), FP.bits(res2.t[:3])) and torch.equal(FP.bits(dd3.t), FP.bits(dd2.t)) and not torch.equal(FP.bits(dd.t), FP.bits(dd2.t))


def test_plan_refuses_phases_above_2(backend):
    lib, dev = backend.lib, backend.device
    left, right, disp, (vl, vr) = (t if isinstance(t, tuple) else t.to(dev) for t in _record_inputs())
    ws = torch.zeros(lib.loss_ws_floats(RB, RH, RW), device=dev)
    res = torch.full((4,), -7.0, device=dev)
    for ph in (3, 7, 8, 12):
        rec = PL.Recorder()
        rec.reprojection_loss_phase(ops._p(left), ops._p(right), ops._p(disp), ops._p(ws), ops._p(res), None, 1.0, RB, RH, RW, ph, None)
        with pytest.raises(_ffi.MadnetHipError):
            rec.compile().run(lib, None)
    backend.sync()
    assert bool((res == -7.0).all())
    with pytest.raises(_ffi.MadnetHipError):      # mh_reprojection_loss_phase keeps refusing the flag
        lib.reprojection_loss_phase(ops._p(left), ops._p(right), ops._p(disp), ops._p(ws), ops._p(res), None, 1.0, RB, RH, RW, 4, None)


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
def test_plans_without_masks_are_unchanged(mode):
    backend = _backend("emul")
    H, W = 60, 100
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    kw = dict(mode=mode, block_config=blocks if mode == "MAD" else None, sample_mode="FIXED", fixed_id=BLOCK, use_graph=False)
    key = "FULL" if mode == "FULL" else (BLOCK,)
    ads = [Adapter(_net(backend, "MADNet", H, W, wn, mode == "MAD"), **dict(kw, **extra)) for extra in ({}, {"valid_masks": None}, {"valid_masks": _masks(H, W)})]
    assert ads[0].eng.valid is None and ads[1].eng.valid is None and ads[2].eng.valid is not None
    r_default, r_none, r_m = (_rows(a._plan(key)[0]) for a in ads)
    assert r_default == r_none
    loss_at = [k for k, row in enumerate(r_default) if row[0] == _ffi.OP_LOSS]
    assert len(loss_at) >= 2 and len(r_m) == len(r_default)
    for k, (a, b) in enumerate(zip(r_default, r_m)):
        if k in loss_at:
            assert a[1][3] in (0, 1, 2) and b[1][3] == a[1][3] | 4 and a[1][:3] == b[1][:3] and a[1][4:] == b[1][4:] and a[0] == b[0] and a[2:] == b[2:]
        else:
            assert a == b
    # the first masks must come before the first plan
    with pytest.raises(RuntimeError, match="before the first"):
        ads[0].set_valid_masks(*_masks(H, W))


# ---- c. one step through the Adapter against the oracle step ---------------------------------------------------------------------------------------------------
def _swapped(vl, vr):
    def reprojection_loss(disp, left, right):
        assert tuple(disp.shape[1:3]) == tuple(vl.shape[1:3]) == tuple(left.shape[1:3])
        return MO.step_loss(disp, left, right, vl, vr)
    return reprojection_loss


def _loss_records(plan):
    return [plan.arr[k] for k in range(plan.n) if plan.arr[k].kind == _ffi.OP_LOSS]


STEP_CASES = [pytest.param(b, mode, id="%s-%s" % (b, mode), marks=[pytest.mark.gpu] if b == "hip" else []) for b in ("emul", "hip") for mode in ("FULL", "MAD")]


@pytest.mark.parametrize("bname,mode", STEP_CASES)
def test_madnet_step_with_masks(bname, mode, monkeypatch):
    backend = _backend(bname)
    H, W, lr = 60, 100, 1e-2
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a).double() for a in (l, r, gt))
    vl, vr = _masks(H, W)
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    net = _net(backend, "MADNet", H, W, wn, bulkhead=mode == "MAD")
    ad = Adapter(net, mode=mode, block_config=blocks if mode == "MAD" else None, lr=lr, sample_mode="FIXED", fixed_id=BLOCK, ssim_th=1e9, valid_masks=(vl, vr))
    eng = net.engine
    out = ad.step(l, r, gt[..., 0])
    backend.sync()
    recs = _loss_records(ad._plan("FULL" if mode == "FULL" else (BLOCK,))[0])
    assert len(recs) >= (1 if mode == "FULL" else 2) and all(oplayout.fields(o).phase & 4 for o in recs)
    wt = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    monkeypatch.setattr(T, "reprojection_loss", _swapped(vl, vr))
    if mode == "FULL":
        o = OM.step(wt, acc, tl, tr, tg, mode="FULL", lr=lr)
    else:
        bv = sum([OM.layer_variables()[n] for n in blocks[BLOCK]], [])
        o = OM.step(wt, acc, tl, tr, tg, mode="MAD", block_vars=bv, block_index=BLOCK, lr=lr)
    monkeypatch.undo()
    plain = T.reprojection_loss(o["disparity"], tl, tr).item()
    print("%s on %s: loss %.9g (oracle, masked %.9g; unmasked %.9g)" % (mode, bname, out["loss"], o["loss"], plain))
    assert abs(o["loss"] - plain) > 1e-3 * abs(plain)               # the step really ran another loss
    assert out["loss"] == eng.res_loss[0].item() and out["blocks"] == ([BLOCK] if mode == "MAD" else [])
    _check(eng, wn, wt, o, backend)


def _dispnet_step(backend, H, W):
    """test_dispnet_parity._run's criteria (as test_smoothness_step._dispnet_step) for one FULL step through the Adapter"""
    lr = 1e-3
    wn = S.calibrated_weights(OD.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a) for a in (l, r, gt))
    vl, vr = _masks(H, W)
    net = _net(backend, "Dispnet", H, W, wn, bulkhead=False)
    ad = Adapter(net, mode="FULL", lr=lr, ssim_th=1e9, valid_masks=(vl, vr))
    eng = net.engine
    out = ad.step(l, r, gt[..., 0])
    backend.sync()
    recs = _loss_records(ad._plan("FULL")[0])
    assert len(recs) >= 1 and all(oplayout.fields(o).phase & 4 for o in recs)
    wt = {k: torch.from_numpy(v.copy()) for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    w64 = {k: torch.from_numpy(v.copy()).double() for k, v in wn.items()}
    a64 = {k: torch.zeros_like(v) for k, v in w64.items()}
    old, T.reprojection_loss = T.reprojection_loss, _swapped(vl, vr)
    try:
        o = OD.step(wt, acc, tl, tr, tg, mode="FULL", lr=lr)
        o64 = OD.step(w64, a64, tl.double(), tr.double(), tg.double(), mode="FULL", lr=lr)
    finally:
        T.reprojection_loss = old
    d = o["disparity"][..., 0]
    plain = T.reprojection_loss(o["disparity"], tl, tr).item()
    print("DispNet %dx%d: loss %.9g (oracle %.9g, float64 %.9g; unmasked %.9g)" % (H, W, out["loss"], o["loss"], o64["loss"], plain))
    assert abs(o["loss"] - plain) > 1e-3 * abs(plain)
    assert d.abs().mean().item() > 0.5
    assert (eng.pred.cpu() - d).abs().mean().item() <= 1e-3
    assert abs(out["loss"] - o["loss"]) <= 2e-5 * max(1.0, abs(o["loss"]))
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
def test_dispnet_step_with_masks_emulated():
    _dispnet_step(_backend("emul"), 40, 64)


@pytest.mark.gpu
def test_dispnet_step_with_masks_gpu(hip):
    _dispnet_step(hip, 64, 128)


# ---- d. other masks under the captured graph --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_valid_masks_after_capture_is_a_fresh_adapter_s_loss(hip):
    """second step with other masks through the captured graph = the first step of a fresh adapter built with those masks, from the same weights and frames.  lr = 0
    keeps the weights of the first adapter where they were (momentum of a zero-scaled gradient moves nothing), so both read the same weights."""
    H, W = 60, 100
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    l, r, gt = S.make_pair(H, W)
    m0, m1 = _masks(H, W, 0), _masks(H, W, 1)
    ad = Adapter(_net(hip, "MADNet", H, W, wn, False), mode="FULL", lr=0.0, ssim_th=1e9, use_graph=True, valid_masks=m0)
    first = ad.step(l, r, gt[..., 0])
    assert torch.equal(ad.eng.params.w, ad.eng.params.w0)
    n_plans = len(ad._plans)
    ad.set_valid_masks(*m1)
    second = ad.step(l, r, gt[..., 0])
    assert len(ad._plans) == n_plans                       # no re-capture
    fresh = Adapter(_net(hip, "MADNet", H, W, wn, False), mode="FULL", lr=0.0, ssim_th=1e9, use_graph=True, valid_masks=m1).step(l, r, gt[..., 0])
    print("loss with masks 0: %.9g, re-masked: %.9g, fresh adapter: %.9g" % (first["loss"], second["loss"], fresh["loss"]))
    assert second["loss"] == fresh["loss"] and second["loss"] != first["loss"]


# ---- e. keyword errors --------------------------------------------------------------------------------------------------------------------------------------------
def test_adapter_keyword_errors(backend):
    wn = S.calibrated_weights(OM.variable_shapes(), 1)
    H, W = 64, 64
    net = _net(backend, "MADNet", H, W, wn, bulkhead=False)
    with pytest.raises(ValueError, match="valid_masks needs loss='reprojection'"):
        Adapter(net, mode="FULL", loss="proxy", valid_masks=_masks(H, W))
    with pytest.raises(NotImplementedError, match="reprojection_scale"):
        Adapter(net, mode="FULL", reprojection_scale=2, valid_masks=_masks(H, W))
    assert net.engine.valid is None and net.engine.loss_kind == "reprojection"          # a refused construction leaves the engine alone
    with pytest.raises(ValueError, match="uint8"):
        Adapter(net, mode="NONE", use_graph=False, valid_masks=tuple(m.float() for m in _masks(H, W)))
    ad = Adapter(_net(backend, "MADNet", H, W, wn, bulkhead=False), mode="NONE", use_graph=False, valid_masks=_masks(H, W))
    assert ad.eng.valid is not None and torch.equal(ad.eng.valid[0].cpu(), _masks(H, W)[0])


class _Reached(Exception):
    pass


def test_mask_invalid_flag_needs_a_calibration(monkeypatch):
    import queue
    sys.path.insert(0, os.path.join(PKG, "Demo"))
    import Live_Adaptation_Demo as LD
    import demo_model
    assert LD.build_parser().parse_args([]).maskInvalid is False

    def stereo(q, **kw):
        raise _Reached()
    monkeypatch.setattr(demo_model, "RealTimeStereo", stereo)
    with pytest.raises(SystemExit, match="--maskInvalid needs --calibration"):            # before any device work: the model is never built
        LD.main(LD.build_parser().parse_args(["--maskInvalid", "--mode", "FULL"]))
    monkeypatch.undo()
    monkeypatch.setattr(demo_model.RealTimeStereo, "_setup_graph", lambda self, shape: (_ for _ in ()).throw(_Reached()))
    with pytest.raises(ValueError, match="mask_invalid needs a calibration"):
        demo_model.RealTimeStereo(queue.Queue(1), image_shape=[64, 64], crop_shape=[-1], mode="FULL", device="cpu", mask_invalid=True)
