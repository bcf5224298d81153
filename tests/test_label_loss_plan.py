"""The label losses inside a plan: PROXY_LOSS / PROXY_LOSS_SCALED carry the loss in a named int slot (`loss`, the first free slot of each).  0 -- every record made
before the slot existed, and the packing fixture -- replays through mh_proxy_loss / mh_proxy_loss_scaled; another value through mh_label_loss / mh_label_loss_scaled
with the proxy rule (rule 0, hi 192).  There is no new op kind and no new Recorder method: the Recorder takes the value from its state attribute `label_loss`,
which the ops.proxy_loss(..., loss=) / ops.proxy_loss_scaled(..., loss=) wrappers set while they record."""
import ctypes as C

import pytest
import torch

import footprint as FP
from madnet_hip import _ffi, oplayout, ops
from madnet_hip import plan as PL
from test_label_loss import NAMES
from test_proxy_scaled import _op_data

B, H, W, S = 2, 37, 53, 2
_P = lambda t: C.c_void_p(t.data_ptr())


def _buffers(lib, dev, scaled):
    n = lib.proxy_scaled_ws_floats(B, H, W, S) if scaled else lib.proxy_ws_floats(B, H, W)
    return FP.Guarded(n, torch.float32, dev), FP.Guarded(2, torch.float32, dev), FP.Guarded(B * H * W, torch.float32, dev)


def _direct(lib, pd, xd, ws, res, dp, name, scaled):
    """the entry point a record with this loss must reach, called directly"""
    k = _ffi.LABEL_LOSS[name]
    if scaled:
        if k == 0:
            lib.proxy_loss_scaled(_P(pd), _P(xd), _P(ws.t), _P(res.t), _P(dp.t), 0.1, 0.75, S, B, H, W, None)
        else:
            lib.label_loss_scaled(_P(pd), _P(xd), _P(ws.t), _P(res.t), _P(dp.t), k, 0.1, 0.75, S, B, H, W, None)
    elif k == 0:
        lib.proxy_loss(_P(pd), _P(xd), _P(ws.t), _P(res.t), _P(dp.t), 0.1, 0.75, B, H, W, None)
    else:
        lib.label_loss(_P(pd), _P(xd), _P(ws.t), _P(res.t), _P(dp.t), k, 0, 192.0, 0.1, 0.75, B, H, W, None)


@pytest.mark.parametrize("scaled", [False, True], ids=["PROXY_LOSS", "PROXY_LOSS_SCALED"])
@pytest.mark.parametrize("name", NAMES)
def test_recorded_loss_replays_to_the_bits_of_the_direct_call(backend, name, scaled):
    lib, dev = backend.lib, backend.device
    pred, px = _op_data(B, H, W, S, 1)
    if not scaled:
        pred = pred * S                     # (at full size the prediction lives at the labels' own scale)
    pd, xd = pred.to(dev), px.to(dev)
    wd, rd, gd = _buffers(lib, dev, scaled)
    _direct(lib, pd, xd, wd, rd, gd, name, scaled)
    backend.sync()
    wp, rp, gp = _buffers(lib, dev, scaled)
    rec = PL.Recorder()
    if scaled:
        ops.proxy_loss_scaled(rec, pd, xd, wp.t, rp.t, S, gp.t, weight=0.1, grad_scale=0.75, loss=name)
    else:
        ops.proxy_loss(rec, pd, xd, wp.t, rp.t, gp.t, weight=0.1, grad_scale=0.75, loss=name)
    assert len(rec.ops) == 1 and rec.label_loss == 0                       # (the attribute is put back)
    op = rec.ops[0]
    assert op.kind == (_ffi.OP_PROXY_LOSS_SCALED if scaled else _ffi.OP_PROXY_LOSS)
    assert oplayout.fields(op).loss == _ffi.LABEL_LOSS[name] == op.i[4 if scaled else 3]
    rec.compile().run(lib, None)
    backend.sync()
    for a, b in ((wd, wp), (rd, rp), (gd, gp)):
        assert torch.equal(a.snapshot(), b.snapshot())                     # payload and guards, on bits
    assert torch.isfinite(rp.t).all() and torch.isfinite(gp.t).all()


def test_a_record_made_without_the_attribute_has_zero_in_the_slot():
    for method, kind, slot, args in (("proxy_loss", _ffi.OP_PROXY_LOSS, 3, (0.1, 1.0, B, H, W, None)),
                                     ("proxy_loss_scaled", _ffi.OP_PROXY_LOSS_SCALED, 4, (0.1, 1.0, S, B, H, W, None))):
        rec = PL.Recorder()
        assert rec.label_loss == 0
        getattr(rec, method)(0x10000, 0x20000, 0x30000, 0x40000, 0x50000, *args)
        op = rec.ops[0]
        assert op.kind == kind and oplayout.fields(op).loss == 0 and op.i[slot] == 0
        rec.label_loss = 5
        getattr(rec, method)(0x10000, 0x20000, 0x30000, 0x40000, 0x50000, *args)
        assert oplayout.fields(rec.ops[1]).loss == 5 and rec.ops[1].i[slot] == 5
        assert [v for k, v in enumerate(rec.ops[1].i) if k != slot] == [v for k, v in enumerate(op.i) if k != slot]        # nothing else moved
    assert "loss" not in oplayout.LAYOUT[_ffi.OP_SUPERVISED_LOSS].at                # the trainer's op is left alone


def test_the_wrappers_refuse_an_unknown_name():
    rec = PL.Recorder()
    t = torch.zeros(1, 2, 2)
    with pytest.raises(ValueError, match="unknown label loss"):
        ops.proxy_loss(rec, t, t, t, t, t, loss="ZNCC")
    with pytest.raises(ValueError, match="unknown label loss"):
        ops.proxy_loss_scaled(rec, t, t, t, t, 2, t, loss="huber")
    assert rec.ops == []
