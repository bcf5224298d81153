"""MadNetEngine packs a fragment bank exactly where a recorded launch reads one: the engine's bank plan (engine._bank_plan) against the library's own
answers -- mh_conv2d_takes_bank on the recorded descriptors, mh_last_kernel() on a replay.  Plans are only recorded, except for the one step of the last
test."""
import ctypes as C
import json
import os

import pytest
import torch

from madnet_hip import _ffi, oplayout, engine as E
from madnet_hip import synthetic as S
from madnet_hip.oplayout import fields
from oracle import madnet as OM

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real-time-self-adaptive-deep-stereo_amd")
BACKENDS = [pytest.param("emul", id="emul"), pytest.param("hip", marks=pytest.mark.gpu, id="hip")]
FORWARD, DGRAD = ("banks", "banks32"), ("banks_d", "banks32t")


def _backend(name):
    from conftest import _emul_backend, _hip_backend
    return _emul_backend() if name == "emul" else _hip_backend()


def _mad_plan(eng, level=4):
    blocks = json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json")))
    lv = OM.layer_variables()
    return eng.build_plan("MAD", lr=1e-4, block_vars=sum([lv[n] for n in blocks[E.LEVELS.index(level)]], []), block_level=level)


def _ops(plan):
    return [plan.arr[k] for k in range(plan.n)]


def _takes_bank(lib, op):
    """the library's answer for a recorded OP_CONV, on its own descriptor and pointers"""
    d, f = oplayout.conv_desc(op), fields(op)
    return lib.conv2d_takes_bank(C.byref(d), C.c_void_p(f.inp), C.c_void_p(f.w), C.c_void_p(f.out), C.c_void_p(f.mask))


def _banks_read(plan):
    """pointers in the bank slots of the plan's launches"""
    slot = {_ffi.OP_CONV: "wb", _ffi.OP_CONV_PLANES: "wb32", _ffi.OP_CONV_PLANES_BWD: "wb32t"}
    return set(int(getattr(fields(o), slot[o.kind])) for o in _ops(plan) if o.kind in slot and getattr(fields(o), slot[o.kind]))


def _banks_packed(plan):
    """destinations of every segment of the plan's OP_PACK_W tables"""
    out = []
    for o in _ops(plan):
        if o.kind != _ffi.OP_PACK_W:
            continue
        f = fields(o)
        table = [t for t in plan.keep if isinstance(t, torch.Tensor) and t.data_ptr() == int(f.segs)][0]
        out += [int(s.dst) for s in (_ffi.PackSeg * f.nseg).from_buffer_copy(table.cpu().numpy().tobytes())]
    return out


def _engine_banks(eng, which=FORWARD + DGRAD):
    return {(w, n): t.data_ptr() for w in which for n, t in getattr(eng, w).items()}


def _check(lib, eng, plan, which):
    """(1) a set wb slot <=> the library reads it, (2) every bank of the dicts `which` is read by a launch of the plan, (3) every packed segment is a bank"""
    for k, o in enumerate(_ops(plan)):
        if o.kind == _ffi.OP_CONV and fields(o).wb:
            assert _takes_bank(lib, o) == 1, "op %d is given a bank its kernel does not read" % k
    read = _banks_read(plan)
    unread = sorted(key for key, p in _engine_banks(eng, which).items() if p not in read)
    assert not unread, "banks no recorded launch reads: %s" % unread
    banks = set(_engine_banks(eng).values())
    packed = _banks_packed(plan)
    assert packed and len(set(packed)) == len(packed) and set(packed) <= banks
    assert set(_engine_banks(eng, which).values()) <= set(packed)


@pytest.mark.parametrize("bname", BACKENDS)
@pytest.mark.parametrize("size", [(128, 256), (320, 1216), (375, 1242)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("planes", [True, False], ids=["default", "USE_PLANES=False"])
@pytest.mark.parametrize("precision", ["mixed", "bf16"])
def test_a_bank_is_packed_iff_a_recorded_launch_reads_it(bname, size, planes, precision):
    """FULL: no exception.  MAD (block level 4): every given bank is read and every packed segment is an engine bank; the forward banks are all read.  The
    input-gradient banks are the ENGINE's -- _bank_plan does not know which input gradients a plan records -- so a MAD plan packs those of the layers
    outside its block too (as before; the benchmark-size MAD plans are unchanged): each of them is read by the FULL plan of the same engine."""
    backend = _backend(bname)
    eng = E.MadNetEngine(backend.lib, size[0], size[1], B=1, device=backend.device, precision=precision, schedule=E.Schedule(USE_PLANES=planes))
    try:
        _check(backend.lib, eng, eng.build_plan("FULL", lr=1e-4), FORWARD + DGRAD)
        _check(backend.lib, eng, _mad_plan(eng), FORWARD)
    finally:
        eng.close()


@pytest.mark.parametrize("bname", BACKENDS)
def test_the_engine_follows_the_librarys_small_layer_limit(bname):
    """mh_tune_conv_bank(128) and nothing said to the engine: at 60x100 (1/4 resolution = 16x32 pixels) the layers of estimator 2, the context network and
    conv4 no longer get small-layer banks -- they run from planes -- and packing still matches reading"""
    backend = _backend(bname)
    lib = backend.lib
    quarter = [E.est_name(2, j) for j in range(2, 6)] + [E.ctx_name(j) for j in range(2, 4)] + [E.pyr_name(4)]
    eng = E.MadNetEngine(lib, 60, 100, B=1, device=backend.device, precision="mixed")
    eng.build_plan("FULL", lr=1e-4)
    assert all(n in eng.banks and n not in eng.banks32 for n in quarter)
    eng.close()
    lib.tune_conv_bank(128)
    try:
        eng = E.MadNetEngine(lib, 60, 100, B=1, device=backend.device, precision="mixed")
        plan = eng.build_plan("FULL", lr=1e-4)
        assert all(n not in eng.banks and n in eng.banks32 for n in quarter)
        _check(lib, eng, plan, FORWARD + DGRAD)
        eng.close()
    finally:
        lib.tune_conv_bank(-1)


@pytest.mark.parametrize("bname", BACKENDS)
def test_replayed_convs_run_the_family_the_query_promised(bname):
    """one FULL step at 128x256 ('mixed', calibrated weights), its ops replayed one at a time: every conv launch runs a bank kernel exactly where its wb
    slot is set, which is exactly where mh_conv2d_takes_bank says 1"""
    backend = _backend(bname)
    lib = backend.lib
    l, r, gt = S.make_pair(128, 256)
    eng = E.MadNetEngine(lib, 128, 256, B=1, device=backend.device, weights=S.calibrated_weights(OM.variable_shapes(), 1), precision="mixed")
    eng.set_inputs(l, r, gt[..., 0])
    plan = eng.build_plan("FULL", lr=1e-4)
    nbank = 0
    for k, o in enumerate(_ops(plan)):
        one = oplayout.on_callers_stream(_ffi.Op.from_buffer_copy(o))
        lib.plan_run(C.byref(one), 1, None)
        if o.kind == _ffi.OP_CONV:
            kernel = lib.last_kernel().decode()
            given = bool(fields(o).wb)
            assert _takes_bank(lib, o) == int(given) and kernel.startswith(("conv_bank_kernel<", "conv_bank_small_kernel<")) == given, (k, given, kernel)
            nbank += given
    backend.sync()
    assert nbank > 0 and torch.isfinite(eng.pred).all() and eng.pred.abs().max().item() > 0
    eng.close()
