"""mh_reprojection_loss_masked: mean_SSIM_l1 over the pixels that exist (include/madnet_hip.h), on the emulated build and, marked gpu, the MI355X.

Oracle: masked_loss_oracle (the header's definition in torch, float64, gradient from autograd).  Bounds: those tests/test_ops_parity.py::
test_reprojection_loss_and_grad and tests/test_loss_tiles.py hold the unmasked op to -- value within 2e-6 max(1, |ref|), gradient within 8 E32 + 1e-12 per pixel
(E32 = the float32 evaluation of the oracle against its float64 evaluation), every gradient element finite, exactly 0 where v = 0.

Inputs: seeded 8-bit-valued frames, disparities in (-1, 5) (taps clamp at both borders), masks with a border band on each side of both views, rectangles in
both, and one rectangle of the right view inside the left view's valid area (left pixels that are invalid through valid_r alone).  The band is 2 .. 5 pixels wide
where the frame allows it: at (1,7,9) a band of 2 on each side leaves 3 x 5 = 15 pixels, fewer than the B H W / 4 = 15.75 the case must keep valid, so there
(and wherever min(H, W) < 12) the band is one pixel; (1,3,3) has all-ones masks."""
import ctypes as C
import functools

import pytest
import torch

import footprint as FP
import masked_loss_oracle as MO
from madnet_hip import ops

MH_ERR_ARG, MH_ERR_ALIGN = -1, -2
SHAPES = [(1, 3, 3), (1, 7, 9), (2, 37, 53), (1, 17, 65), (2, 31, 31)]      # around the 16 x 32 tile and its 2-pixel halo
_ids = lambda s: "%dx%dx%d" % s


SEEDS = {(1, 7, 9): 2}           # chosen with the oracle on the CPU so that N1 >= B H W / 4, N2 >= 1 and a pixel is invalid through valid_r alone (asserted in test a); else 5


def _inputs(shape, seed=None):
    B, H, W = shape
    seed = SEEDS.get(shape, 5) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    left = torch.floor(torch.rand(B, H, W, 3, generator=g) * 256)
    right = torch.floor(torch.rand(B, H, W, 3, generator=g) * 256)
    disp = torch.rand(B, H, W, generator=g) * 6 - 1
    vl = torch.ones(B, H, W, dtype=torch.uint8)
    vr = torch.ones(B, H, W, dtype=torch.uint8)
    if (H, W) != (3, 3):
        for m in (vl, vr):
            t, b, l, r = (int(k) if min(H, W) >= 12 else 1 for k in torch.randint(2, 6, (4,), generator=g))
            m[:, :t] = 0; m[:, H - b:] = 0; m[:, :, :l] = 0; m[:, :, W - r:] = 0
        rh, rw = max(1, H // 8), max(1, W // 8)
        vl[:, H // 2:H // 2 + rh, W // 4:W // 4 + rw] = 0
        vl[B - 1, H // 4:H // 4 + rh, W // 2:W // 2 + rw] = 0
        vr[:, H // 3:H // 3 + rh, W // 2:W // 2 + rw] = 0                 # inside the left view's valid area: left pixels that sample it are invalid through valid_r alone
        vr[0, 2 * H // 3:2 * H // 3 + 1, W // 3:W // 3 + rw] = 0
    return left, right, disp, vl, vr


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs (CPU) and both evaluations of the oracle, made once, never modified"""
    left, right, disp, vl, vr = _inputs(shape)
    o64 = MO.evaluate(disp, left, right, vl, vr, torch.float64)
    o32 = MO.evaluate(disp, left, right, vl, vr, torch.float32)
    e32 = (o32["grad"].double() - o64["grad"]).abs().max().item()
    return dict(shape=shape, left=left, right=right, disp=disp, vl=vl, vr=vr, o=o64, e32=e32)


def _run(backend, c, phases=(0,), grad=True, grad_scale=1.0, masked=True, plan_masks=None, **over):
    """one call (or its phases in turn) with result, ddisp and an exact-size NaN-filled workspace in guarded allocations -> (result [4], ddisp, ws Guarded)"""
    lib, dev = backend.lib, backend.device
    B, H, W = c["shape"]
    t = dict(c, **over)
    ws = FP.Guarded(lib.loss_ws_floats(B, H, W), torch.float32, dev)
    res = FP.Guarded(4, torch.float32, dev)
    dd = FP.Guarded(B * H * W, torch.float32, dev) if grad else None
    ws.t.fill_(float("nan"))
    if plan_masks is not None:
        ops.loss_set_valid(lib, ws.t, plan_masks[0].to(dev), plan_masks[1].to(dev))
    left, right, disp = t["left"].to(dev), t["right"].to(dev), t["disp"].to(dev)
    valid = (t["vl"].to(dev), t["vr"].to(dev)) if masked else None
    for ph in phases:
        ops.reprojection_loss(lib, left, right, disp, ws.t, res.t, dd.t.view(B, H, W) if grad else None, grad_scale=grad_scale, phase=ph, valid=valid)
    backend.sync()
    what = "masked loss %s" % (c["shape"],)
    ws.assert_guards(what); res.assert_guards(what)
    if grad:
        dd.assert_guards(what)
    return res.t.cpu().clone(), (dd.t.cpu().view(B, H, W).clone() if grad else None), ws


# ---- a. float64 oracle ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_masked_loss_equals_the_float64_oracle(backend, shape):
    c = _case(shape)
    o = c["o"]
    B, H, W = shape
    v = o["v"]
    only_r = (c["vl"] != 0) & ~v
    print("%s: N1 %d of %d, N2 %d, invalid through valid_r alone %d" % (shape, o["n1"], B * H * W, o["n2"], int(only_r.sum())))
    assert 4 * o["n1"] >= B * H * W and o["n2"] >= 1
    if shape == (1, 3, 3):
        assert bool(c["vl"].all()) and bool(c["vr"].all())
    else:
        assert int(only_r.sum()) >= 1 and int((c["vl"] == 0).sum()) > 0
    res, dd, _ = _run(backend, c)
    err = (dd.double() - o["grad"]).abs().max().item()
    print("  result %r, oracle %r; max|ddisp - g64| %.3g, E32 %.3g" % (res[:3].tolist(), [o["loss"], o["ss"], o["l1"]], err, c["e32"]))
    for got, ref in zip(res[:3].tolist(), (o["loss"], o["ss"], o["l1"])):
        assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (got, ref)
    assert torch.isfinite(dd).all()
    assert err <= 8 * c["e32"] + 1e-12, (err, c["e32"])
    assert bool((dd[~v] == 0).all())


# ---- b. all-ones masks ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phases", [(0,), (1, 2)], ids=["phase0", "phase1then2"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_all_ones_masks_give_the_unmasked_bits(backend, shape, phases):
    """N1 = B H W and N2 = B (H-2) (W-2) are below 2^24 here, so (float)N * 3.0f and the unmasked kernel's (float)B * (float)H * (float)W * 3.0f are the same
    float (every factor and the product are exact) and so are the float64 divisors of the final reduction: the same bits."""
    c = _case(shape)
    ones = torch.ones_like(c["vl"])
    assert shape[0] * shape[1] * shape[2] < 2 ** 24
    r0, d0, _ = _run(backend, c, phases=phases, masked=False)
    r1, d1, _ = _run(backend, c, phases=phases, vl=ones, vr=ones)
    assert torch.equal(FP.bits(r0[:3]), FP.bits(r1[:3])), (r0, r1)
    assert torch.equal(FP.bits(d0), FP.bits(d1))
    assert torch.isfinite(r1[:3]).all() and torch.isfinite(d1).all()


# ---- c. nothing under an invalid pixel matters ----------------------------------------------------------------------------------------------------------
def test_values_under_invalid_pixels_reach_nothing(backend):
    c = _case((2, 37, 53))
    v = c["o"]["v"]
    nan = float("nan")
    left, right, disp = c["left"].clone(), c["right"].clone(), c["disp"].clone()
    left[~v] = nan                                      # every invalid pixel of the left view (also those invalid through valid_r or the warp)
    right[c["vr"] == 0] = nan                           # the right view's band and rectangles
    disp[c["vl"] == 0] = nan
    idx = (~v & (c["vl"] != 0)).nonzero()[:7]           # a few pixels that are invalid through the right view: an absurd disparity
    assert len(idx) == 7
    disp[idx[:, 0], idx[:, 1], idx[:, 2]] = 1e30
    # (their taps then clamp to column 0, which lies in the right view's band: still invalid)
    assert torch.equal(MO.validity(disp, c["vl"], c["vr"]), v)
    r0, d0, _ = _run(backend, c)
    r1, d1, _ = _run(backend, c, left=left, right=right, disp=disp)
    assert torch.isfinite(r1[:3]).all() and torch.isfinite(d1).all()
    assert torch.equal(FP.bits(r0[:3]), FP.bits(r1[:3])) and torch.equal(FP.bits(d0), FP.bits(d1))


# ---- d. empty sets --------------------------------------------------------------------------------------------------------------------------------------------
def test_empty_sets(backend):
    c = _case((2, 37, 53))
    res, dd, _ = _run(backend, c, vl=torch.zeros_like(c["vl"]))
    assert bool((res[:3] == 0).all()) and bool((dd == 0).all())
    B, H, W = c["shape"]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    checker = (((yy + xx) % 2) == 0).to(torch.uint8)[None].expand(B, H, W).contiguous()
    o = MO.evaluate(c["disp"], c["left"], c["right"], checker, c["vr"], torch.float64)
    o32 = MO.evaluate(c["disp"], c["left"], c["right"], checker, c["vr"], torch.float32)
    assert o["n2"] == 0 and o["n1"] > 0 and o["ss"] == 0.0
    res, dd, _ = _run(backend, c, vl=checker)
    assert res[1].item() == 0.0
    assert abs(res[2].item() - o["l1"]) <= 2e-6 * max(1.0, abs(o["l1"])) and abs(res[0].item() - o["loss"]) <= 2e-6 * max(1.0, abs(o["loss"]))
    e32 = (o32["grad"].double() - o["grad"]).abs().max().item()
    assert torch.isfinite(dd).all() and (dd.double() - o["grad"]).abs().max().item() <= 8 * e32 + 1e-12 and bool((dd[~o["v"]] == 0).all())


# ---- e. footprint -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 17, 65)], ids=_ids)
def test_footprint_phases_and_repeated_calls(backend, shape):
    """exact-size guarded workspace prefilled with NaN (_run asserts the guards); the mask bytes a plan keeps in ws are not written; result[3] is untouched; phase 1
    alone leaves result alone; two calls give the same bits"""
    c = _case(shape)
    lib = backend.lib
    B, H, W = shape
    n = B * H * W
    other = (torch.ones_like(c["vl"]) * 0xA5, torch.ones_like(c["vr"]) * 0x5A)       # bytes the op must leave where a plan put them (it reads its masks from the pointers)
    r0, d0, ws = _run(backend, c, plan_masks=other)
    raw = ws.t.view(torch.uint8).cpu()
    o = 4 * int(lib.loss_valid_offset(B, H, W))
    assert o % 16 == 0 and o >= 4 * int(lib.smoothness_ws_floats(B, H, W))
    o2 = o + (n + 15) // 16 * 16
    assert bool((raw[o:o + n] == 0xA5).all()) and bool((raw[o2:o2 + n] == 0x5A).all())
    assert o2 + (n + 15) // 16 * 16 + 8 * int(lib.smoothness_ws_floats(B, H, W)) <= 4 * (8 * n + 12 * B * (H - 2) * (W - 2))       # the counts end inside the retired map region
    assert FP.bits(r0[3:4]).item() == FP.NAN32
    r1, d1, _ = _run(backend, c)
    assert torch.equal(FP.bits(r0[:3]), FP.bits(r1[:3])) and torch.equal(FP.bits(d0), FP.bits(d1))
    r12, d12, _ = _run(backend, c, phases=(1, 2))
    assert torch.equal(FP.bits(r0[:3]), FP.bits(r12[:3])) and torch.equal(FP.bits(d0), FP.bits(d12)) and FP.bits(r12[3:4]).item() == FP.NAN32
    ronly, donly, _ = _run(backend, c, phases=(1,))
    assert bool((FP.bits(ronly) == FP.NAN32).all()) and torch.equal(FP.bits(d0), FP.bits(donly))
    rf, _, _ = _run(backend, c, grad=False)
    assert torch.equal(FP.bits(r0[:3]), FP.bits(rf[:3]))
    rs, ds, _ = _run(backend, c, grad_scale=0.25)
    assert torch.equal(FP.bits(ds), FP.bits(d0 * 0.25)) and torch.equal(FP.bits(rs[:3]), FP.bits(r0[:3]))


# ---- f. argument errors -----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(backend):
    lib, dev = backend.lib, backend.device
    c = _case((1, 7, 9))
    B, H, W = c["shape"]
    left, right, disp, vl, vr = (c[k].to(dev) for k in ("left", "right", "disp", "vl", "vr"))
    ws = torch.full((lib.loss_ws_floats(B, H, W) + 4,), -7.0, device=dev)
    res = torch.full((4,), -7.0, device=dev)
    dd = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(left=p(left), right=p(right), disp=p(disp), valid_l=p(vl), valid_r=p(vr), ws=p(ws), result=p(res), ddisp=p(dd), grad_scale=1.0, B=B, H=H, W=W,
                phase=0, stream=None)
    bad = [dict(valid_l=None), dict(valid_r=None), dict(left=None), dict(right=None), dict(disp=None), dict(ws=None), dict(result=None), dict(phase=-1),
           dict(phase=3), dict(phase=4), dict(H=2), dict(W=2), dict(B=0), dict(B=2, H=16384, W=16384)]
    for change in bad:
        assert lib._raw_mh_reprojection_loss_masked(*dict(good, **change).values()) == MH_ERR_ARG, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_reprojection_loss_masked: ") and len(msg) > len("mh_reprojection_loss_masked: "), (change, msg)
    assert lib._raw_mh_reprojection_loss_masked(*dict(good, ws=C.c_void_p(ws.data_ptr() + 4)).values()) == MH_ERR_ALIGN
    backend.sync()
    for t in (ws, res, dd):
        assert bool((t == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_reprojection_loss_masked(*good.values()) == 0
    backend.sync()
    assert bool((res[:3] != -7.0).all()) and res[3].item() == -7.0 and bool((dd != -7.0).all())
