"""MAD adaptation on every block and on several blocks per step (--numBlocks, Stereo_Online_Adaptation.py:98-118,181-208) against the float64 oracle:
all six disparities per arithmetic mode, every block's gradient in fp32 and in 'mixed', plans of several blocks (oracle, bit invariants, poisoned elided
buffers, captured graph) and the Adapter loop around them.

Bounds: EPE_TOL and _check of test_engine_parity.py; for the 'mixed' gradients 4 x m, where m is what the float64 oracle itself loses when the gradient
map behind every conv of the trained block is rounded to bf16 (oracle.madnet.RoundGradBf16) -- nothing here is taken from the engine's output.

Every figure the tests print also goes, appended, into the file the environment variable MAD_BLOCKS_PROFILE names, if it is set (profiles/mad_blocks.txt was
collected that way); unset, the tests write nothing."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from madnet_hip import engine as E
from madnet_hip import _ffi, oplayout
from madnet_hip import synthetic as S
from oracle import madnet as OM
from test_engine_parity import EPE_TOL, PKG, _backend, _check, _proxy_from, _setup

F64 = torch.float64
H0, W0 = 60, 100
BOTH = [pytest.param("emul", id="emul"), pytest.param("hip", marks=pytest.mark.gpu, id="hip")]
PROFILE = os.environ.get("MAD_BLOCKS_PROFILE")          # a file name: the printed figures are appended there too (profiles/mad_blocks.txt is made this way)


def _report(line):
    print(line)
    if PROFILE:
        with open(PROFILE, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _cfg(cfg):
    return json.load(open(os.path.join(PKG, "block_config", cfg)))


def _bv(cfg, block):
    lv = OM.layer_variables()
    return sum([lv[n] for n in _cfg(cfg)[block]], [])


@functools.lru_cache(maxsize=None)
def _weights(seed):
    return S.calibrated_weights(OM.variable_shapes(), seed)


@functools.lru_cache(maxsize=None)
def _pair(H, W, frame=0):
    return S.make_pair(H, W, frame=frame)


def _torch_inputs(H, W, seed, frame):
    wt = {k: torch.from_numpy(v.copy()) for k, v in _weights(seed).items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    return wt, acc, tuple(torch.from_numpy(a) for a in _pair(H, W, frame))


def _engine(backend, H, W, seed, frame, precision, **kw):
    eng = E.MadNetEngine(backend.lib, H, W, B=1, device=backend.device, weights=_weights(seed), precision=precision, **kw)
    l, r, gt = _pair(H, W, frame)
    eng.set_inputs(l, r, gt[..., 0])
    return eng


def _flat(grads, names):
    return torch.cat([grads[n].flatten().to(F64) for n in names])


def _rel(a, b):
    return (a - b).norm().item() / max(b.norm().item(), 1e-300)


# =====================================================================================================================
# A. the oracle's new options
# =====================================================================================================================
def test_oracle_block_list_of_one_equals_the_shorthand_bit_for_bit():
    """step(blocks=[(i, vars)]) IS step(block_index=i, block_vars=vars): same loss, gradients, weights and momentum, bit for bit -- with the reprojection scale
    and with the proxy loss too."""
    for block, kw in ((1, {}), (4, {"reprojection_scale": 2}), (3, {"loss": "proxy"})):
        bv = _bv("MadNet_full.json", block)
        res = []
        for form in ("shorthand", "list"):
            wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
            k = dict(kw)
            if k.get("loss") == "proxy":
                k["proxy"] = _proxy_from(gt)[..., None]
            if form == "shorthand":
                o = OM.step(wt, acc, l, r, gt, mode="MAD", block_vars=bv, block_index=block, lr=1e-2, **k)
            else:
                o = OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(block, bv)], lr=1e-2, **k)
            res.append((o, wt, acc))
        (a, wa, ma), (b, wb, mb) = res
        assert a["loss"] == b["loss"] and a["epe"] == b["epe"] and a["bad3"] == b["bad3"] and torch.equal(a["disparity"], b["disparity"])
        assert list(a["grads"]) == list(b["grads"]) == bv
        for n in bv:
            assert torch.equal(a["grads"][n], b["grads"][n]), n
        for n in wa:
            assert torch.equal(wa[n], wb[n]) and torch.equal(ma[n], mb[n]), n
    with pytest.raises(ValueError):
        wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
        OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(0, _bv("MadNet_full.json", 0))], block_index=0)


def test_oracle_block_list_is_one_forward_then_every_update():
    """Two blocks: each block's gradient is the one its own single-block step computes from the SAME pre-update weights (one forward pass), the update of one
    block does not enter the other's gradient, and everything outside the two blocks stays untouched."""
    b0, b4 = _bv("MadNet_full.json", 0), _bv("MadNet_full.json", 4)
    wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
    o = OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(0, b0), (4, b4)], lr=1e-2)
    assert sorted(o["grads"]) == sorted(b0 + b4)
    for block, bv in ((0, b0), (4, b4)):
        w1, a1, _ = _torch_inputs(H0, W0, 1, 0)
        o1 = OM.step(w1, a1, l, r, gt, mode="MAD", block_vars=bv, block_index=block, lr=1e-2)
        assert o1["loss"] == o["loss"]
        for n in bv:
            assert torch.equal(o1["grads"][n], o["grads"][n]) and torch.equal(w1[n], wt[n]) and torch.equal(a1[n], acc[n]), n
    w0 = _weights(1)
    for n in wt:
        if n not in o["grads"]:
            assert torch.equal(wt[n], torch.from_numpy(w0[n])) and not acc[n].any(), n


def test_oracle_float64_agrees_with_float32_on_all_six_disparities():
    """dtype=torch.float64 runs weights, frames and every op in double: the six maps come back in double and the float32 oracle sits ~1e-5 px from them
    (fp32 round-off, 2^-24 relative per operation, through ~30 layers and the x20 disparity scale; measured 7e-6 px on the two full-resolution maps)."""
    wt, _, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
    with torch.no_grad():
        d32 = OM.forward(wt, l, r)
        d64 = OM.forward(wt, l, r, dtype=F64)
    assert len(d32) == len(d64) == 6
    for i, (a, b) in enumerate(zip(d32, d64)):
        assert a.dtype == torch.float32 and b.dtype == F64 and a.shape == b.shape
        err = (a - b).abs().mean().item()
        print("disparity %d: float32 vs float64 oracle, mean |d| %.3g px (mean disparity %.3g px)" % (i, err, b.abs().mean().item()))
        assert err <= 2e-5, (i, err)
    # ... and the step: gradients in double, the caller's float32 weights updated
    bv = _bv("MadNet_full.json", 2)
    wa, aa, _ = _torch_inputs(H0, W0, 1, 0)
    wb, ab, _ = _torch_inputs(H0, W0, 1, 0)
    oa = OM.step(wa, aa, l, r, gt, mode="MAD", block_vars=bv, block_index=2, lr=1e-2)
    ob = OM.step(wb, ab, l, r, gt, mode="MAD", block_vars=bv, block_index=2, lr=1e-2, dtype=F64)
    assert all(g.dtype == F64 for g in ob["grads"].values()) and all(w.dtype == torch.float32 for w in wb.values())
    assert _rel(_flat(oa["grads"], bv), _flat(ob["grads"], bv)) <= 1e-4
    assert abs(oa["loss"] - ob["loss"]) <= 1e-6
    for n in bv:
        assert not torch.equal(wb[n], torch.from_numpy(_weights(1)[n])), n


def test_oracle_bf16_gradient_hook():
    """RoundGradBf16: identity forward, the incoming gradient rounded to bf16 (8 significant bits, round to nearest even); step(bf16_grad_model=True) puts it behind
    the convs of the trained block only, so the forward results stay what they are and the block gradient moves by a bf16-sized amount."""
    x = torch.tensor([1.0, 1.00390625, 1.01171875, -3.1415926], dtype=F64, requires_grad=True)     # 1 + 2^-8 ties to even (1.0), 1 + 3 * 2^-8 ties to even (1 + 2^-6)
    y = OM.RoundGradBf16.apply(x)
    assert torch.equal(y.detach(), x.detach())
    (y * x.detach()).sum().backward()
    assert torch.equal(x.grad, torch.tensor([1.0, 1.0, 1.015625, -3.140625], dtype=F64)), x.grad
    bv = _bv("MadNet_full.json", 1)
    out = []
    for model in (False, True):
        wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
        out.append(OM.step(wt, acc, l, r, gt, mode="MAD", block_vars=bv, block_index=1, lr=1e-2, dtype=F64, bf16_grad_model=model))
    assert out[0]["loss"] == out[1]["loss"] and torch.equal(out[0]["disparity"], out[1]["disparity"])
    m = _rel(_flat(out[1]["grads"], bv), _flat(out[0]["grads"], bv))
    assert 0.0 < m <= 2.0 ** -8, m          # no element's relative rounding error exceeds half a bf16 ulp, 2^-9; a few layers of it stay below 2^-8


# =====================================================================================================================
# B. forward pass: all six disparities per arithmetic mode
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _disparities64(H, W):
    wt, _, (l, r, gt) = _torch_inputs(H, W, 1, 0)
    with torch.no_grad():
        return tuple(d[..., 0] for d in OM.forward(wt, l, r, dtype=F64))


def _forward_plan(eng):
    """a NONE-mode forward pass that also writes every level's full-resolution disparity (disp_k)"""
    return eng.build_plan("NONE", make_disps=tuple(E.LEVELS))


# 60x100: the padded path (64x128 inside), coarsest level 1x2.  128x320: no padding; the quarter resolution 32x80 is one full 64-column tile plus a ragged one.
@pytest.mark.parametrize("bname,size", [pytest.param("emul", (60, 100), id="emul-60x100"), pytest.param("emul", (128, 320), id="emul-128x320", marks=pytest.mark.slow),
                                        pytest.param("hip", (60, 100), id="hip-60x100", marks=pytest.mark.gpu),
                                        pytest.param("hip", (128, 320), id="hip-128x320", marks=pytest.mark.gpu)])
def test_forward_every_level_within_tolerance(bname, size):
    """Every one of the six disparities (levels 6 .. 3, the context output, the rescaled prediction) of the fp32 and the 'mixed' forward pass within EPE_TOL of
    the float64 oracle -- a MAD block's loss reads its own level's map, not the last one.  Plain bf16 is printed beside them, not gated.

    Before this test 'mixed' ran the estimators of levels 6 .. 4 and conv7 .. conv12 in plain bf16 (judged by the LAST map only): emulator 60x100 mean error
    per map 2.2e-5 / 6.4e-4 / 4.4e-3 / 3.4e-4 / 7.3e-5 / 7.2e-5 px, 128x320 9.4e-5 / 1.6e-3 / 5.7e-3 / 4.2e-4 / 1.3e-4 / 1.3e-4 px -- levels 5 and 4 outside the
    tolerance.  With split-bf16 there too: 60x100 1.1e-9 / 5.0e-7 / 8.1e-6 / 3.6e-5 / 6.8e-5 / 6.7e-5, 128x320 2.9e-7 / 3.2e-6 / 1.4e-5 / 3.8e-5 / 9.9e-5 / 9.9e-5."""
    backend = _backend(bname)
    H, W = size
    ref = _disparities64(H, W)
    err = {}
    for prec in ("fp32", "mixed", "bf16"):
        eng = _engine(backend, H, W, 1, 0, prec)
        _forward_plan(eng).run(backend.lib, 0)
        backend.sync()
        maps = [eng.disp_k[k] for k in E.LEVELS] + [eng.pred]
        err[prec] = [(m.cpu()[0] - d[0]).abs().mean().item() for m, d in zip(maps, ref)]
        assert all(np.isfinite(e) for e in err[prec]), (prec, err[prec])
    _report("forward %s %dx%d: mean |disparity - float64 oracle| per map, px" % (bname, H, W))
    _report("  map            mean|d|      fp32       mixed      bf16")
    for i, name in enumerate(["level 6", "level 5", "level 4", "level 3", "context", "prediction"]):
        _report("  %-12s %9.3g %10.3g %10.3g %10.3g" % (name, ref[i].abs().mean().item(), err["fp32"][i], err["mixed"][i], err["bf16"][i]))
    for prec in ("fp32", "mixed"):
        for i, e in enumerate(err[prec]):
            assert e <= EPE_TOL, (prec, i, e)


# =====================================================================================================================
# C. gradient of every block, both block configurations, fp32 and 'mixed'
# =====================================================================================================================
CFGS = ["MadNet_full.json", "MadNet_piramid_only.json"]
# candidate (weights seed, frame index) pairs of the 'mixed' cases, in the order they are tried: all of them at 60x100 first, then all of them at 128x256
CANDIDATES = [(1, 0), (14, 0), (12, 0), (5, 0), (72, 0), (23, 0), (99, 0)]
BIAS_SHIFT = 5e-5            # 1e-3 px / 20: the forward tolerance at the scale of V
CONDITION = 1e-3             # the float64 oracle's block gradient may move by this much (relative L2) under +-BIAS_SHIFT
# (H, W, seed, frame): the first candidate that meets the condition, per block configuration and block -- evaluated on the CPU with conditioning() below and written
# here as literals; the test re-asserts the condition for its literal only.  Measured movement (MadNet_full.json; MadNet_piramid_only.json within 2 % of it unless given):
#   block 0  60x100: 1.0, no gradient, 1.0, 1.0, 1.8e-3, no gradient, 1.0 (level 6 is 1x2 pixels)     128x256: 3.1e-3, 7.0e-4
#   block 1  60x100: 0.45, 2.1e-3, 8.0e-4
#   block 2  60x100: 9.6e-3, 2.6e-3, 4.8e-3, 1.6e-3, 1.3e-3, 2.7e-3, 2.8e-3                          128x256: 1.0e-2, 3.8e-3, 3.6e-3, 2.3e-3, 7.8e-4
#   block 3  60x100: 6.7e-3, 4.3e-3, 1.1e-2, 7.2e-4
#   block 4  60x100: 6.9e-3, 6.7e-2, 5.5e-3, 3.0e-3, 1.9e-2, no gradient, no gradient                128x256: 4.9e-3, 9.2e-2, 4.9e-3, 2.5e-2, 8.3e-3, 8.5e-4
#            MadNet_piramid_only.json at 128x256: 3.7e-3, 9.6e-2, 5.4e-3, 1.5e-2, 4.2e-3, 1.01e-3, 7.9e-4
# (a seeded search at 128x256 found these three: of seeds 15 .. 102, frame 0, block 2 qualifies on 59, 72, 74 and block 4 on 23 (full) / 99 (piramid_only) only --
#  the curvature of the reprojection loss alone moves most gradients by 2e-3 .. 7e-3 per 1e-3 px)
_FULL = {0: (128, 256, 14, 0), 1: (60, 100, 12, 0), 2: (128, 256, 72, 0), 3: (60, 100, 5, 0), 4: (128, 256, 23, 0)}
CHOSEN = {"MadNet_full.json": _FULL, "MadNet_piramid_only.json": {**_FULL, 4: (128, 256, 99, 0)}}


def _oracle64(cfg, block, seed, frame, H, W, bias_shift=0.0, bf16_grad_model=False, lr=1e-2):
    bv = _bv(cfg, block)
    wt, acc, (l, r, gt) = _torch_inputs(H, W, seed, frame)
    if bias_shift:
        wt["model/G%d/fgc-volume-filtering-%d/disp-6/biases" % (E.LEVELS[block], E.LEVELS[block])] += bias_shift
    o = OM.step(wt, acc, l, r, gt, mode="MAD", block_vars=bv, block_index=block, lr=lr, dtype=F64, bf16_grad_model=bf16_grad_model)
    return o, wt


@functools.lru_cache(maxsize=None)
def conditioning(cfg, block, seed, frame, H=H0, W=W0):
    """how far the float64 oracle's gradient of the block moves (relative L2, the worse of the two signs) when the bias of the level's last estimator layer is
    shifted by +-BIAS_SHIFT: an input on which a disparity sits on the relu kink of _make_disp, or a loss term on one of its own kinks, moves by far more than
    the forward tolerance could explain -- such an input can neither convict nor acquit a 'mixed' gradient"""
    bv = _bv(cfg, block)
    g0 = _flat(_oracle64(cfg, block, seed, frame, H, W)[0]["grads"], bv)
    if not g0.any():
        return float("inf")          # every disparity of the level on the flat side of the relu: no gradient to compare at all
    return max(_rel(_flat(_oracle64(cfg, block, seed, frame, H, W, bias_shift=s)[0]["grads"], bv), g0) for s in (BIAS_SHIFT, -BIAS_SHIFT))


@functools.lru_cache(maxsize=None)
def _reference_and_model(cfg, block, seed, frame, H=H0, W=W0):
    """(the float64 oracle's step, its post-step weights, m): m = relative L2 between the oracle with bf16-rounded gradient maps and the exact one"""
    bv = _bv(cfg, block)
    o, wt = _oracle64(cfg, block, seed, frame, H, W)
    om, _ = _oracle64(cfg, block, seed, frame, H, W, bf16_grad_model=True)
    return o, wt, _rel(_flat(om["grads"], bv), _flat(o["grads"], bv))


def _fp32_cases():
    out = []
    for cfg in CFGS:
        for block in range(5):
            # the emulator takes the blocks test_engine_parity.test_mad_step leaves out there (1, 2, 3 of MadNet_full.json); the MI355X takes all ten
            if cfg == CFGS[0] and block in (1, 2, 3):
                out.append(pytest.param("emul", cfg, block, id="emul-%s-%d" % (cfg[7:-5], block)))
            out.append(pytest.param("hip", cfg, block, marks=pytest.mark.gpu, id="hip-%s-%d" % (cfg[7:-5], block)))
    return out


def _mixed_cases():
    out = []
    for cfg in CFGS:
        for block in range(5):
            if cfg == CFGS[0]:         # (blocks 2 and 4 need a 128x256 input: `slow` on the emulator)
                out.append(pytest.param("emul", cfg, block, id="emul-%s-%d" % (cfg[7:-5], block), marks=([pytest.mark.slow] if block in (2, 4) else [])))
            out.append(pytest.param("hip", cfg, block, marks=pytest.mark.gpu, id="hip-%s-%d" % (cfg[7:-5], block)))
    return out


@pytest.mark.parametrize("bname,cfg,block", _fp32_cases())
def test_block_gradient_fp32(bname, cfg, block):
    """One fp32 MAD step on the block at 60x100 against the float64 oracle, judged by _check of test_engine_parity.py."""
    backend = _backend(bname)
    eng, wn, wt, acc, (l, r, gt) = _setup(backend, H0, W0)
    bv = _bv(cfg, block)
    eng.build_plan("MAD", lr=1e-2, block_vars=bv, block_level=E.LEVELS[block]).run(backend.lib, 0)
    o = OM.step(wt, acc, l, r, gt, mode="MAD", block_vars=bv, block_index=block, lr=1e-2, dtype=F64)
    o["disparity"] = o["disparity"].to(torch.float32)
    _check(eng, wn, wt, o, backend)
    go, ge = _flat(o["grads"], bv), torch.cat([eng.params.tensor(n, "g").cpu().flatten().to(F64) for n in bv])
    _report("gradient fp32 %s %s block %d: relative L2 vs float64 oracle %.3g" % (bname, cfg, block, _rel(ge, go)))


def _mixed_gates(eng, cfg, block, seed, frame, label, H=H0, W=W0, outside=None):
    """the gates of a 'mixed' block gradient: relative L2 <= 4 m, cosine >= 0.999 (against the float64 oracle), every variable outside the block untouched"""
    bv = _bv(cfg, block)
    o, _, m = _reference_and_model(cfg, block, seed, frame, H, W)
    go = _flat(o["grads"], bv)
    ge = torch.cat([eng.params.tensor(n, "g").cpu().flatten().to(F64) for n in bv])
    rel = _rel(ge, go)
    cos = torch.nn.functional.cosine_similarity(ge, go, dim=0).item()
    _report("gradient mixed %s %s block %d (seed %d, frame %d): m %.3g  engine relative L2 %.3g (%.2f m)  cosine %.6f"
            % (label, cfg, block, seed, frame, m, rel, rel / m, cos))
    w0 = _weights(seed)
    for n in w0:
        if n not in (bv if outside is None else outside):
            assert torch.equal(eng.params.tensor(n).cpu(), torch.from_numpy(w0[n])), n
    assert torch.isfinite(ge).all()
    assert rel <= 4 * m, (cfg, block, rel, m)
    assert cos >= 0.999, (cfg, block, cos)
    return rel, m, cos


@pytest.mark.parametrize("bname,cfg,block", _mixed_cases())
def test_block_gradient_mixed(bname, cfg, block):
    """One 'mixed' MAD step on the block on an input the float64 oracle alone is well conditioned on (CHOSEN: blocks 1 and 3 at 60x100, blocks 0, 2 and 4 at
    128x256; the condition is re-asserted), against the float64 oracle: relative L2 of the block gradient <= 4 x m, cosine >= 0.999, everything outside the block
    bit-identical.  m / engine relative L2 / cosine per block: profiles/mad_blocks.txt (MI355X and emulator)."""
    backend = _backend(bname)
    H, W, seed, frame = CHOSEN[cfg][block]
    c = conditioning(cfg, block, seed, frame, H, W)
    _report("conditioning %s block %d: (%dx%d, seed %d, frame %d) moves by %.3g under +-%g" % (cfg, block, H, W, seed, frame, c, BIAS_SHIFT))
    assert c <= CONDITION, ("the committed input is not well conditioned for this block", cfg, block, c)
    eng = _engine(backend, H, W, seed, frame, "mixed")
    eng.build_plan("MAD", lr=1e-2, block_vars=_bv(cfg, block), block_level=E.LEVELS[block]).run(backend.lib, 0)
    backend.sync()
    o, _, _ = _reference_and_model(cfg, block, seed, frame, H, W)
    assert (eng.pred.cpu() - o["disparity"][..., 0]).abs().mean().item() <= EPE_TOL
    assert abs(eng.res_loss[0].item() - o["loss"]) <= 1e-4 * max(1.0, abs(o["loss"]))
    _mixed_gates(eng, cfg, block, seed, frame, bname, H, W)


# =====================================================================================================================
# D. plans that train several blocks
# =====================================================================================================================
def _plan_blocks(cfg, blist):
    return [(E.LEVELS[b], _bv(cfg, b)) for b in blist]


def _state(eng, backend):
    backend.sync()
    P = eng.params
    return P.w.cpu().clone(), P.g[:P.total].cpu().clone(), P.m.cpu().clone()


def _ranges_equal(eng, a, b, names, what):
    for o, c in eng.params.ranges(names):
        for x, y, nm in zip(a, b, "wgm"):
            assert torch.equal(x[o:o + c], y[o:o + c]), (what, nm, o, (x[o:o + c] - y[o:o + c]).abs().max().item())


def _multi_cases():
    full, pyr = CFGS
    lists = [(full, (0, 4)), (full, (4, 0)), (full, (1, 2)), (full, (0, 2, 4)), (full, (0, 1, 2, 3, 4)), (pyr, (2, 4))]
    emul = {(full, (0, 4), "fp32"), (full, (1, 2), "mixed"), (full, (0, 1, 2, 3, 4), "fp32")}
    out = []
    for cfg, bl in lists:
        for prec in ("fp32", "mixed"):
            tag = "%s-%s-%s" % (cfg[7:-5], "".join(map(str, bl)), prec)
            if (cfg, bl, prec) in emul:        # (all five blocks on the emulator: nine engine runs, `slow`)
                out.append(pytest.param("emul", cfg, bl, prec, id="emul-" + tag, marks=([pytest.mark.slow] if len(bl) == 5 else [])))
            out.append(pytest.param("hip", cfg, bl, prec, marks=pytest.mark.gpu, id="hip-" + tag))
    return out


@pytest.mark.parametrize("bname,cfg,blist,prec", _multi_cases())
def test_multi_block_plan(bname, cfg, blist, prec, monkeypatch):
    """One MAD step that trains several blocks (Adapter(num_blocks=k) records loss, backward and update per block, one after the other).
    fp32: against the multi-block float64 oracle with _check.  'mixed': recorded with MH_POISON_ELIDED=1 (every fp32 buffer whose store the plan drops is NaN from the
    start) -- nothing in w / g / m is NaN and every block's gradient passes the gates of the single-block 'mixed' test.
    Bits, both modes: the plan equals part='grad' followed by part='update'; every block's w / g / m ranges equal those of its single-block plan on a fresh
    engine; the reversed block list ends in the same weights."""
    backend = _backend(bname)
    lr = 1e-2
    blocks = _plan_blocks(cfg, blist)
    names = sum((bv for _, bv in blocks), [])
    if prec == "mixed":
        monkeypatch.setenv("MH_POISON_ELIDED", "1")
    eng = _engine(backend, H0, W0, 1, 0, prec)
    assert eng.sched.POISON_ELIDED == (prec == "mixed")
    plan = eng.build_plan("MAD", lr=lr, blocks=blocks)
    plan.run(backend.lib, 0)
    whole = _state(eng, backend)
    for t in whole:
        assert torch.isfinite(t).all()
    if prec == "fp32":
        wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
        o = OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(b, _bv(cfg, b)) for b in blist], lr=lr, dtype=F64)
        o["disparity"] = o["disparity"].to(torch.float32)
        _check(eng, _weights(1), wt, o, backend)
    else:
        _report("multi-block mixed %s %s %s: plan.elided = %d buffers" % (bname, cfg, blist, len(plan.elided)))
        for lo, nb in plan.elided:
            # whoever still points into an elided buffer must be an input gradient that was told so (it stages the bf16 shadow instead) or the writer itself
            for i in range(plan.n):
                hits = oplayout.pointers_into(plan.arr[i], lo, lo + nb)
                if hits:
                    f = oplayout.fields(plan.arr[i])
                    _report("  elided %#x (%d bytes): op %d kind %d slots %s flags %#x" % (lo, nb, i, plan.arr[i].kind, hits, f.flags))
                    assert plan.arr[i].kind == _ffi.OP_CONV and f.mode == 1 and f.precision == 1, (i, hits)
                    assert f.flags & (oplayout.CONV_SHADOW_ONLY | oplayout.CONV_IN_F32_STALE | oplayout.CONV_MASK_F32_STALE), (i, hits, f.flags)
        wt, acc, (l, r, gt) = _torch_inputs(H0, W0, 1, 0)
        o = OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(b, _bv(cfg, b)) for b in blist], lr=lr, dtype=F64)
        assert (eng.pred.cpu() - o["disparity"][..., 0]).abs().mean().item() <= EPE_TOL
        assert abs(eng.res_loss[0].item() - o["loss"]) <= 1e-4 * max(1.0, abs(o["loss"]))
        w0 = _weights(1)
        for n in w0:
            if n not in names:
                assert torch.equal(eng.params.tensor(n).cpu(), torch.from_numpy(w0[n])), n
        for b in blist:                                 # (a block's gradient in the several-block step is its single-block gradient: same reference, same m)
            _mixed_gates(eng, cfg, b, 1, 0, "%s in %s" % (bname, "".join(map(str, blist))), outside=names)
        monkeypatch.delenv("MH_POISON_ELIDED")
    # ---- bits: grad then update
    e2 = _engine(backend, H0, W0, 1, 0, prec)
    e2.build_plan("MAD", lr=lr, blocks=blocks, part="grad").run(backend.lib, 0)
    backend.sync()
    w_before = e2.params.w.cpu().clone()
    for n, v in _weights(1).items():                   # the 'grad' part moves no weight
        assert torch.equal(e2.params.tensor(n).cpu(), torch.from_numpy(v)), n
    e2.build_plan("MAD", lr=lr, blocks=blocks, part="update").run(backend.lib, 0)
    split = _state(e2, backend)
    assert not torch.equal(w_before, split[0])
    _ranges_equal(eng, whole, split, names, "grad + update")
    assert torch.equal(whole[0], split[0]) and torch.equal(whole[2], split[2])
    # ---- bits: every block alone on a fresh engine
    for b in blist:
        e1 = _engine(backend, H0, W0, 1, 0, prec)
        e1.build_plan("MAD", lr=lr, block_vars=_bv(cfg, b), block_level=E.LEVELS[b]).run(backend.lib, 0)
        _ranges_equal(eng, whole, _state(e1, backend), _bv(cfg, b), "single block %d" % b)
    # ---- bits: the reversed list
    if len(blist) == 2:
        e3 = _engine(backend, H0, W0, 1, 0, prec)
        e3.build_plan("MAD", lr=lr, blocks=blocks[::-1]).run(backend.lib, 0)
        assert torch.equal(whole[0], _state(e3, backend)[0])


@pytest.mark.parametrize("bname", BOTH)
@pytest.mark.parametrize("variant", ["scale2", "proxy"])
def test_multi_block_plan_scaled_and_proxy(bname, variant):
    """Blocks (0, 4) in one fp32 step with --reprojectionScale 2 / with the proxy-label loss of the continual variant, against the multi-block float64 oracle."""
    backend = _backend(bname)
    cfg, blist, lr = CFGS[0], (0, 4), 1e-2
    eng, wn, wt, acc, (l, r, gt) = _setup(backend, H0, W0)
    kw = {}
    if variant == "scale2":
        eng.set_reprojection_scale(2)
        kw["reprojection_scale"] = 2
    else:
        px = _proxy_from(gt)
        eng.loss_kind = "proxy"
        eng.set_inputs(l, r, gt[..., 0], proxy=px)
        kw.update(loss="proxy", proxy=px[..., None])
    eng.build_plan("MAD", lr=lr, blocks=_plan_blocks(cfg, blist)).run(backend.lib, 0)
    o = OM.step(wt, acc, l, r, gt, mode="MAD", blocks=[(b, _bv(cfg, b)) for b in blist], lr=lr, dtype=F64, **kw)
    o["disparity"] = o["disparity"].to(torch.float32)
    _check(eng, wn, wt, o, backend)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("cfg,blist", [(CFGS[0], (0, 4)), (CFGS[0], (4, 0)), (CFGS[0], (1, 2)), (CFGS[0], (0, 2, 4)), (CFGS[0], (0, 1, 2, 3, 4)), (CFGS[1], (2, 4))],
                         ids=["full-04", "full-40", "full-12", "full-024", "full-01234", "piramid_only-24"])
def test_multi_block_captured_graph_replays_equal_the_eager_plan(hip, prec, cfg, blist):
    """The captured hipGraph of a several-block plan against the same plan run eagerly (the method of test_captured_graph_replays_equal_the_eager_plan_bit_for_bit):
    three steps on successive frames from the same weights end with torch.equal weights, momentum, gradients and disparity."""
    blocks = _plan_blocks(cfg, blist)
    pairs = [_pair(H0, W0, t) for t in range(3)]
    res = []
    for graph in (False, True):
        eng = _engine(hip, H0, W0, 1, 0, prec)
        plan = eng.build_plan("MAD", lr=1e-3, blocks=blocks)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            if graph:
                w_keep = eng.params.w.clone()
                plan.capture(hip.lib, st.cuda_stream)
                assert torch.equal(eng.params.w, w_keep)
            for l, r, gt in pairs:
                eng.set_inputs(l, r, gt[..., 0])
                st.synchronize()
                plan.launch(hip.lib, st.cuda_stream)
                st.synchronize()
        res.append((eng.params.w.clone(), eng.params.m.clone(), eng.params.g.clone(), eng.pred.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a - b).abs().max().item()
    assert (res[0][1] != 0).any()


# =====================================================================================================================
# E. the loop around it
# =====================================================================================================================
def _softmax(x):
    return np.exp(x) / np.sum(np.exp(x), axis=0)


@pytest.mark.parametrize("bname", BOTH)
@pytest.mark.parametrize("sample_mode", ["PROBABILITY", "SEQUENTIAL", "ARGMAX"])
def test_adapter_two_blocks_per_step_matches_reference_loop(bname, sample_mode):
    """Adapter(num_blocks=2) over three successive frames against the restated reference loop (Stereo_Online_Adaptation.py:178-253) driven by the multi-block
    oracle: the sampled blocks, loss and EPE of every step, the reward on BOTH trained blocks and the fetch counter.  Emulator: 48x64, plans run eagerly;
    MI355X: 60x100, the captured graph."""
    import Nets
    from madnet_hip.adapter import Adapter
    from Sampler import sampler_factory
    backend = _backend(bname)
    (H, W), lr, steps = ((48, 64) if bname == "emul" else (H0, W0)), 1e-3, 3
    blocks_cfg = _cfg(CFGS[0])
    wn = _weights(1)
    frames = [_pair(H, W, t) for t in range(steps)]
    left = torch.zeros(1, H, W, 3, device=backend.device); right = torch.zeros_like(left)
    params = {"left_img": left, "right_img": right, "split_layers": [None], "sequence": True, "train_portion": "BEGIN", "bulkhead": True, "weights": wn}
    if bname == "emul":
        params["_lib"] = backend.lib
    net = Nets.get_stereo_net("MADNet", params)
    ad = Adapter(net, mode="MAD", block_config=blocks_cfg, lr=lr, sample_mode=sample_mode, num_blocks=2, ssim_th=10.0, use_graph=(bname == "hip"))
    np.random.seed(7)
    got = [ad.step(fr[0], fr[1], fr[2][..., 0]) for fr in frames]
    wt = {k: torch.from_numpy(v.copy()) for k, v in wn.items()}
    acc = {k: torch.zeros_like(v) for k, v in wt.items()}
    np.random.seed(7)
    sampler = sampler_factory.get_sampler(sample_mode, 2, 0)
    dist = np.zeros(5); l1 = l2 = 0.0; last = []; counter = [0] * 5
    for t, fr in enumerate(frames):
        blocks = [int(b) for b in np.asarray(sampler.sample(_softmax(dist))).reshape(-1)]
        assert len(blocks) == 2 and blocks[0] != blocks[1]
        for b in blocks:
            counter[b] += 1
        o = OM.step(wt, acc, *(torch.from_numpy(a) for a in fr), mode="MAD", blocks=[(b, _bv(CFGS[0], b)) for b in blocks], lr=lr)
        if t == 0:
            l1 = l2 = o["loss"]
        gain = (2 * l1 - l2) - o["loss"]
        dist = 0.99 * dist
        for i in last:
            dist[i] += 0.01 * gain
        last = blocks; l2 = l1; l1 = o["loss"]
        assert got[t]["blocks"] == blocks, (t, got[t]["blocks"], blocks)
        assert abs(got[t]["loss"] - o["loss"]) <= 1e-4 * max(1.0, abs(o["loss"])), (t, got[t]["loss"], o["loss"])
        assert abs(got[t]["epe"] - o["epe"]) <= 1e-3 * max(1.0, o["epe"])
    assert np.allclose(ad.sample_distribution, dist, atol=1e-6)
    assert np.count_nonzero(dist) >= 2                       # both blocks of a step were rewarded
    assert list(ad.fetch_counter) == counter and sum(ad.fetch_counter) == 2 * steps
    for n in wt:                                             # ... and the weights went where the oracle's went
        assert (net.engine.params.tensor(n).cpu() - wt[n]).abs().max().item() <= 2e-5 * max(1.0, wt[n].abs().max().item()), n
