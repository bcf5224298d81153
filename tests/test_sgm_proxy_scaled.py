"""mh_sgm_proxy_scaled (the matcher on half-size gray frames, labels doubled and written to their 2 x 2 pixels) against tests/sgm_scaled_oracle.py, the numpy
restatement of the definition in include/madnet_hip.h.

Pass rule: that of tests/test_sgm_proxy_paths.py::check -- the valid mask `out > 0` and floor(out) equal the oracle's exactly, `out` is within one float32 ulp at
the magnitude of the oracle's (doubled) label; doubling is exact, so it keeps the half-resolution bound.  With the median the magnitude is twice the largest
half-resolution label of the pixel's 3x3 window.  No pixel is excluded.

Frames come from madnet_hip.synthetic.make_pair, the small ones are windows of the 40 x 256 pair."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as FP
import sgm8_oracle
import sgm_scaled_oracle as SC
import sgm_speckle_oracle as SO
from madnet_hip import ops, synthetic as S
from madnet_hip.proxy import ProxyMatcher
from test_sgm_proxy_paths import check

MH_ERR_ARG, MH_ERR_ALIGN = -1, -2
_frames, _ref = {}, {}

# name -> (B, H, W, D), D = the full-resolution range
CASES = {
    "1x40x256_D128": (1, 40, 256, 128),                    # the fixture's frame
    "2x27x45_D128": (2, 27, 45, 128),                      # odd H and W, two scenes, w = 23 < D / 2
    "1x13x17_D128": (1, 13, 17, 128),                      # the smallest legal frame: h = 7, w = 9
    "1x41x131_D256": (1, 41, 131, 256),                    # two disparities per lane, odd sizes
    "1x26x140_D384": (1, 26, 140, 384),                    # three disparities per lane
}
WINDOWS = {"2x27x45_D128": (8, 150), "1x13x17_D128": (16, 200), "1x26x140_D384": (10, 100)}      # (row, column) of the window's corner in the 40 x 256 pair
MODES = [(4, 0), (8, 1)]


def frames(name):
    """(left, right) uint8 [B,H,W,3] of a case, made once"""
    if name not in _frames:
        B, H, W, D = CASES[name]
        if name in WINDOWS:
            y, x = WINDOWS[name]
            pairs = [tuple(a[:, y:y + H, x:x + W] for a in S.make_pair(40, 256, stream_id=b)) for b in range(B)]
        else:
            pairs = [S.make_pair(H, W, stream_id=b) for b in range(B)]
        l, r = (np.ascontiguousarray(np.concatenate([p[i] for p in pairs])).astype(np.uint8) for i in range(2))
        assert l.shape == (B, H, W, 3)
        l.setflags(write=False); r.setflags(write=False)
        _frames[name] = (l, r)
    return _frames[name]


def half_labels(name, paths, median):
    """the oracle's half-resolution labels [B,h,w] of a case, made once; the median is applied to the shared unfiltered map"""
    key = (name, paths)
    if key not in _ref:
        l, r = frames(name)
        _ref[key] = SC.half_stage(l, r, CASES[name][3], paths=paths, median=0)
        _ref[key].setflags(write=False)
    if not median:
        return _ref[key]
    if key + (1,) not in _ref:
        _ref[key + (1,)] = np.stack([sgm8_oracle.median3(o) for o in _ref[key]])
        _ref[key + (1,)].setflags(write=False)
    return _ref[key + (1,)]


def check_scaled(got, half, half_raw, H, W, median):
    """got [B,H,W] against the doubled, upsampled oracle labels `half`; half_raw: the oracle's labels in front of the median"""
    ref = SC.up2(half, H, W)
    assert (ref > 0).sum() >= 40 and np.unique(np.floor(ref[ref > 0])).size >= 3, "the case compares (almost) nothing"
    if median:
        check(got, ref, scale=SC.up2(np.stack([sgm8_oracle.window_max(o) for o in half_raw]), H, W))
    else:
        check(got, ref)


def run(backend, l, r, D, paths, median, scale=2, ws=None, out=None, **kw):
    dev = backend.device
    B, H, W, _ = l.shape
    lt, rt = torch.from_numpy(np.array(l)).to(dev), torch.from_numpy(np.array(r)).to(dev)
    ws = ops.sgm_proxy_ws(backend.lib, B, H, W, D, dev, paths=paths, median=median, scale=scale) if ws is None else ws
    out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev) if out is None else out
    ops.sgm_proxy(backend.lib, lt, rt, ws, out, D, paths=paths, median=median, scale=scale, **kw)
    backend.sync()
    return out.cpu().numpy().reshape(B, H, W), ws


def align16(n):
    return (n + 15) // 16 * 16


def ws_formula(lib, B, H, W, D, paths, median):
    h, w = (H + 1) // 2, (W + 1) // 2
    return align16(2 * B * h * w) + lib.sgm_ws_bytes_ex(B, h, w, D // 2, paths, median) + align16(B * h * w * 4)


# ---- 1. oracle equality ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths,median", MODES, ids=["4paths", "8paths-median"])
@pytest.mark.parametrize("name", list(CASES))
def test_scaled_vs_oracle(backend, name, paths, median):
    B, H, W, D = CASES[name]
    l, r = frames(name)
    got, _ = run(backend, l, r, D, paths, median)
    check_scaled(got, half_labels(name, paths, median), half_labels(name, paths, 0), H, W, median)


def test_scaled_float_frames_vs_oracle(backend):
    """float32 frames with fractions on both sides of .5 (exact in float32), a few values outside 0 .. 255: the oracle on the same floats"""
    name = "2x27x45_D128"
    B, H, W, D = CASES[name]
    l, r = frames(name)
    rng = np.random.default_rng(27045)
    fr = np.array([-0.4375, -0.25, 0.25, 0.4375, 0.5, 0.5625, 0.75], np.float32)
    lf, rf = ((a.astype(np.float32) + fr[rng.integers(0, fr.size, a.shape)]).astype(np.float32) for a in (l, r))
    lf[0, 3, 5] = -3.25; lf[1, 20, 40] = 258.75; rf[0, 26, 44] = 300.5; rf[1, 0, 0] = -0.75
    half = SC.half_stage(lf, rf, D, paths=8, median=0)
    assert not np.array_equal(SC.half_gray(lf[0]), SC.half_gray(l[0])), "the fractions changed nothing"
    got, _ = run(backend, lf, rf, D, 8, 1)
    check_scaled(got, np.stack([sgm8_oracle.median3(o) for o in half]), half, H, W, 1)


# ---- 2. the half stage against the existing kernels --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths,median", MODES, ids=["4paths", "8paths-median"])
def test_scaled_is_up2_of_the_matcher_on_the_oracles_half_grays(backend, paths, median):
    """mh_sgm_proxy_ex on RGB frames whose channels equal the oracle's half gray, at (h, w, D / 2); up2 of its labels equals the new entry bit for bit"""
    name = "2x27x45_D128"
    B, H, W, D = CASES[name]
    l, r = frames(name)
    h, w = (H + 1) // 2, (W + 1) // 2
    gl, gr = (np.stack([SC.as_rgb(SC.half_gray(a)) for a in v]) for v in (l, r))
    assert gl.shape == (B, h, w, 3)
    small, _ = run(backend, gl, gr, D // 2, paths, median, scale=1)
    got, _ = run(backend, l, r, D, paths, median)
    assert (got > 0).any()
    assert np.array_equal(got.view(np.uint32), SC.up2(small, H, W).view(np.uint32))


# ---- 3. scale 1 through the new entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths,median", MODES, ids=["4paths", "8paths-median"])
def test_scale_1_is_mh_sgm_proxy_ex(backend, paths, median):
    lib, dev = backend.lib, backend.device
    for shape in ((1, 7, 9, 64), (2, 23, 131, 64), (1, 375, 1242, 128), (3, 12, 129, 192), (1, 3, 3, 64), (0, 9, 9, 64), (1, 9, 9, 100)):
        assert lib.sgm_ws_bytes_scaled(*shape, paths, median, 1) == lib.sgm_ws_bytes_ex(*shape, paths, median)
    B, H, W, D = 2, 27, 45, 64
    l, r = frames("2x27x45_D128")
    lt, rt = torch.from_numpy(np.array(l)).to(dev), torch.from_numpy(np.array(r)).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    outs = []
    for scaled in (False, True):
        ws = torch.empty(lib.sgm_ws_bytes_ex(B, H, W, D, paths, median), dtype=torch.uint8, device=dev)
        out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
        if scaled:
            lib.sgm_proxy_scaled(p(lt), p(rt), 1, p(ws), p(out), B, H, W, D, 10, 120, 95, 1, paths, median, 1, None)
        else:
            lib.sgm_proxy_ex(p(lt), p(rt), 1, p(ws), p(out), B, H, W, D, 10, 120, 95, 1, paths, median, None)
        backend.sync()
        outs.append(out.cpu().numpy())
    assert (outs[0] > 0).any()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


# ---- 4. guards and determinism -----------------------------------------------------------------------------------------------------------------------
def test_scaled_workspace_size_is_the_formula(backend):
    lib = backend.lib
    for B, H, W, D in list(CASES.values()) + [(1, 375, 1242, 128), (3, 14, 18, 256)]:
        for paths, median in ((4, 0), (4, 1), (8, 0), (8, 1)):
            n = lib.sgm_ws_bytes_scaled(B, H, W, D, paths, median, 2)
            assert n == ws_formula(lib, B, H, W, D, paths, median) and n % 16 == 0, (B, H, W, D, paths, median, n)
    assert lib.sgm_ws_bytes_scaled(1, 375, 1242, 128, 4, 0, 2) * 7 < lib.sgm_ws_bytes_ex(1, 375, 1242, 128, 4, 0)


@pytest.mark.parametrize("paths,median", MODES, ids=["4paths", "8paths-median"])
@pytest.mark.parametrize("name", ["2x27x45_D128", "1x13x17_D128"])
def test_scaled_exact_workspace_and_guarded_labels(backend, name, paths, median):
    """ws of exactly mh_sgm_ws_bytes_scaled bytes between guard zones, guard zones around the labels: the last odd row and column do not spill, every label is
    overwritten, a second call into the same buffers gives the same bits"""
    lib, dev = backend.lib, backend.device
    B, H, W, D = CASES[name]
    l, r = frames(name)
    nbytes = lib.sgm_ws_bytes_scaled(B, H, W, D, paths, median, 2)
    assert nbytes == ws_formula(lib, B, H, W, D, paths, median)
    ws = FP.Guarded(nbytes, torch.uint8, dev)
    out = FP.Guarded(B * H * W, torch.float32, dev)
    assert ws.ptr() % 16 == 0
    got, _ = run(backend, l, r, D, paths, median, ws=ws.t, out=out.t)
    ws.assert_guards("scaled sgm ws %s (%d bytes)" % (name, nbytes))
    FP.assert_fully_written(out, B * H * W, "scaled sgm labels %s" % name)
    check_scaled(got, half_labels(name, paths, median), half_labels(name, paths, 0), H, W, median)
    again, _ = run(backend, l, r, D, paths, median, ws=ws.t, out=out.t)
    ws.assert_guards("scaled sgm ws %s, second call" % name)
    out.assert_guards("scaled sgm labels %s, second call" % name)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "a second call into the same workspace changed the result"


def test_scaled_labels_at_an_unaligned_address(backend):
    """the labels start 4, 8 and 12 bytes behind a 16-byte boundary: the wide stores of the upsampling begin at the row's own boundary, guards intact, same bits"""
    lib, dev = backend.lib, backend.device
    name = "2x27x45_D128"
    B, H, W, D = CASES[name]
    l, r = frames(name)
    want, ws = run(backend, l, r, D, 4, 0)
    for off in (1, 2, 3):
        g = FP.Guarded(B * H * W + off, torch.float32, dev)
        out = g.t[off:]
        assert out.data_ptr() % 16 == 4 * off
        got, _ = run(backend, l, r, D, 4, 0, ws=ws, out=out)
        g.assert_guards("scaled sgm labels at +%d floats" % off)
        assert bool((FP.bits(g.t[:off]) == g.fill).all()), "the floats in front of the labels were written"
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), off


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------------------------------
def test_scaled_argument_checks(backend):
    lib, dev = backend.lib, backend.device
    B, H, W, D = 1, 13, 17, 128
    for bad in ((B, H, W, D, 4, 0, 0), (B, H, W, D, 4, 0, 3), (B, H, W, D, 4, 0, -1), (B, H, W, 64, 4, 0, 2), (B, H, W, 192, 4, 0, 2), (B, 12, W, D, 4, 0, 2),
                (B, H, 16, D, 4, 0, 2), (0, H, W, D, 4, 0, 2), (B, H, W, D, 6, 0, 2), (B, H, W, D, 4, 2, 2), (B, H, W, 512, 4, 0, 2)):
        assert lib.sgm_ws_bytes_scaled(*bad) == 0, bad
    l = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
    big = torch.zeros(1, 26, 34, 3, dtype=torch.uint8, device=dev)      # H = 12 and W = 16 read inside it
    ws = torch.empty(lib.sgm_ws_bytes_ex(1, 26, 34, 192, 8, 1), dtype=torch.uint8, device=dev)      # large enough for every call below, legal or not
    out = torch.full((26 * 34,), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(left=p(big), right=p(big), u8=1, ws=p(ws), out=p(out), B=B, H=H, W=W, D=D, p1=10, p2=120, uniq=95, lr_tol=1, paths=8, median=1, scale=2, stream=None)
    bad = [(dict(scale=0), MH_ERR_ARG), (dict(scale=3), MH_ERR_ARG), (dict(scale=-1), MH_ERR_ARG), (dict(D=64), MH_ERR_ARG), (dict(D=192), MH_ERR_ARG),
           (dict(H=12), MH_ERR_ARG), (dict(W=16), MH_ERR_ARG), (dict(paths=6), MH_ERR_ARG), (dict(median=2), MH_ERR_ARG), (dict(scale=1, D=256), MH_ERR_ARG),
           (dict(scale=1, H=6), MH_ERR_ARG), (dict(left=None), MH_ERR_ARG), (dict(out=None), MH_ERR_ARG), (dict(p1=0), MH_ERR_ARG), (dict(uniq=101), MH_ERR_ARG),
           (dict(ws=C.c_void_p(ws.data_ptr() + 8)), MH_ERR_ALIGN), (dict(scale=1, ws=C.c_void_p(ws.data_ptr() + 8)), MH_ERR_ALIGN)]
    for change, code in bad:
        a = dict(good, **change)
        assert lib._raw_mh_sgm_proxy_scaled(*a.values()) == code, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_sgm_proxy_scaled: ") and len(msg) > len("mh_sgm_proxy_scaled: "), (change, msg)
    backend.sync()
    assert bool((out == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_sgm_proxy_scaled(*good.values()) == 0
    backend.sync()
    assert bool((out[:B * H * W] == 0).all()) and bool((out[B * H * W:] == -7.0).all())      # flat frames: d1 = 0 everywhere -> rejected, every element written
    short = torch.empty(lib.sgm_ws_bytes_scaled(B, H, W, D, 8, 1, 2) - 1, dtype=torch.uint8, device=dev)
    o2 = torch.full((B, H, W), -7.0, device=dev)
    with pytest.raises(AssertionError, match="workspace too small"):
        ops.sgm_proxy(lib, l, l, short, o2, D, paths=8, median=True, scale=2)
    with pytest.raises(AssertionError, match="workspace too small"):
        ops.sgm_proxy(lib, l, l, ops.sgm_proxy_ws(lib, B, H, W, D, dev, scale=2), o2, D, scale=1)      # the scale 2 workspace is an eighth of what scale 1 needs
    backend.sync()
    assert bool((o2 == -7.0).all())


# ---- 6. through ProxyMatcher -------------------------------------------------------------------------------------------------------------------------
def test_matcher_scale_2_with_speckle_filter(backend):
    """the filter runs on the full-resolution map with the same size and max_diff = 2 x speckle_range"""
    lib, dev = backend.lib, backend.device
    name = "1x40x256_D128"
    B, H, W, D = CASES[name]
    l, r = frames(name)
    lt, rt = torch.from_numpy(np.array(l)).to(dev), torch.from_numpy(np.array(r)).to(dev)
    m = ProxyMatcher(lib, B, H, W, max_disp=D, device=dev, scale=2, speckle_size=40, speckle_range=1.0)
    assert m.scale == 2 and m.max_disp == D and m.ws.numel() == lib.sgm_ws_bytes_scaled(B, H, W, D, 4, 0, 2)
    assert m.speckle_ws.numel() == lib.sgm_speckle_ws_bytes(B, H, W) and m.speckle_range == 1.0
    got = m.compute(lt, rt)
    backend.sync()
    got = got.cpu().numpy()
    plain = SC.up2(half_labels(name, 4, 0), H, W)
    ref = SO.speckle(plain, 40, 2.0)
    print("valid labels: %d unfiltered, %d filtered" % ((plain > 0).sum(), (ref > 0).sum()))
    assert 0 < (ref > 0).sum() < (plain > 0).sum()
    assert not np.array_equal(ref > 0, SO.speckle(plain, 40, 1.0) > 0), "the range does not matter on this frame"
    check(got, ref)


def test_matcher_scale_1_gives_todays_bits(backend):
    lib, dev = backend.lib, backend.device
    name = "1x40x256_D128"
    B, H, W, D = CASES[name]
    l, r = frames(name)
    lt, rt = torch.from_numpy(np.array(l)).to(dev), torch.from_numpy(np.array(r)).to(dev)
    m = ProxyMatcher(lib, B, H, W, max_disp=D, device=dev, scale=1, paths=8, median=True)
    d = ProxyMatcher(lib, B, H, W, max_disp=D, device=dev, paths=8, median=True)
    assert m.scale == d.scale == 1 and m.ws.numel() == d.ws.numel() == lib.sgm_ws_bytes_ex(B, H, W, D, 8, 1) and m.params == d.params
    got = m.compute(lt, rt)
    direct = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib.sgm_proxy_ex(p(lt), p(rt), 1, p(d.ws), p(direct), B, H, W, D, 10, 120, 95, 1, 8, 1, None)
    backend.sync()
    assert (direct > 0).any()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), direct.cpu().numpy().view(np.uint32))
    with pytest.raises(AssertionError, match="scale"):
        ProxyMatcher(lib, B, H, W, max_disp=D, device=dev, scale=3)
    with pytest.raises(AssertionError, match="128, 256 or 384"):
        ProxyMatcher(lib, B, H, W, max_disp=64, device=dev, scale=2)


# ---- 7. what the option costs in label quality, on the oracle ---------------------------------------------------------------------------------------
def _quality(out, gt):
    valid = out > 0
    both = valid & (gt > 0)
    err = np.abs(out - gt)[both]
    return valid.mean(), (err > 3).mean(), err.mean()


def test_oracle_quality_of_half_resolution_labels():
    """Asserted on the oracle only (no library, no backend); the equality tests above carry it over to the kernels.  Four paths, D = 128, stream_id = 0.
    96 x 320: the oracle gives valid / bad3 / EPE 0.862 / 0.0330 / 1.105 at half resolution (0.825 / 0.0215 / 0.817 at full); the caps sit about 20 % beyond
    those deterministic numbers: they gate a changed definition, not noise.  40 x 256: 0.721 / 0.1316 / 2.289 against 0.675 / 0.0516 / 1.201 -- on frames a few
    dozen rows high the option is clearly worse, and that stays visible."""
    l, r, gt = S.make_pair(96, 320, stream_id=0)
    q = _quality(SC.sgm_proxy_scaled(l.astype(np.uint8), r.astype(np.uint8), 128, paths=4)[0], gt[0, :, :, 0])
    print("96x320 half resolution: valid %.3f  bad3 %.4f  EPE %.3f" % q)
    assert q[0] >= 0.84 and q[1] <= 0.04 and q[2] <= 1.3
    l, r = frames("1x40x256_D128")
    gt = S.make_pair(40, 256, stream_id=0)[2][0, :, :, 0]
    qh = _quality(SC.up2(half_labels("1x40x256_D128", 4, 0), 40, 256)[0], gt)
    qf = _quality(sgm8_oracle.sgm_proxy(l, r, 128, paths=4)[0], gt)
    print("40x256: full resolution valid %.3f  bad3 %.4f  EPE %.3f;  half resolution valid %.3f  bad3 %.4f  EPE %.3f" % (qf + qh))
    assert qh[1] > qf[1]
