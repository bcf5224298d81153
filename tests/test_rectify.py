"""mh_rectify_map / mh_remap, op level, and madnet_hip.rectify on top of them -- on the CPU emulator and, marked gpu, on the product library.

Tolerance: no chosen number (the rule of tests/test_frame_prepare.py).  The yardstick is a float64 evaluation of the header's formula on the parameters as fp32
holds them (tests/rectify_oracle.py); the numpy-fp32 statement of the same formula, operation by operation in the header's order, is measured against it per case
(max abs over every pixel of both views, none excluded), and the kernel has to stay within 2x that distance -- or within one float32 ulp of the coordinate where
that distance is 0.  The remap is compared at the KERNEL's own map, so that coordinate error is not mixed in.

Measured (max abs distance from the float64 yardstick, statement / kernel; the emulator and the MI355X print the same figure in every case, and in every case the
kernel's bits EQUAL the numpy-fp32 statement's -- asserted nowhere, the rule above is the test):
  map, distortion cases (raw pixels)     41x67 2.66e-4 / 2.66e-4    16x24 3.39e-4 / 3.39e-4    5x7 2.25e-4 / 2.25e-4    70x80 3.27e-4 / 3.27e-4
  map, W <= 0 cases (raw pixels)         41x67 1.12e-3 / 1.12e-3    16x24 1.04e-4 / 1.04e-4    5x7 2.10e-5 / 2.10e-5    70x80 3.95e-3 / 3.95e-3
                                         (coordinates of up to 4156 pixels next to the W = 0 line; exactly (-2, -2) behind it; the distortion cases reach 600 .. 1200 in the overhang)
  remap (0..255 scale)                   uint8 and float32 sources, Cs 1 / 3 / 4, 19x23 and 16x24: 2.10e-5 .. 2.68e-5 / the same figure in each of the 12 cases
  exact cases                            0 / 0: the map is (u, v) bit for bit, the remap the cast of the frame
  stereo_calibration (float64, host)     rows |v_l - v_r| <= 1.14e-13 px, |(u_l - u_r) - f |T| / Z| <= 1.39e-13 px = 1.23 eps f, against the bound of 64 eps f
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import footprint as FP
import rectify_oracle as RO
from madnet_hip import _ffi, ops, rectify

RAW = (37, 53)
OUT_SIZES = [(41, 67), (16, 24), (5, 7), (70, 80)]          # 16x24: aligned quads; 41x67, 5x7: odd pixel counts (view 1 starts off a 16-byte boundary, partial quads;
                                                            # 5x7 is less than one workgroup); 70x80: 6 remap / 22 map workgroups per view


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _cams(Ho, Wo, kind):
    """two views with different models for an Ho x Wo rectified frame of the 37x53 raw views"""
    if kind == "distort":
        # view 0: strong barrel, view 1: strong pincushion; both tangential terms; a few degrees about every axis; a rectified focal length of 0.45x the raw one
        # (scaled to the span of the output's pixel centres), so that the output window hangs over every edge of the source
        raw = [_K(44.0, 46.0, 25.3, 17.6), _K(41.0, 40.0, 27.1, 19.2)]
        D = [[-0.35, 0.10, 0.012, -0.009, -0.015], [0.40, 0.20, -0.012, 0.015, 0.05]]
        R = [RO.rot(3.0, -4.0, 2.5), RO.rot(-2.0, 3.0, -3.0)]
        P = [_K(0.45 * k[0, 0] * (Wo - 1) / 52.0, 0.45 * k[1, 1] * (Ho - 1) / 36.0, (Wo - 1) / 2.0 + 0.7, (Ho - 1) / 2.0 - 0.4) for k in raw]
    else:
        # "wneg": rotations so large that W = (R^T (x, y, 1))_z changes sign inside the frame: view 0 about y (left of u = Wo / 4 + 0.37), view 1 about x (below
        # v = 0.644 Ho + 0.37); the offsets keep the W = 0 line between two pixels, so no pixel has a W that is rounding noise
        raw = [_K(44.0, 46.0, 25.3, 17.6), _K(41.0, 40.0, 27.1, 19.2)]
        D = [[], [0.0, 0.0]]                               # (shorter than 5: the missing terms are 0)
        R = [RO.rot(0.0, 45.0, 0.0), RO.rot(60.0, 0.0, 0.0)]
        P = [_K(Wo / 4.0, Ho / 4.0, Wo / 2.0 + 0.37, Ho / 2.0 + 0.37) for _ in raw]
    return [{"K": raw[i], "D": D[i], "R": R[i], "P": P[i]} for i in range(2)]


def _model(cam):
    return ops.camera_model(cam["K"].tolist(), list(cam["D"]), np.asarray(cam["R"]).tolist(), np.asarray(cam["P"]).tolist())


def _kernel_map(backend, cams, Ho, Wo):
    """the map of mh_rectify_map inside guards, twice: same bits, every element written"""
    got = []
    for _ in range(2):
        g = FP.Guarded(len(cams) * Ho * Wo * 2, device=backend.device)
        ops.rectify_map(backend.lib, [_model(c) for c in cams], g.t.view(len(cams), Ho, Wo, 2))
        backend.sync()
        FP.assert_fully_written(g, g.n, "rectify_map output")
        got.append(g.t.view(len(cams), Ho, Wo, 2).cpu().numpy())
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "two calls differ"
    return got[0]


def _kernel_remap(backend, src, map_):
    V, Ho, Wo = map_.shape[:3]
    s, m = torch.from_numpy(src).to(backend.device), torch.from_numpy(map_).to(backend.device)
    got = []
    for _ in range(2):
        g = FP.Guarded(V * Ho * Wo * 3, device=backend.device)
        ops.remap(backend.lib, s, m, g.t.view(V, Ho, Wo, 3))
        backend.sync()
        FP.assert_fully_written(g, g.n, "remap output")
        got.append(g.t.view(V, Ho, Wo, 3).cpu().numpy())
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "two calls differ"
    return got[0]


@pytest.mark.parametrize("kind", ["distort", "wneg"])
@pytest.mark.parametrize("size", OUT_SIZES, ids=["%dx%d" % s for s in OUT_SIZES])
def test_map_against_the_float64_formula(backend, size, kind):
    Ho, Wo = size
    cams = _cams(Ho, Wo, kind)
    k = _kernel_map(backend, cams, Ho, Wo)
    s32, y64, w64 = [], [], []
    for c in cams:
        a, _ = RO.rectify_map(c, Ho, Wo, np.float32)
        b, w = RO.rectify_map(c, Ho, Wo, np.float64)
        s32.append(a); y64.append(b); w64.append(w)
    s32, y64, w64 = np.stack(s32), np.stack(y64), np.stack(w64)
    Hs, Ws = RAW
    if kind == "distort":
        assert (w64 > 0).all()
        for i in range(2):                                  # the window hangs over every edge of the source
            assert y64[i, ..., 0].min() < -1 and y64[i, ..., 0].max() > Ws and y64[i, ..., 1].min() < -1 and y64[i, ..., 1].max() > Hs, i
    else:
        bad = w64 <= 0
        assert all(bad[i].any() and not bad[i].all() for i in range(2)) and np.abs(w64).min() > 1e-3
        assert np.array_equal(k[bad], np.full((int(bad.sum()), 2), -2.0, np.float32)), "W <= 0 must give exactly (-2, -2)"
        assert not (k[~bad] == -2.0).all(-1).any()
    ok, host_d, kern_d = RO.within_rule(k, s32, y64)
    same = np.array_equal(k.view(np.uint32), s32.view(np.uint32))
    print("map %s %dx%d (%s): statement %.3g kernel %.3g from the float64 formula, same bits as the statement: %s" % (kind, Ho, Wo, backend.name, host_d, kern_d, same))
    assert ok, (kind, size, host_d, kern_d)


def _handmade_map(Ho, Wo, Hs, Ws, seed):
    """[2,Ho,Wo,2]: random positions from 3 pixels outside to 3 pixels outside, and in the first rows the cases the issue names"""
    rng = np.random.default_rng(seed)
    m = np.stack([rng.uniform(-3.0, Ws + 2.0, (2, Ho, Wo)), rng.uniform(-3.0, Hs + 2.0, (2, Ho, Wo))], -1).astype(np.float32)
    special = [(4.0, 7.0), (0.0, 0.0), (Ws - 1.0, Hs - 1.0), (Ws - 1.0, 3.25), (10.5, Hs - 1.0), (Ws - 1.5, Hs - 1.25),      # integers, the last row and column
               (-0.25, 5.0), (6.5, -0.75), (-0.5, -0.5), (-0.999, Hs - 0.5), (Ws - 0.25, -0.125), (Ws - 0.5, Hs - 0.5),      # in (-1, 0) / the last partial cell
               (-1.0, 5.0), (5.0, -1.0), (float(Ws), 5.0), (5.0, float(Hs)), (-7.5, 4.0), (4.0, -9.0), (Ws + 30.0, 2.0), (3.0, Hs + 11.0),   # beyond every edge
               (-2.0, -2.0), (float("nan"), 3.0), (3.0, float("inf")), (-1e30, 1e30)]                                          # the mark; not finite; huge
    for v in range(2):
        for j, xy in enumerate(special):
            m[v, (j + 5 * v) // Wo, (j + 5 * v) % Wo] = xy
        m[v, -1, -1] = (Ws - 1.0, Hs - 1.0)
        m[v, -1, -2] = (-2.0, -2.0)
    return m


@pytest.mark.parametrize("cs", [1, 3, 4])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_remap_against_float64_bilinear(backend, dtype, cs):
    Hs, Ws = RAW
    rng = np.random.default_rng(7 + cs)
    src = rng.integers(0, 256, (2, Hs, Ws, cs), dtype=np.uint8) if dtype == "uint8" else (rng.random((2, Hs, Ws, cs)) * 255.0).astype(np.float32)
    worst = []
    for Ho, Wo in ((19, 23), (16, 24)):                     # 437 pixels per view: partial quad, view 1 unaligned; 384: the vector path in both views
        m = _handmade_map(Ho, Wo, Hs, Ws, seed=Ho)
        k = _kernel_remap(backend, src, m)
        s32, y64 = RO.remap(src, m, np.float32), RO.remap(src, m, np.float64)
        # what the hand-made entries must give whatever the arithmetic: exact source values, zeros
        c3 = [0, 0, 0] if cs == 1 else [0, 1, 2]
        assert np.array_equal(k[0, 0, 0], src[0, 7, 4][c3].astype(np.float32)) and np.array_equal(k[0, 0, 2], src[0, Hs - 1, Ws - 1][c3].astype(np.float32))
        assert np.array_equal(k[:, -1, -1], src[:, Hs - 1, Ws - 1][:, c3].astype(np.float32)) and not k[:, -1, -2].any()
        assert not k[0, 0, 12:24].any() if Wo >= 24 else not k[0, 0, 12:23].any()          # beyond the edges, the mark, the non-finite ones: nothing sampled
        assert k[0, 0, 6].any() and k[0, 0, 8].any()       # a coordinate in (-1, 0) still takes its inside tap
        assert np.isfinite(k).all()
        ok, host_d, kern_d = RO.within_rule(k, s32, y64)
        same = np.array_equal(k.view(np.uint32), s32.view(np.uint32))
        print("remap %s Cs %d %dx%d (%s): statement %.3g kernel %.3g from float64 bilinear, same bits as the statement: %s" % (dtype, cs, Ho, Wo, backend.name, host_d, kern_d, same))
        assert ok, (dtype, cs, Ho, Wo, host_d, kern_d)
        worst.append(kern_d)
    assert max(worst) < 1e-3                                # (sanity of the yardstick itself: float32 rounding of values <= 255)


def _exact_cams(shift=0.0):
    """every field a power of two or an integer, D = 0, R = I: every step of the formula is exact"""
    k = _K(64.0, 64.0, 26.0, 18.0)
    return [{"K": k, "D": [], "R": np.eye(3), "P": _K(64.0, 64.0, 26.0 - shift, 18.0)} for _ in range(2)]


def test_exact_identity_and_shift(backend):
    Hs, Ws = RAW
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)
    uv = np.stack(np.meshgrid(np.arange(Ws, dtype=np.float32), np.arange(Hs, dtype=np.float32)), -1)
    m = _kernel_map(backend, _exact_cams(), Hs, Ws)
    assert np.array_equal(m.view(np.uint32), np.stack([uv, uv]).view(np.uint32)), "the identity map must be (u, v) bit for bit"
    out = _kernel_remap(backend, src, m)
    assert np.array_equal(out, src.astype(np.float32)), "the remap at the identity map must be the cast of the frame"
    for cams in (_exact_cams(),):                           # ... and the yardstick agrees that nothing is lost: distance 0 -> the one-ulp branch of the rule
        y64 = np.stack([RO.rectify_map(c, Hs, Ws, np.float64)[0] for c in cams])
        s32 = np.stack([RO.rectify_map(c, Hs, Ws, np.float32)[0] for c in cams])
        ok, host_d, kern_d = RO.within_rule(m, s32, y64)
        assert ok and host_d == 0.0 and kern_d == 0.0
    m3 = _kernel_map(backend, _exact_cams(shift=3.0), Hs, Ws)
    assert np.array_equal(m3[..., 0], np.stack([uv[..., 0] + 3.0] * 2)) and np.array_equal(m3[..., 1], np.stack([uv[..., 1]] * 2))
    out3 = _kernel_remap(backend, src, m3)
    assert np.array_equal(out3[:, :, :Ws - 3], src[:, :, 3:].astype(np.float32)) and not out3[:, :, Ws - 3:].any()


def test_argument_errors_launch_nothing(backend):
    lib, dev = backend.lib, backend.device
    Hs, Ws = 6, 8
    cams = (_ffi.CameraModel * 4)(*[_model(c) for c in _exact_cams() + _exact_cams()])
    gm, go = FP.Guarded(2 * Hs * Ws * 2, device=dev), FP.Guarded(2 * Hs * Ws * 3, device=dev)
    src = torch.zeros(2, Hs, Ws, 3, dtype=torch.uint8, device=dev)
    before_m, before_o = gm.snapshot(), go.snapshot()
    p = lambda t: C.c_void_p(t.data_ptr())

    def bad_map(msg="mh_rectify_map", **kw):
        a = dict(cams=cams, V=2, Ho=Hs, Wo=Ws, map=p(gm.t))
        a.update(kw)
        assert lib._raw_mh_rectify_map(a["cams"], a["V"], a["Ho"], a["Wo"], a["map"], None) == -1 and msg in lib.last_error().decode(), kw       # MH_ERR_ARG

    bad_map(cams=None); bad_map(map=None)
    for v in (0, -1, 5):
        bad_map(V=v)
    for v in (0, -3):
        bad_map(Ho=v); bad_map(Wo=v)
    for field in ("fx", "fy", "fxn", "fyn"):
        for value in (0.0, float("nan"), float("inf"), -float("inf")):
            broken = (_ffi.CameraModel * 2)(*[_model(c) for c in _exact_cams()])
            setattr(broken[1], field, value)
            bad_map(cams=broken, msg="focal length")
    with pytest.raises(_ffi.MadnetHipError, match="mh_rectify_map"):
        lib.rectify_map(cams, 0, Hs, Ws, p(gm.t), None)

    def bad_remap(**kw):
        a = dict(src=p(src), u8=1, map=p(gm.t), out=p(go.t), V=2, Hs=Hs, Ws=Ws, Cs=3, Ho=Hs, Wo=Ws)
        a.update(kw)
        rc = lib._raw_mh_remap(a["src"], a["u8"], a["map"], a["out"], a["V"], a["Hs"], a["Ws"], a["Cs"], a["Ho"], a["Wo"], None)
        assert rc == -1 and "mh_remap" in lib.last_error().decode(), kw

    bad_remap(src=None); bad_remap(map=None); bad_remap(out=None)
    for v in (0, -1, 5):
        bad_remap(V=v)
    for name in ("Hs", "Ws", "Ho", "Wo"):
        for v in (0, -2):
            bad_remap(**{name: v})
    for v in (0, 2, 5, -1):
        bad_remap(Cs=v)
    bad_remap(V=2, Hs=32768, Ws=32769, Cs=1)               # 2^31 + 65536 source elements (2^31 exactly is legal)
    bad_remap(V=1, Hs=23171, Ws=23171, Cs=4)               # 4 x 23171^2 = 2^31 + 37316
    with pytest.raises(_ffi.MadnetHipError, match="mh_remap"):
        lib.remap(p(src), 1, p(gm.t), p(go.t), 2, Hs, Ws, 2, Hs, Ws, None)
    backend.sync()
    FP.assert_untouched(gm, before_m, "map after refused calls")
    FP.assert_untouched(go, before_o, "out after refused calls")
    assert C.sizeof(_ffi.CameraModel) == 22 * 4


def test_rectifier_class_json_and_uploaded_maps(backend, tmp_path):
    """Rectifier from a dict and from a JSON file; a view given as "map": file.npy takes that map as it is; apply() on uint8 and float32 frames of 3 and 4 channels"""
    Hs, Ws = RAW
    Ho, Wo = 16, 24
    cams = _cams(Ho, Wo, "distort")
    cal = {"size": [Hs, Ws], "out_size": [Ho, Wo], "left": {k: np.asarray(v).tolist() for k, v in cams[0].items()},
           "right": {k: np.asarray(v).tolist() for k, v in cams[1].items()}}
    r = rectify.Rectifier(backend.lib, cal, backend.device)
    backend.sync()
    direct = _kernel_map(backend, cams, Ho, Wo)
    assert np.array_equal(r.map.cpu().numpy().view(np.uint32), direct.view(np.uint32))
    np.save(str(tmp_path / "right_map.npy"), direct[1])
    cal2 = dict(cal, right={"map": "right_map.npy"})
    (tmp_path / "cal.json").write_text(json.dumps(cal2))
    r2 = rectify.Rectifier(backend.lib, str(tmp_path / "cal.json"), backend.device)
    assert torch.equal(r2.map, r.map)
    rng = np.random.default_rng(2)
    raw4 = rng.integers(0, 256, (2, Hs, Ws, 4), dtype=np.uint8)
    a = r.apply(torch.from_numpy(raw4).to(backend.device))
    b = r2.apply(torch.from_numpy(raw4[..., :3].astype(np.float32)).to(backend.device))
    backend.sync()
    assert a.shape == (2, Ho, Wo, 3) and a.dtype == torch.float32 and torch.equal(a, b)
    ok, _, _ = RO.within_rule(a.cpu().numpy(), RO.remap(raw4, direct, np.float32), RO.remap(raw4, direct, np.float64))
    assert ok
    with pytest.raises(ValueError, match="calibration is for"):
        r.apply(torch.zeros(2, Hs + 1, Ws, 3, dtype=torch.uint8, device=backend.device))
    with pytest.raises(ValueError, match="lacks"):
        rectify.Rectifier(backend.lib, {"size": [Hs, Ws], "left": cal["left"]}, backend.device)
    # a default out_size is the raw size; from_stereo builds the same thing from extrinsics
    r3 = rectify.Rectifier.from_stereo(cams[0]["K"], cams[0]["D"], cams[1]["K"], cams[1]["D"], RO.rot(0.5, -1.0, 0.3), [-0.1, 0.004, 0.002], RAW,
                                       lib=backend.lib, device=backend.device)
    assert tuple(r3.map.shape) == (2, Hs, Ws, 2) and r3.out_size == RAW


def test_stereo_calibration_rows_agree_and_disparity_is_f_baseline_over_depth():
    """Host side, float64.  A seeded cloud seen by two cameras that differ in focal length, are rotated against each other and have a skewed baseline; the pixels
    go through the inverse of each view's rectifying map (no distortion: p_rect ~ Kn R_i K_i^-1 p): the rows agree and u_l - u_r = f |T| / Z.
    Bound: a coordinate is reached through fewer than 30 float64 roundings, each at most eps / 2 relative on quantities no larger than 2 f (pixel coordinates stay
    below 1.3 f here), i.e. 30 eps f per coordinate and 60 eps f for a difference of two -- stated as 64 eps f.  Measured: rows 1.14e-13 px, disparity 1.39e-13 px =
    1.23 eps f (f = 509, eps f = 1.13e-13)."""
    K1, K2 = _K(520.0, 515.0, 318.0, 242.0), _K(498.0, 503.0, 330.0, 236.0)
    R, T = RO.rot(1.5, -2.5, 1.0), np.array([-0.12, 0.011, -0.007])
    cal = rectify.stereo_calibration(K1, [], K2, [], R, T, (480, 640))
    R1, R2, P1, P2 = (np.asarray(cal[s][k]) for s, k in (("left", "R"), ("right", "R"), ("left", "P"), ("right", "P")))
    Kn = P1[:, :3]
    f = Kn[0, 0]
    for Rm in (R1, R2):
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(Rm), 1.0)
    assert np.array_equal(Kn, P2[:, :3]) and Kn[0, 1] == 0.0 and np.allclose(Kn, 0.5 * (K1 + K2))
    assert np.isclose(P2[0, 3], -f * np.linalg.norm(T)) and not P1[:, 3].any()
    rng = np.random.default_rng(5)
    X1 = np.stack([rng.uniform(-1.0, 1.0, 300), rng.uniform(-0.8, 0.8, 300), rng.uniform(2.0, 8.0, 300)])
    X2 = R @ X1 + T[:, None]
    p1, p2 = K1 @ (X1 / X1[2]), K2 @ (X2 / X2[2])
    q1, q2 = Kn @ (R1 @ np.linalg.solve(K1, p1)), Kn @ (R2 @ np.linalg.solve(K2, p2))
    q1, q2 = q1 / q1[2], q2 / q2[2]
    Z = (R1 @ X1)[2]
    bound = 64 * np.finfo(np.float64).eps * f
    rows = float(np.abs(q1[1] - q2[1]).max())
    disp = float(np.abs((q1[0] - q2[0]) - f * np.linalg.norm(T) / Z).max())
    print("stereo_calibration: rows %.3g px, disparity %.3g px = %.2f eps f (bound 64 eps f = %.3g)" % (rows, disp, disp / (np.finfo(np.float64).eps * f), bound))
    assert (q1[0] - q2[0]).min() > 0
    assert rows <= bound and disp <= bound
