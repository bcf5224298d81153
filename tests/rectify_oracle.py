"""Host statements of mh_rectify_map and mh_remap (include/madnet_hip.h) for tests/test_rectify.py: the fp32 statement in numpy, operation by operation in the
header's order (numpy rounds every float32 operation once and fuses nothing), and the float64 yardstick -- the same formula in float64 on the parameters as fp32
holds them.  A camera is a dict {"K": 3x3, "D": up to 5, "R": 3x3, "P": 3x3 / 3x4}."""
import numpy as np

INVALID = -2.0


def rot(ax_deg, ay_deg, az_deg):
    """R = Rz Ry Rx, float64"""
    ax, ay, az = (np.deg2rad(v) for v in (ax_deg, ay_deg, az_deg))
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ ry @ rx


def fields(cam, dtype):
    """the 22 numbers of mh_camera_model as fp32 holds them, in `dtype`"""
    K, R, P = (np.asarray(cam[k], np.float64) for k in ("K", "R", "P"))
    D = list(np.asarray(cam.get("D", []), np.float64).reshape(-1)) + [0.0] * 5
    f = dict(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], k1=D[0], k2=D[1], p1=D[2], p2=D[3], k3=D[4], fxn=P[0, 0], fyn=P[1, 1], cxn=P[0, 2], cyn=P[1, 2])
    f = {k: dtype(np.float32(v)) for k, v in f.items()}
    f["R"] = [dtype(np.float32(v)) for v in R.reshape(-1)]
    return f


def rectify_map(cam, Ho, Wo, dtype):
    """[Ho,Wo,2] in `dtype` (np.float32: the fp32 statement; np.float64: the yardstick), the header's association"""
    c = fields(cam, dtype)
    R = c["R"]
    one, two = dtype(1.0), dtype(2.0)
    with np.errstate(all="ignore"):
        u = np.broadcast_to(np.arange(Wo, dtype=dtype)[None, :], (Ho, Wo))
        v = np.broadcast_to(np.arange(Ho, dtype=dtype)[:, None], (Ho, Wo))
        x = (u - c["cxn"]) / c["fxn"]
        y = (v - c["cyn"]) / c["fyn"]
        X = (R[0] * x + R[3] * y) + R[6]
        Y = (R[1] * x + R[4] * y) + R[7]
        W = (R[2] * x + R[5] * y) + R[8]
        xp = X / W
        yp = Y / W
        xx, yy, xy = xp * xp, yp * yp, xp * yp
        r2 = xx + yy
        r4 = r2 * r2
        r6 = r4 * r2
        rad = ((one + c["k1"] * r2) + c["k2"] * r4) + c["k3"] * r6
        xd = (xp * rad + (two * c["p1"]) * xy) + c["p2"] * (r2 + two * xx)
        yd = (yp * rad + c["p1"] * (r2 + two * yy)) + (two * c["p2"]) * xy
        mx = c["fx"] * xd + c["cx"]
        my = c["fy"] * yd + c["cy"]
    ok = (W > 0) & np.isfinite(mx) & np.isfinite(my)
    out = np.stack([np.where(ok, mx, dtype(INVALID)), np.where(ok, my, dtype(INVALID))], -1)
    assert out.dtype == dtype
    return out, W


def _taps(src, y, x):
    """src [Hs,Ws,C] -> [..., C] at integer arrays (y, x); 0 outside"""
    Hs, Ws = src.shape[:2]
    inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
    s = src[np.where(inside, y, 0), np.where(inside, x, 0)]
    return np.where(inside[..., None], s, src.dtype.type(0))


def remap(src, map_, dtype):
    """src [V,Hs,Ws,Cs] (any dtype; Cs 1, 3, 4), map_ [V,Ho,Wo,2] float32 -> [V,Ho,Wo,3] in `dtype`: the header's bilinear statement"""
    V, Hs, Ws, Cs = src.shape
    s3 = src[..., [0, 0, 0]] if Cs == 1 else src[..., :3]
    s3 = s3.astype(dtype)
    out = np.zeros(map_.shape[:3] + (3,), dtype)
    one = dtype(1.0)
    for i in range(V):
        mx, my = map_[i, ..., 0].astype(dtype), map_[i, ..., 1].astype(dtype)
        with np.errstate(all="ignore"):
            live = (mx > -1) & (mx < Ws) & (my > -1) & (my < Hs)
        mx, my = np.where(live, mx, dtype(0)), np.where(live, my, dtype(0))
        x0f, y0f = np.floor(mx), np.floor(my)
        tx, ty = (mx - x0f)[..., None], (my - y0f)[..., None]
        ux, uy = one - tx, one - ty
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        s00, s01, s10, s11 = _taps(s3[i], y0, x0), _taps(s3[i], y0, x0 + 1), _taps(s3[i], y0 + 1, x0), _taps(s3[i], y0 + 1, x0 + 1)
        top = s00 * ux + s01 * tx
        bot = s10 * ux + s11 * tx
        o = top * uy + bot * ty
        assert o.dtype == dtype
        out[i] = np.where(live[..., None], o, dtype(0))
    return out


def ulp32(y):
    """the spacing of float32 at |y| (y: float64 array)"""
    return np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)


def within_rule(kernel, stmt32, y64):
    """the rule of tests/test_frame_prepare.py: the kernel's distance from the float64 yardstick is at most 2x the fp32 statement's (max abs over the case), or one
    float32 ulp of the value where the statement's distance is 0.  -> (ok, statement distance, kernel distance)"""
    k, s = kernel.astype(np.float64), stmt32.astype(np.float64)
    host_d, kern_d = float(np.abs(s - y64).max()), float(np.abs(k - y64).max())
    if host_d > 0:
        return kern_d <= 2.0 * host_d, host_d, kern_d
    return bool(np.all(np.abs(k - y64) <= ulp32(y64))), host_d, kern_d
