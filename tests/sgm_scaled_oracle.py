"""The numpy restatement of mh_sgm_proxy_scaled at scale 2 (include/madnet_hip.h) on top of tests/sgm8_oracle.py (no tests here): the 2 x 2 mean of the gray
frame in integers, today's matcher on the half frame over D / 2 disparities, every label doubled and written to its 2 x 2 pixels.  No library."""
import numpy as np

import sgm8_oracle
import sgm_oracle


def half_gray(img):
    """[H,W,3] uint8, or float32 holding 0..255 -> uint8 [(H + 1) // 2, (W + 1) // 2]: (g(2y, 2x) + g(2y, x1) + g(y1, 2x) + g(y1, x1) + 2) >> 2 of the gray g of
    sgm_oracle.gray, x1 = min(2x + 1, W - 1), y1 = min(2y + 1, H - 1)"""
    g = sgm_oracle.gray(img)
    H, W = g.shape
    y0, x0 = np.arange(0, H, 2), np.arange(0, W, 2)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    s = g[y0][:, x0] + g[y0][:, x1] + g[y1][:, x0] + g[y1][:, x1]
    return ((s + 2) >> 2).astype(np.uint8)


def as_rgb(g2):
    """a gray image as the RGB image whose three channels equal it (77 + 150 + 29 = 256: its gray is itself)"""
    return np.ascontiguousarray(np.repeat(np.asarray(g2)[..., None], 3, axis=-1))


def up2(l, H, W):
    """[..., h, w] labels -> float32 [..., H, W]: out(y, x) = 2 l(y >> 1, x >> 1) where that label is > 0, else 0"""
    l = np.asarray(l, dtype=np.float32)
    d = np.where(l > 0, np.float32(2) * l, np.float32(0)).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(d, 2, axis=-2), 2, axis=-1)[..., :H, :W])


def half_stage(left, right, D, paths=4, median=0, p1=10, p2=120, uniq=95, lr_tol=1, before_median=False):
    """left, right [B,H,W,3] -> the half-resolution labels float32 [B,h,w] of the matcher over D / 2 disparities"""
    assert D in (128, 256, 384)
    gl = np.stack([as_rgb(half_gray(a)) for a in left])
    gr = np.stack([as_rgb(half_gray(a)) for a in right])
    return sgm8_oracle.sgm_proxy(gl, gr, D // 2, p1=p1, p2=p2, uniq=uniq, lr_tol=lr_tol, paths=paths, median=0 if before_median else median)


def sgm_proxy_scaled(left, right, D=128, paths=4, median=0, **kw):
    """left, right [B,H,W,3] -> float32 [B,H,W]; 0 = rejected"""
    H, W = np.asarray(left).shape[1:3]
    return up2(half_stage(left, right, D, paths, median, **kw), H, W)
