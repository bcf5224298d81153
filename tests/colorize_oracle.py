"""numpy statement of mh_colorize, written from the text of include/madnet_hip.h ("preprocessing.colorize_img ... fused with the float -> uint8
normalisation"): every step one float32 operation or a table read, so a kernel that follows the header gives these bytes exactly.  No library is
loaded here and no test lives here."""
import numpy as np

F = np.float32
BAD = 256

# the header's (x, y) points of `jet`, per channel
_JET = (((0, 0), (.35, 0), (.66, 1), (.89, 1), (1, .5)),
        ((0, 0), (.125, 0), (.375, 1), (.64, 1), (.91, 0), (1, 0)),
        ((0, .5), (.11, 1), (.34, 1), (.65, 0), (1, 0)))


def _piecewise(points, n=256):
    """the header's piecewise-linear map in float64: entry 0 the first y, entry n - 1 the last, between them the segment whose right end is the first
    with 255 xb >= 255 x_i"""
    p = np.array(points, dtype=np.float64)
    x, y = p[:, 0] * (n - 1), p[:, 1]
    xi = (n - 1) * np.linspace(0, 1, n)
    out = np.empty(n)
    out[0], out[-1] = y[0], y[-1]
    for i in range(1, n - 1):
        k = int(np.searchsorted(x, xi[i]))
        out[i] = (xi[i] - x[k - 1]) / (x[k] - x[k - 1]) * (y[k] - y[k - 1]) + y[k - 1]
    return out


def table(cmap):
    """float32 [256][3]; cmap 0 = gray, 1 = jet"""
    if cmap == 0:
        g = np.arange(256, dtype=F) / F(255.0)
        return np.stack([g, g, g], 1)
    return np.stack([_piecewise(c) for c in _JET], 1).astype(F)


def codes(value, vmin=None, vmax=None):
    """step 1: idx per pixel, BAD for a non-finite value.  value: float32 [B,H,W]"""
    v = np.asarray(value, dtype=F)
    fin = np.isfinite(v)
    if vmin is None:
        vmin, vmax = (v[fin].min(), v[fin].max()) if fin.any() else (F(np.inf), F(-np.inf))
    vmin, vmax = F(vmin), F(vmax)
    out = np.zeros(v.shape, dtype=np.int64)
    if vmax != vmin:
        with np.errstate(all="ignore"):
            n = (v - vmin).astype(F) / F(vmax - vmin)
            t = np.rint((n * F(255.0)).astype(F))
        out = np.where(t >= 255, 255, np.where(t > 0, np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0), 0)).astype(np.int64)
    out[~fin] = BAD
    return out


def colorize(value, cmap, out_kind, vmin=None, vmax=None):
    """out_kind 0 -> float32 [B,H,W,3]; out_kind 1 -> uint8 [H,W,3] of image 0"""
    lut = table(cmap)
    k = codes(value, vmin, vmax)
    bad = k == BAD
    rgb = lut[np.where(bad, 0, k)]
    if out_kind == 0:
        rgb = rgb.copy()
        rgb[bad] = (1.0, 0.0, 0.0)
        return rgb
    rgb, bad = rgb[0], bad[0]
    image_max = rgb[~bad].max() if (~bad).any() else F(0)
    scale = F(0) if image_max < F(1e-6) else F(255.0) / F(image_max)
    out = (rgb * scale).astype(F).astype(np.uint8)
    out[bad] = (255, 0, 0)
    return out
