"""Rectifier.valid_masks: which pixels of a rectified (rescaled, cropped / padded) frame show something, and the live demo's mask_invalid run.

A rectified pixel is valid when its map position lies inside the raw view (0 <= mx <= Ws - 1, 0 <= my <= Hs - 1); the 0/1 image goes through the frames' own
rescale_image and crop_or_pad and stays valid where the result is >= 1 - 1e-5.  Checked against what an all-255 frame pair reads after Rectifier.apply: 255 (to
1e-5) exactly where the mask is 1, nothing claimed valid that reads less.  The synthetic calibration is the `distort` pair of tests/test_rectify.py (re-stated
here): strong distortion, rotations and a rectified focal length that makes the output window hang over every edge of the 37 x 53 source."""
import os
import queue
import sys

import numpy as np
import pytest
import torch

import rectify_oracle as RO
from madnet_hip import rectify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
DEMO = os.path.join(PKG, "Demo")
if DEMO not in sys.path:
    sys.path.insert(0, DEMO)

RAW = (37, 53)
OUT_SIZES = [(41, 67), (16, 24), (70, 80)]


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)


def _calibration(Ho, Wo):
    raw = [_K(44.0, 46.0, 25.3, 17.6), _K(41.0, 40.0, 27.1, 19.2)]
    D = [[-0.35, 0.10, 0.012, -0.009, -0.015], [0.40, 0.20, -0.012, 0.015, 0.05]]
    R = [RO.rot(3.0, -4.0, 2.5), RO.rot(-2.0, 3.0, -3.0)]
    P = [_K(0.45 * k[0, 0] * (Wo - 1) / 52.0, 0.45 * k[1, 1] * (Ho - 1) / 36.0, (Wo - 1) / 2.0 + 0.7, (Ho - 1) / 2.0 - 0.4) for k in raw]
    views = [{"K": raw[i], "D": D[i], "R": R[i], "P": P[i]} for i in range(2)]
    return {"size": list(RAW), "out_size": [Ho, Wo], "left": views[0], "right": views[1]}


def _white(dev):
    return torch.full((2, RAW[0], RAW[1], 3), 255, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("size", OUT_SIZES, ids=lambda s: "%dx%d" % s)
def test_mask_is_where_a_white_pair_reads_white(backend, size):
    Ho, Wo = size
    rc = rectify.Rectifier(backend.lib, _calibration(Ho, Wo), backend.device)
    vl, vr = rc.valid_masks()
    assert vl.dtype == torch.uint8 and tuple(vl.shape) == (1, Ho, Wo) == tuple(vr.shape) and str(vl.device).startswith(str(backend.device)[:3])
    out = rc.apply(_white(backend.device))
    backend.sync()
    lo = out.min(dim=-1).values.cpu()                      # [2,Ho,Wo]: the darkest channel
    v = torch.cat([vl, vr]).cpu()
    white, black = lo >= 255.0 * (1 - 1e-5), out.max(dim=-1).values.cpu() == 0
    print("%dx%d: valid %d + %d of %d, black %d, in between %d" % (Ho, Wo, int(v[0].sum()), int(v[1].sum()), Ho * Wo, int(black.sum()), int((~white & ~black).sum())))
    assert torch.equal(v != 0, white)                      # 1 exactly where the pair reads 255, so 0 where it reads 0 and nothing in between is claimed valid
    assert bool((v[black] == 0).all()) and bool(black.any()) and bool((~white & ~black).any()) and bool(white[0].any()) and bool(white[1].any())
    assert set(v.unique().tolist()) == {0, 1}


def test_uploaded_map_view_follows_the_same_rule(backend):
    Ho, Wo = 9, 12
    m = np.zeros((Ho, Wo, 2), np.float32)
    m[..., 0] = np.linspace(-1.5, RAW[1] + 0.5, Wo)[None, :]
    m[..., 1] = np.linspace(-0.25, RAW[0] - 1.0, Ho)[:, None]           # the last row sits exactly on the last source row: valid
    cal = _calibration(Ho, Wo)
    cal["right"] = {"map": m}
    rc = rectify.Rectifier(backend.lib, cal, backend.device)
    vr = rc.valid_masks()[1].cpu()[0]
    ref = (m[..., 0] >= 0) & (m[..., 0] <= RAW[1] - 1) & (m[..., 1] >= 0) & (m[..., 1] <= RAW[0] - 1)
    assert np.array_equal(vr.numpy() != 0, ref) and ref[-1].any() and not ref[0].any() and not ref.all()


def test_pad_is_invalid_and_rescale_invalidates_every_touched_pixel(backend, monkeypatch):
    from Data_utils import preprocessing as P
    monkeypatch.setattr(P, "_lib", lambda: backend.lib)
    Ho, Wo = 41, 67
    rc = rectify.Rectifier(backend.lib, _calibration(Ho, Wo), backend.device)
    plain = torch.cat(rc.valid_masks()).cpu()
    # a crop shape larger than the frame: the pad is invalid, the frame keeps its mask
    th, tw = Ho + 6, Wo + 11
    v = torch.cat(rc.valid_masks(None, (th, tw))).cpu()
    pt, pl = (th - Ho) // 2, (tw - Wo) // 2
    assert tuple(v.shape) == (2, th, tw) and torch.equal(v[:, pt:pt + Ho, pl:pl + Wo], plain)
    inner = torch.zeros(th, tw, dtype=torch.bool)
    inner[pt:pt + Ho, pl:pl + Wo] = True
    assert not v[:, ~inner].any()
    # rescale, then crop in one direction and pad in the other -- the frames' own way: where the mask is 1 the white pair still reads 255, where the pair reads
    # 0 the mask is 0
    image_shape, crop_shape = (30, 50), (24, 56)
    import demo_model
    v = torch.cat(rc.valid_masks(image_shape, crop_shape)).cpu()
    x = demo_model.crop_or_pad(P.rescale_image(rc.apply(_white(backend.device)), image_shape), *crop_shape)
    backend.sync()
    lo, hi = x.min(dim=-1).values.cpu(), x.max(dim=-1).values.cpu()
    assert tuple(v.shape) == (2, 24, 56) == tuple(lo.shape)
    assert bool((lo[v != 0] >= 255.0 * (1 - 2e-5)).all()) and not v[hi == 0].any() and bool((v != 0).any()) and bool((hi == 0).any())
    assert not v[:, :, :3].any() and not v[:, :, 53:].any()         # the pad of the width 50 -> 56


# ---- the live demo with mask_invalid ------------------------------------------------------------------------------------------------------------------------------
def _shift_calibration(h, w, shift):
    """the exact pinhole pair of tests/test_rectify_demo.py: rectified pixel u shows raw pixel u + shift, the last `shift` columns have no source"""
    K = [[64.0, 0.0, float(w // 2)], [0.0, 64.0, float(h // 2)], [0.0, 0.0, 1.0]]
    Pm = [[64.0, 0.0, float(w // 2 - shift), 0.0], [0.0, 64.0, float(h // 2), 0.0], [0.0, 0.0, 1.0, 0.0]]
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    view = {"K": K, "D": [0.0, 0.0, 0.0, 0.0, 0.0], "R": eye, "P": Pm}
    return {"size": [h, w], "left": view, "right": dict(view)}


def _run_loop(lib, device, n_frames, monkeypatch, cam, crop_shape, **kw):
    import demo_model
    import grabber
    from Data_utils import preprocessing as P
    if lib is not None:
        monkeypatch.setattr(P, "_lib", lambda: lib)
    q = queue.Queue(1)
    dd = demo_model.RealTimeStereo(q, model_name="MADNet", weight_path="calibrated:1", learning_rate=1e-4,
                                   block_config_path=os.path.join(PKG, "block_config", "MadNet_full.json"), image_shape=[-1], crop_shape=crop_shape, SSIMTh=10.0,
                                   mode="FULL", device=device, max_frames=n_frames, _lib=lib, **kw)
    gg = grabber.get_camera("Synthetic", q, config={"height": cam[0], "width": cam[1], "distinct": 2}, framerate=0)
    gg.start(); dd.start()
    dd.join(600)
    gg.stop(); gg.join(10)
    assert not dd.is_alive() and not gg.is_alive()
    if dd.error is not None:
        raise dd.error
    return dd


def _demo(lib, device, monkeypatch, cam, crop):
    cal = _shift_calibration(cam[0], cam[1], 5)
    runs = [_run_loop(lib, device, 3, monkeypatch, cam, crop, calibration=cal, mask_invalid=m) for m in (False, True)]
    plain, masked = ([h[0] for h in dd.history] for dd in runs)
    print("losses without masks %r, with %r" % (plain, masked))
    assert len(plain) == 3 == len(masked) and all(np.isfinite(plain)) and all(np.isfinite(masked))
    assert all(a != b for a, b in zip(plain, masked))
    vl, vr = runs[1]._net.engine.valid
    pt, pl = (crop[0] - cam[0]) // 2, (crop[1] - cam[1]) // 2
    ref = torch.zeros(1, crop[0], crop[1], dtype=torch.uint8)
    ref[:, pt:pt + cam[0], pl:pl + cam[1] - 5] = 1                   # the frame inside the pad, without the 5 columns that have no source
    assert torch.equal(vl.cpu(), ref) and torch.equal(vr.cpu(), ref) and runs[0]._net.engine.valid is None


@pytest.mark.slow
def test_demo_with_mask_invalid_emulated(monkeypatch):
    from conftest import _emul_backend
    _demo(_emul_backend().lib, "cpu", monkeypatch, (40, 56), [48, 64])


@pytest.mark.gpu
def test_demo_with_mask_invalid_gpu(hip, monkeypatch):
    _demo(None, "cuda", monkeypatch, (56, 96), [64, 112])
