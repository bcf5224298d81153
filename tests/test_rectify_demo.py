"""The live demo on RAW camera pairs: RealTimeStereo(..., calibration=...) / Live_Adaptation_Demo.py --calibration rectify every frame pair on the device
(madnet_hip.rectify over mh_rectify_map / mh_remap) in front of rescale and crop.  Emulated like tests/test_live_demo.py (whose _run_loop this copies, with the
camera's size and the preparation's shapes as arguments); marked gpu, the CLI on the MI355X.

The exact calibration (focal lengths 64, integer principal points, no distortion, R = I) makes every step of the map formula exact: the map is (u, v), the remap
of an 8-bit frame is its cast, so the run must equal the run without a calibration bit for bit; with the rectified principal point 3 pixels to the left the
network must see the frames shifted by 3 pixels, zero-filled at the right edge."""
import json
import os
import queue
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
DEMO = os.path.join(PKG, "Demo")
if DEMO not in sys.path:
    sys.path.insert(0, DEMO)


def exact_calibration(h, w, shift=0):
    K = [[64.0, 0.0, float(w // 2)], [0.0, 64.0, float(h // 2)], [0.0, 0.0, 1.0]]
    P = [[64.0, 0.0, float(w // 2 - shift), 0.0], [0.0, 64.0, float(h // 2), 0.0], [0.0, 0.0, 1.0, 0.0]]
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    view = {"K": K, "D": [0.0, 0.0, 0.0, 0.0, 0.0], "R": eye, "P": P}
    return {"size": [h, w], "left": view, "right": dict(view)}


def _run_loop(lib, device, mode, n_frames, monkeypatch, cam, image_shape, crop_shape, **kw):
    import demo_model
    import grabber
    from Data_utils import preprocessing as P
    if lib is not None:
        monkeypatch.setattr(P, "_lib", lambda: lib)
    q = queue.Queue(1)
    seen = []
    dd = demo_model.RealTimeStereo(q, model_name="MADNet", weight_path="calibrated:1", learning_rate=1e-4,
                                   block_config_path=os.path.join(PKG, "block_config", "MadNet_full.json"), image_shape=image_shape,
                                   crop_shape=crop_shape, SSIMTh=kw.pop("SSIMTh", 10.0), mode=mode, device=device, max_frames=n_frames,
                                   on_frame=lambda it, rec, l, r, d: seen.append((it, rec, l.clone(), r.clone(), d.clone())), _lib=lib, **kw)
    gg = grabber.get_camera("Synthetic", q, config={"height": cam[0], "width": cam[1], "distinct": 2}, framerate=0)
    gg.start(); dd.start()
    dd.join(600)
    gg.stop(); gg.join(10)
    assert not dd.is_alive() and not gg.is_alive()
    if dd.error is not None:
        raise dd.error
    return dd, seen


def test_identity_calibration_is_the_uncalibrated_run_bit_for_bit_emulated(monkeypatch, tmp_path):
    """four MAD frames, camera 64x96 -> rescale 40x72 -> crop 32x64: losses, trained blocks, the frames the network saw and every weight equal the run without
    a calibration; the calibration goes in once as a dict and once as the JSON file the CLI takes"""
    from conftest import _emul_backend
    backend = _emul_backend()
    cam, image_shape, crop_shape = (64, 96), [40, 72], [32, 64]
    runs = []
    cal_file = tmp_path / "identity.json"
    cal_file.write_text(json.dumps(exact_calibration(*cam)))
    for calibration in (None, str(cal_file)):
        np.random.seed(11)                                  # the sampler draws from numpy's global generator: both runs train the same blocks
        dd, seen = _run_loop(backend.lib, "cpu", "MAD", 4, monkeypatch, cam, image_shape, crop_shape, calibration=calibration)
        assert len(seen) == 4 and (dd._rectifier is None) == (calibration is None)
        runs.append((dd, seen))
    (da, sa), (db, sb) = runs
    assert [h for h in da.history] == [h for h in db.history]                                   # loss (a float: equal bits), blocks, reset per frame
    for a, b in zip(sa, sb):
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])    # left, right, disparity
    assert torch.equal(da._net.engine.params.w, db._net.engine.params.w) and not torch.equal(da._net.engine.params.w, da._net.engine.params.w0)


def test_shift_calibration_feeds_the_shifted_frames_emulated(monkeypatch):
    """rectified principal point 3 pixels to the left of the raw one: rectified pixel u shows raw pixel u + 3; no rescale, no crop: the network sees exactly that"""
    from conftest import _emul_backend
    from madnet_hip import synthetic as S
    backend = _emul_backend()
    H, W = 48, 64
    dd, seen = _run_loop(backend.lib, "cpu", "NONE", 2, monkeypatch, (H, W), [-1], [H, W], calibration=exact_calibration(H, W, shift=3))
    assert len(seen) == 2
    for k, (_, _, left, right, _) in enumerate(seen):
        l, r, _ = S.make_pair(H, W, stream_id=k)
        for got, raw in ((left, l), (right, r)):
            raw = torch.from_numpy(raw.astype(np.uint8).astype(np.float32))
            assert tuple(got.shape) == (1, H, W, 3)
            assert torch.equal(got[:, :, :W - 3], raw[:, :, 3:]) and not got[:, :, W - 3:].any()
    with pytest.raises(ValueError, match="calibration is for"):     # a camera of another size than the calibration states
        dd._prepare(np.zeros((2, H + 2, W, 3), np.uint8))


@pytest.mark.gpu
def test_live_demo_cli_with_calibration_gpu(tmp_path):
    """The CLI on the MI355X: 8 synthetic 480x640 frames in MAD mode through --calibration (the exact identity): a finite loss on every frame, the PNGs written."""
    cal = tmp_path / "cal.json"
    cal.write_text(json.dumps(exact_calibration(480, 640)))
    out = tmp_path / "disp"
    r = subprocess.run([sys.executable, os.path.join(DEMO, "Live_Adaptation_Demo.py"), "--weights", "calibrated:1", "--mode", "MAD", "--frames", "8", "--framerate", "0",
                        "--calibration", str(cal), "--output", str(out), "--logDispStep", "4", "--SSIMTh", "10"], capture_output=True, text=True, timeout=600, cwd=DEMO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    steps = [l for l in r.stdout.splitlines() if l.startswith("Step ")]
    assert len(steps) == 8 and all(np.isfinite(float(l.split(":")[1])) for l in steps)
    assert sorted(os.listdir(str(out))) == ["disparity_0.png", "disparity_4.png"]
    assert "detector stopped" in r.stdout and "Camera grabber stopped" in r.stdout
