"""What rectification adds to the live demo's frame preparation, on one GPU.
usage: python scripts/exp/rectify_bench.py [--calls N] [--warm N]
For raw frames of 480 x 640 and 720 x 1280 (uint8, 3 channels), a calibration with lens distortion and a rotation of a few degrees per view:
  apply      Rectifier.apply on frames resident on the device: HIP events around ONE call, microseconds per pair (one mh_remap launch plus the allocation of its
             output from torch's caching allocator)
  map        the one-off cost at construction: mh_rectify_map for both views (events around the two launches)
  _prepare   RealTimeStereo._prepare on a host frame pair, without a calibration (upload, cast, rescale to 480 x 640, crop to 320 x 512: the code of the parent
             commit, unchanged by this feature) and with one (upload of the 8-bit frames, remap, rescale, crop), alternating in blocks, three rounds after a
             warm-up of both: events around one call AND a host clock around the call plus a synchronise (the upload of pageable host memory blocks the host).
             The network is not built: the figures are the preparation alone."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
for p in (ROOT, PKG, os.path.join(PKG, "Demo")):
    sys.path.insert(0, p)
import numpy as np
import torch
from madnet_hip import _ffi, ops, synthetic as S
from madnet_hip.rectify import Rectifier

argv = sys.argv[1:]
calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 200
warm = int(argv[argv.index("--warm") + 1]) if "--warm" in argv else 30
lib = _ffi.lib()


def calibration(h, w):
    """a plausible raw pair: focal length 0.8 w, barrel distortion, a few degrees between the views; the rectified view keeps the raw size"""
    def rot(ax, ay, az):
        ax, ay, az = np.deg2rad([ax, ay, az])
        rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        return (rz @ ry @ rx).tolist()
    f = 0.8 * w
    K = [[f, 0.0, w / 2.0 + 3.5], [0.0, f, h / 2.0 - 2.25], [0.0, 0.0, 1.0]]
    P = [[f, 0.0, w / 2.0, 0.0], [0.0, f, h / 2.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    return {"size": [h, w],
            "left": {"K": K, "D": [-0.28, 0.09, 0.001, -0.0007, -0.01], "R": rot(1.0, -1.5, 0.8), "P": P},
            "right": {"K": K, "D": [-0.26, 0.08, -0.0008, 0.0012, -0.008], "R": rot(-0.7, 1.2, -0.5), "P": P}}


def timed(fn, n):
    """HIP events around one call (us) and the host clock around the call plus a synchronise (us)"""
    ev, host = [], []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(); fn(); e1.record(); e1.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
        ev.append(e0.elapsed_time(e1) * 1e3)
    return np.asarray(ev), np.asarray(host)


def line(name, ev, host=None):
    s = "  %-46s events: median %8.1f  min %8.1f  p90 %8.1f us" % (name, np.median(ev), ev.min(), np.percentile(ev, 90))
    if host is not None:
        s += "   host clock: median %8.1f us" % np.median(host)
    print(s); sys.stdout.flush()


for h, w in ((480, 640), (720, 1280)):
    print("raw frames 2 x %d x %d x 3 uint8" % (h, w))
    l, r, _ = S.make_pair(h, w)
    frames = np.stack([l[0].astype(np.uint8), r[0].astype(np.uint8)])
    cal = calibration(h, w)
    rect = Rectifier(lib, cal, "cuda")
    dev_frames = torch.from_numpy(frames).cuda()
    out = rect.new_output()
    torch.cuda.synchronize()
    covered = float((rect.apply(dev_frames).sum(-1) > 0).float().mean())
    cams = [ops.camera_model(cal[s]["K"], cal[s]["D"], cal[s]["R"], cal[s]["P"]) for s in ("left", "right")]
    timed(lambda: ops.rectify_map(lib, cams, rect.map), warm)
    ev, _ = timed(lambda: ops.rectify_map(lib, cams, rect.map), calls)
    line("mh_rectify_map, both views in one launch (once)", ev)
    timed(lambda: rect.apply(dev_frames), warm)
    ev, _ = timed(lambda: rect.apply(dev_frames), calls)
    line("Rectifier.apply, resident frames (new output)", ev)
    ev, _ = timed(lambda: rect.apply(dev_frames, out=out), calls)
    line("Rectifier.apply, resident frames (given output)", ev)
    print("  share of rectified pixels with a source: %.3f; bytes per pair: %.2f MB read (frames) + %.2f MB (map) + %.2f MB written"
          % (covered, frames.nbytes / 1e6, rect.map.numel() * 4 / 1e6, out.numel() * 4 / 1e6))

    import demo_model
    import queue
    preps = {}
    for name, c in (("without calibration (the parent's path)", None), ("with calibration", cal)):
        dd = demo_model.RealTimeStereo(queue.Queue(1), image_shape=[-1], crop_shape=[-1], mode="NONE", device="cuda", calibration=c)     # no shape: no network is built
        dd._image_shape, dd._crop_shape = [480, 640], [320, 512]
        dd._ready, dd._net_shape = True, (320, 512)
        preps[name] = (lambda dd=dd: dd._prepare(frames))
    for fn in preps.values():
        timed(fn, warm)
    for rnd in range(3):
        med = {}
        for name, fn in preps.items():
            ev, host = timed(fn, calls)
            med[name] = (np.median(ev), np.median(host))
            line("round %d  _prepare %s" % (rnd, name), ev, host)
        a, b = med["without calibration (the parent's path)"], med["with calibration"]
        print("  round %d  the calibration adds %.1f us (events), %.1f us (host clock) per pair" % (rnd, b[0] - a[0], b[1] - a[1])); sys.stdout.flush()
