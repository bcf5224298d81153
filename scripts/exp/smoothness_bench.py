"""Cost of the edge-aware smoothness term on one GPU, at the KITTI frame size 1 x 375 x 1242.
usage: python scripts/exp/smoothness_bench.py [--calls N] [--warm N] [--rounds N] [--weight W] [--precision P]
HIP events around ONE call, microseconds; every form is warmed first, then the forms alternate in rounds in the same process:
  (i)  mh_smoothness_loss alone (two launches: tile kernel, final reduction), with and without the gradient, and the reprojection loss beside it for scale;
  (ii) Adapter.step of MADNet, FULL and MAD (block_config/MadNet_piramid_only.json, PROBABILITY sampler) with smoothness weight 0 and weight W: the whole
       step as its caller sees it (upload of device frames through the input table, ONE graph replay, read-back, host bookkeeping).
Bytes the op moves per call, from the shapes: reads disp (4 n) + the frame (12 n), writes partial sums (4 per tile) and, with the gradient, reads and writes ddisp
when it accumulates (8 n) or writes it (4 n), n = B H W pixels; halo re-reads are served by the caches."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)
import numpy as np
import torch
import Nets
from madnet_hip import _ffi, ops, engine as E, synthetic as S
from madnet_hip.adapter import Adapter

argv = sys.argv[1:]
opt = lambda name, default, typ: typ(argv[argv.index(name) + 1]) if name in argv else default
calls, warm, rounds = opt("--calls", 200, int), opt("--warm", 30, int), opt("--rounds", 3, int)
weight, precision = opt("--weight", 0.1, float), opt("--precision", "mixed", str)
lib = _ffi.lib()
B, H, W = 1, 375, 1242
n = B * H * W
l, r, gt = S.make_pair(H, W)
left, right, gtd = (torch.from_numpy(a).cuda() for a in (l, r, gt[..., 0]))
g = torch.Generator().manual_seed(1)
disp = (torch.rand(B, H, W, generator=g) * 160.0).cuda()
ws = torch.zeros(lib.loss_ws_floats(B, H, W), device="cuda")
res = torch.zeros(4, device="cuda")
dd = torch.zeros(B, H, W, device="cuda")


def timed(fn, count):
    ev = []
    for _ in range(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e3)
    return np.asarray(ev)


def report(title, forms):
    print(title)
    for _, fn in forms:
        timed(fn, warm)
    for rnd in range(rounds):
        for name, fn in forms:
            ev = timed(fn, calls)
            print("  round %d  %-58s median %8.1f  min %8.1f  p90 %8.1f us" % (rnd, name, np.median(ev), ev.min(), np.percentile(ev, 90)))
            sys.stdout.flush()


tiles = int(lib.smoothness_ws_floats(B, H, W))
print("bytes per call at %d x %d x %d: value only %.2f MB; with the gradient written %.2f MB, accumulated %.2f MB; %d tiles"
      % (B, H, W, (16 * n + 4 * tiles) / 1e6, (20 * n + 4 * tiles) / 1e6, (24 * n + 4 * tiles) / 1e6, tiles))
report("(i) the op alone, float32: HIP events around one call, %d calls after %d warm-up calls, %d rounds" % (calls, warm, rounds), [
    ("mh_smoothness_loss, value only (2 launches)", lambda: ops.smoothness_loss(lib, disp, left, ws, res, None, weight=weight)),
    ("mh_smoothness_loss, value + gradient written (2 launches)", lambda: ops.smoothness_loss(lib, disp, left, ws, res, dd, weight=weight)),
    ("mh_smoothness_loss, value + gradient accumulated", lambda: ops.smoothness_loss(lib, disp, left, ws, res, dd, weight=weight, accumulate=True)),
    ("mh_reprojection_loss, value + gradient (2 launches)", lambda: ops.reprojection_loss(lib, left, right, disp, ws, res, dd)),
    ("mh_reprojection_loss + smoothness (4 launches)", lambda: ops.reprojection_loss(lib, left, right, disp, ws, res, dd, smoothness=weight)),
])

wn = S.calibrated_weights(dict(E.madnet_manifest()), 1)
cfg = json.load(open(os.path.join(PKG, "block_config", "MadNet_piramid_only.json")))


def adapter(mode, w):
    net = Nets.get_stereo_net("MADNet", {"left_img": left, "right_img": right, "split_layers": [None], "sequence": True, "train_portion": "BEGIN",
                                         "bulkhead": mode == "MAD", "weights": wn, "precision": precision})
    np.random.seed(0)
    ad = Adapter(net, mode=mode, block_config=cfg if mode == "MAD" else None, lr=1e-4, sample_mode="PROBABILITY", num_blocks=1, ssim_th=1e9, smoothness=w)
    for key in ([(i,) for i in range(len(cfg))] if mode == "MAD" else ["FULL"]):
        ad._plan(key)
    return ad


steps = []
for mode in ("FULL", "MAD"):
    for w in (0.0, weight):
        ad = adapter(mode, w)
        steps.append(("Adapter.step %s, smoothness %g" % (mode, w), lambda ad=ad: ad.step(left, right, gtd)))
report("(ii) Adapter.step, MADNet %s, captured graph: HIP events around one step, %d calls after %d warm-up calls, %d rounds" % (precision, calls, warm, rounds), steps)
