"""What matching at half resolution does to the matcher's labels, on the CPU with the oracles of tests/ (sgm8_oracle.py, sgm_scaled_oracle.py): valid share / share of
valid labels more than 3 px off the ground truth (where it is > 0) / mean error in px, at full resolution and at half resolution with the labels doubled, on
madnet_hip.synthetic.make_pair frames.  The table of DESIGN.md.
usage: python scripts/exp/sgm_scale_quality.py [HxW[:stream_id] ...]      (default: 40x256 96x320 128x416 188x621 192x640:1 375x1242; four paths, full-resolution
range 128, p1 10, p2 120, uniq 95, lr_tol 1)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import sgm8_oracle
import sgm_scaled_oracle
from madnet_hip import synthetic as S


def quality(o, gt):
    valid = o > 0
    both = valid & (gt > 0)
    err = np.abs(o - gt)[both]
    return "%.3f / %.4f / %.3f" % (valid.mean(), (err > 3).mean(), err.mean())


def parse(a):
    size, _, sid = a.partition(":")
    return tuple(map(int, size.split("x"))) + (int(sid or 0),)


cases = [parse(a) for a in sys.argv[1:]] or [(40, 256, 0), (96, 320, 0), (128, 416, 0), (188, 621, 0), (192, 640, 1), (375, 1242, 0)]
print("| frame (`stream_id`) | full resolution | half resolution, labels x 2 |")
for H, W, sid in cases:
    l, r, gt = S.make_pair(H, W, stream_id=sid)
    l, r, gt = l.astype(np.uint8), r.astype(np.uint8), gt[0, :, :, 0]
    full = sgm8_oracle.sgm_proxy(l, r, 128, paths=4)[0]
    half = sgm_scaled_oracle.sgm_proxy_scaled(l, r, 128, paths=4)[0]
    print("| %dx%d (%d) | %s | %s |" % (H, W, sid, quality(full, gt), quality(half, gt))); sys.stdout.flush()
