"""What the speckle filter does to the matcher's labels, on the CPU with the oracles of tests/ (sgm_oracle.py, sgm_speckle_oracle.py): valid share / share of valid
labels more than 3 px off the ground truth (where it is > 0) / mean error in px, unfiltered and behind the filter, on madnet_hip.synthetic.make_pair frames.
usage: python scripts/exp/sgm_speckle_quality.py [HxW ...]      (default: 40x256 96x320 188x621 375x1242; four paths, D = 128, p1 10, p2 120, uniq 95, lr_tol 1)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import sgm_oracle
import sgm_speckle_oracle
from madnet_hip import synthetic as S


def quality(o, gt):
    valid = o > 0
    both = valid & (gt > 0)
    err = np.abs(o - gt)[both]
    return "%.3f / %.3f / %.2f" % (valid.mean(), (err > 3).mean(), err.mean())


sizes = [tuple(map(int, a.split("x"))) for a in sys.argv[1:]] or [(40, 256), (96, 320), (188, 621), (375, 1242)]
for H, W in sizes:
    l, r, gt = S.make_pair(H, W)
    gt = gt[0, :, :, 0]
    o = sgm_oracle.sgm_proxy(l.astype(np.uint8), r.astype(np.uint8), 128)
    row = ["%dx%d" % (H, W), "unfiltered " + quality(o[0], gt)]
    for size, rng in ((100, 1.0), (100, 2.0)):
        row.append("(%d, %.1f) " % (size, rng) + quality(sgm_speckle_oracle.speckle(o, size, rng)[0], gt))
    print(" | ".join(row)); sys.stdout.flush()
    shares = ["%d: %.3f" % (size, (sgm_speckle_oracle.speckle(o, size, 1.0) > 0).mean()) for size in (50, 100, 200, 400)]
    print("   valid share at range 1.0 by size  " + "  ".join(shares)); sys.stdout.flush()
