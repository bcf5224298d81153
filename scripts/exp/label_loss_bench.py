"""Per-call time of the label-loss op on one GPU, at the KITTI frame size 1 x 375 x 1242.
usage: python scripts/exp/label_loss_bench.py [--calls N] [--warm N] [--rounds N]
HIP events around ONE call (result and gradient), microseconds; every form is warmed first, then the forms alternate in rounds in the same process:
  mh_proxy_loss                      the entry point every existing record uses: partial sums, final reduction, gradient (three launches)
  mh_label_loss mean_l1 / mean_l2    the same three launches (the normaliser is sum(valid))
  mh_label_loss sum_l1 / sum_huber / mean_huber     two launches: the partial-sum launch writes the gradient
and the scaled forms at scale 2 (mh_proxy_loss_scaled: three launches; mh_label_loss_scaled sum_huber: two).
The op is launch-bound at this size (1.9 MB read per pass), so the figures are dominated by the number of launches."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)
import numpy as np
import torch
from madnet_hip import _ffi, ops

argv = sys.argv[1:]
calls = int(argv[argv.index("--calls") + 1]) if "--calls" in argv else 200
warm = int(argv[argv.index("--warm") + 1]) if "--warm" in argv else 30
rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 3
lib = _ffi.lib()
B, H, W, S = 1, 375, 1242, 2
g = torch.Generator().manual_seed(1)
pred = (torch.rand(B, H, W, generator=g) * 160.0).cuda()
label = 1.0 + torch.rand(B, H, W, generator=g) * 149.0
label[torch.rand(B, H, W, generator=g) < 0.3] = 0.0
label = label.cuda()
ws = torch.zeros(max(lib.proxy_ws_floats(B, H, W), lib.proxy_scaled_ws_floats(B, H, W, S)), device="cuda")
res = torch.zeros(4, device="cuda")
dp = torch.zeros(B, H, W, device="cuda")


def timed(fn, n):
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record(); e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e3)
    return np.asarray(ev)


forms = [("mh_proxy_loss (3 launches)", lambda: ops.proxy_loss(lib, pred, label, ws, res, dp, weight=0.01))]
for name, n in (("mean_l1", 3), ("mean_l2", 3), ("sum_l1", 2), ("sum_huber", 2), ("mean_huber", 2)):
    forms.append(("mh_label_loss %s (%d launches)" % (name, n), lambda name=name: ops.label_loss(lib, pred, label, ws, res, name, 0, 192.0, dpred=dp, weight=0.01)))
forms.append(("mh_proxy_loss_scaled s=2 (3 launches)", lambda: ops.proxy_loss_scaled(lib, pred, label, ws, res, S, dp, weight=0.1)))
forms.append(("mh_label_loss_scaled s=2 sum_huber (2 launches)", lambda: ops.proxy_loss_scaled(lib, pred, label, ws, res, S, dp, weight=0.1, loss="sum_huber")))
print("label losses at %d x %d x %d, float32: HIP events around one call, %d calls after %d warm-up calls, %d rounds" % (B, H, W, calls, warm, rounds))
for _, fn in forms:
    timed(fn, warm)
for rnd in range(rounds):
    for name, fn in forms:
        ev = timed(fn, calls)
        print("  round %d  %-50s median %7.1f  min %7.1f  p90 %7.1f us" % (rnd, name, np.median(ev), ev.min(), np.percentile(ev, 90)))
        sys.stdout.flush()
