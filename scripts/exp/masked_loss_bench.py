"""Cost of the masked reprojection loss on one GPU, B = 1, at 375 x 1242 (KITTI) and 320 x 512 (the live demo's crop).
usage: python scripts/exp/masked_loss_bench.py [--replays N] [--warm N] [--rounds N] [--precision P]
(i)  the op alone: a one-record plan (LOSS, phase 0, value + gradient) captured into a graph; HIP events around N back-to-back replays, microseconds per replay.
     Forms: unmasked (mh_reprojection_loss_phase -- its tile kernel is the parent commit's, instruction for instruction), masked with all-ones masks, masked with
     a rectification-like mask (border wedges + pad).  They alternate in rounds in the same process, every form warmed first.
(ii) Adapter.step of MADNet FULL through the captured graph (the engine path of bench.py), without masks and with them: HIP events around one step.
Bytes per call, from the shapes (n = B H W): the count pass reads disp (4 n) and three mask bytes per pixel (its own and the two taps': <= 3 n, mostly cache hits),
the tile kernel reads disp (4 n), both frames (12 n + the two taps' 24 n through the caches) and, masked, the same mask bytes again, and writes ddisp (4 n)."""
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
from madnet_hip import plan as PL
from madnet_hip.adapter import Adapter

argv = sys.argv[1:]
opt = lambda name, default, typ: typ(argv[argv.index(name) + 1]) if name in argv else default
replays, warm, rounds = opt("--replays", 2000, int), opt("--warm", 200, int), opt("--rounds", 3, int)
precision = opt("--precision", "mixed", str)
lib = _ffi.lib()
stream = torch.cuda.Stream()


def wedge_masks(H, W):
    """what rectification + crop_or_pad leave: a pad band, and wedges a few percent of the width that grow towards two corners"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    vl = ((xx >= 0.03 * W * yy / H + 4) & (xx < W - 4) & (yy >= 6) & (yy < H - 6 - 0.02 * H * xx / W)).to(torch.uint8)[None]
    vr = ((xx >= 4) & (xx < W - 4 - 0.03 * W * (1 - yy / H)) & (yy >= 6 + 0.02 * H * xx / W) & (yy < H - 6)).to(torch.uint8)[None]
    return vl.cuda().contiguous(), vr.cuda().contiguous()


def op_forms(H, W):
    B = 1
    l, r, _ = S.make_pair(H, W)
    left, right = (torch.from_numpy(a).cuda() for a in (l, r))
    g = torch.Generator().manual_seed(1)
    disp = (torch.rand(B, H, W, generator=g) * 160.0).cuda()
    forms = []
    for name, masks in (("unmasked", None), ("masked, all-ones masks", (torch.ones(B, H, W, dtype=torch.uint8, device="cuda"),) * 2), ("masked, wedge masks", wedge_masks(H, W))):
        ws = torch.zeros(lib.loss_ws_floats(B, H, W), device="cuda")
        res, dd = torch.zeros(4, device="cuda"), torch.zeros(B, H, W, device="cuda")
        rec = PL.Recorder()
        if masks is not None:
            ops.loss_set_valid(lib, ws, *masks)
        ops.reprojection_loss(rec, left, right, disp, ws, res, dd, valid=masks)
        plan = rec.compile()
        with torch.cuda.stream(stream):
            plan.capture(lib, stream.cuda_stream)
        forms.append(("%dx%d %s" % (H, W, name), plan, (left, right, disp, ws, res, dd, masks)))
    return forms


def per_replay_us(plan, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(count):
            plan.launch(lib, stream.cuda_stream)
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


print("(i) the op alone: HIP events around %d back-to-back graph replays of a one-record plan, after %d warm-up replays, %d rounds; us per replay" % (replays, warm, rounds))
for H, W in ((375, 1242), (320, 512)):
    forms = op_forms(H, W)
    for _, plan, _ in forms:
        per_replay_us(plan, warm)
    for rnd in range(rounds):
        print("  round %d  " % rnd + "   ".join("%s %7.2f" % (name, per_replay_us(plan, replays)) for name, plan, _ in forms))
        sys.stdout.flush()

B, H, W = 1, 375, 1242
l, r, gt = S.make_pair(H, W)
left, right, gtd = (torch.from_numpy(a).cuda() for a in (l, r, gt[..., 0]))
wn = S.calibrated_weights(dict(E.madnet_manifest()), 1)


def adapter(masks):
    net = Nets.get_stereo_net("MADNet", {"left_img": left, "right_img": right, "split_layers": [None], "sequence": True, "train_portion": "BEGIN",
                                         "bulkhead": False, "weights": wn, "precision": precision})
    ad = Adapter(net, mode="FULL", lr=1e-4, ssim_th=1e9, valid_masks=masks)
    ad._plan("FULL")
    return ad


def step_us(ad, count):
    ev = []
    for _ in range(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); ad.step(left, right, gtd); e1.record(); e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e3)
    return np.asarray(ev)


steps = [("FULL step, no masks", adapter(None)), ("FULL step, wedge masks", adapter(wedge_masks(H, W)))]
print("(ii) Adapter.step, MADNet %s FULL at %d x %d, captured graph: HIP events around one step, 200 steps after 30 warm-up steps, %d rounds; us" % (precision, H, W, rounds))
for _, ad in steps:
    step_us(ad, 30)
for rnd in range(rounds):
    for name, ad in steps:
        ev = step_us(ad, 200)
        print("  round %d  %-26s median %8.1f  min %8.1f  p90 %8.1f" % (rnd, name, np.median(ev), ev.min(), np.percentile(ev, 90)))
        sys.stdout.flush()
