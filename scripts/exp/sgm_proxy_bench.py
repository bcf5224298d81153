"""The on-device proxy matcher (mh_sgm_proxy) on KITTI size, and the continual loop with and without it.
usage: python scripts/exp/sgm_proxy_bench.py MODE [--paths {4,8}] [--median] [--speckle N] [--scale {1,2}]      (the matcher's options, for total / kernels / loop / speckle / scale)
  total    1 x 375 x 1242, D = 128: workspace bytes, wall time of one call (events around 100 calls, after 20), uint8 and float32 frames
  kernels  the same calls and nothing else -- run it under `rocprofv3 --kernel-trace --stats` for the time per kernel
  speckle  the same call without and with the speckle filter (--speckle N, default 100, range 1.0), alternating in blocks of 100 calls, three rounds after a
           warm-up of both, one process: the filter's cost is the difference of the medians; and the filter alone on the matcher's labels
  scale    the same call at scale 1 and at scale 2 (half-size frames, mh_sgm_proxy_scaled), alternating in blocks of 100 calls, three rounds after a warm-up of
           both, one process: workspace bytes, medians, their ratio
  parent PATH   the call at scale 1 through this tree's library and through another build of the library at PATH (the parent commit's; it needs no symbol this
           tree added), both loaded into one process, alternating in blocks of 100 calls, three rounds: same bits, medians and spread of both
  loop     Adapter.step (MADNet, MAD and FULL, 320 x 1216 resident frames, 200 steps after 20): alone / with the matcher of the NEXT frame on a second stream
           in front of an event the step waits for (the prefetcher's position)
  script   Stereo_Continual_Adaptation.py --proxies list against --proxies sgm on the same 220-row list (8 distinct 375 x 1242 frames as PNGs, cropped to
           320 x 1216 by the script): frames / s over the last 200 Adapter.step calls"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)
import numpy as np
import torch
from madnet_hip import _ffi, engine as E, synthetic as S
from madnet_hip.proxy import ProxyMatcher

argv = sys.argv[1:]
median = "--median" in argv
if median:
    argv.remove("--median")
paths = 4
if "--paths" in argv:
    paths = int(argv[argv.index("--paths") + 1])
    del argv[argv.index("--paths"):argv.index("--paths") + 2]
speckle = 0
if "--speckle" in argv:
    speckle = int(argv[argv.index("--speckle") + 1])
    del argv[argv.index("--speckle"):argv.index("--speckle") + 2]
scale = 1
if "--scale" in argv:
    scale = int(argv[argv.index("--scale") + 1])
    del argv[argv.index("--scale"):argv.index("--scale") + 2]
mode = argv[0] if argv else "total"
if mode == "speckle" and not speckle:
    speckle = 100
lib = _ffi.lib()


def matcher_calls(n, warm, dtype):
    H, W, D = 375, 1242, 128
    l, r, _ = S.make_pair(H, W)
    tl, tr = (torch.from_numpy(a.astype(dtype)).cuda() for a in (l, r))
    m = ProxyMatcher(lib, 1, H, W, max_disp=D, paths=paths, median=median, speckle_size=speckle, scale=scale)
    out = m.new_output()
    for _ in range(warm):
        m.compute(tl, tr, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); m.compute(tl, tr, out=out); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return m, out, np.asarray(ts)


if mode in ("total", "kernels"):
    for dtype in (np.uint8, np.float32):
        m, out, ts = matcher_calls(100, 20, dtype)
        if mode == "total":
            print("mh_sgm_proxy 1x375x1242 D=128 paths %d median %d scale %d %-7s workspace %.1f MB   one call: median %.3f ms, min %.3f, max %.3f   valid share %.3f"
                  % (paths, median, scale, np.dtype(dtype).name, m.ws.numel() / 1e6, np.median(ts), ts.min(), ts.max(), float((out > 0).float().mean())))


def timed(fn, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.asarray(ts)


if mode == "speckle":
    from madnet_hip import ops
    H, W, D = 375, 1242, 128
    l, r, _ = S.make_pair(H, W)
    tl, tr = (torch.from_numpy(a.astype(np.uint8)).cuda() for a in (l, r))
    plain = ProxyMatcher(lib, 1, H, W, max_disp=D, paths=paths, median=median)
    filt = ProxyMatcher(lib, 1, H, W, max_disp=D, paths=paths, median=median, speckle_size=speckle)
    o0, o1, o2 = plain.new_output(), filt.new_output(), filt.new_output()
    runs = {"matcher alone": lambda: plain.compute(tl, tr, out=o0), "matcher + speckle": lambda: filt.compute(tl, tr, out=o1),
            "speckle alone": lambda: ops.sgm_speckle(lib, o0, o2, filt.speckle_ws, speckle, 1.0)}
    for fn in runs.values():
        timed(fn, 20)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2), "the filter behind the matcher and the filter on the matcher's labels differ"
    print("1x375x1242 D=128 paths %d median %d uint8, speckle filter (%d, 1.0): filter workspace %.1f MB, valid share %.4f -> %.4f"
          % (paths, median, speckle, filt.speckle_ws.numel() / 1e6, float((o0 > 0).float().mean()), float((o1 > 0).float().mean())))
    for rnd in range(3):
        med = {}
        for name, fn in runs.items():
            ts = timed(fn, 100)
            med[name] = np.median(ts)
            print("round %d  %-18s one call: median %.3f ms, min %.3f, max %.3f" % (rnd, name, np.median(ts), ts.min(), ts.max()))
        print("round %d  the filter adds %.3f ms = %.1f %% of the matcher" % (rnd, med["matcher + speckle"] - med["matcher alone"],
              100.0 * (med["matcher + speckle"] - med["matcher alone"]) / med["matcher alone"])); sys.stdout.flush()

if mode == "scale":
    H, W, D = 375, 1242, 128
    l, r, _ = S.make_pair(H, W)
    tl, tr = (torch.from_numpy(a.astype(np.uint8)).cuda() for a in (l, r))
    ms = {sc: ProxyMatcher(lib, 1, H, W, max_disp=D, paths=paths, median=median, scale=sc) for sc in (1, 2)}
    outs = {sc: m.new_output() for sc, m in ms.items()}
    runs = {sc: (lambda sc=sc: ms[sc].compute(tl, tr, out=outs[sc])) for sc in (1, 2)}
    for fn in runs.values():
        timed(fn, 20)
    torch.cuda.synchronize()
    for sc in (1, 2):
        print("1x375x1242 D=128 paths %d median %d uint8 scale %d: workspace %.1f MB, valid share %.4f"
              % (paths, median, sc, ms[sc].ws.numel() / 1e6, float((outs[sc] > 0).float().mean())))
    for rnd in range(3):
        med = {}
        for sc, fn in runs.items():
            ts = timed(fn, 100)
            med[sc] = np.median(ts)
            print("round %d  scale %d  one call: median %.3f ms, min %.3f, max %.3f" % (rnd, sc, np.median(ts), ts.min(), ts.max()))
        print("round %d  scale 1 / scale 2 = %.2f" % (rnd, med[1] / med[2])); sys.stdout.flush()

if mode == "parent":
    import ctypes as C
    H, W, D = 375, 1242, 128
    l, r, _ = S.make_pair(H, W)
    tl, tr = (torch.from_numpy(a.astype(np.uint8)).cuda() for a in (l, r))
    old = C.CDLL(argv[1])
    old.mh_sgm_proxy_ex.restype = C.c_int
    old.mh_sgm_proxy_ex.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p]
    m = ProxyMatcher(lib, 1, H, W, max_disp=D, paths=paths, median=median)
    o_new, o_old = m.new_output(), m.new_output()
    ws_old = torch.empty_like(m.ws)

    def call_old():
        rc = old.mh_sgm_proxy_ex(tl.data_ptr(), tr.data_ptr(), 1, ws_old.data_ptr(), o_old.data_ptr(), 1, H, W, D, 10, 120, 95, 1, paths, int(median), None)
        assert rc == 0, rc
    runs = {"parent": call_old, "this tree": lambda: m.compute(tl, tr, out=o_new)}
    for fn in runs.values():
        timed(fn, 20)
    torch.cuda.synchronize()
    print("1x375x1242 D=128 paths %d median %d uint8, scale 1 through mh_sgm_proxy_scaled against mh_sgm_proxy_ex of %s: same bits: %s, valid share %.4f"
          % (paths, median, argv[1], "yes" if torch.equal(o_new.view(torch.int32), o_old.view(torch.int32)) else "NO", float((o_new > 0).float().mean())))
    for rnd in range(3):
        for name, fn in runs.items():
            ts = timed(fn, 100)
            print("round %d  %-10s one call: median %.3f ms, min %.3f, max %.3f" % (rnd, name, np.median(ts), ts.min(), ts.max()))
        sys.stdout.flush()

if mode == "loop":
    import Nets
    from madnet_hip.adapter import Adapter
    H, W = 320, 1216
    wn = S.calibrated_weights(dict(E.madnet_manifest()), 1)
    pairs = [S.make_pair(H, W, stream_id=100, frame=t) for t in range(8)]
    z = torch.zeros(1, H, W, 3, device="cuda")
    frames = [tuple(torch.as_tensor(a, dtype=torch.float32, device="cuda") for a in (l, r, np.ascontiguousarray(g[..., 0]))) for l, r, g in pairs]
    m = ProxyMatcher(lib, 1, H, W, max_disp=128, paths=paths, median=median, scale=scale)
    side = torch.cuda.Stream()
    for amode in ("MAD", "FULL"):
        net = Nets.get_stereo_net("MADNet", {"left_img": z, "right_img": z, "split_layers": [None], "sequence": True, "train_portion": "BEGIN",
                                             "bulkhead": amode == "MAD", "weights": wn})
        import json
        ad = Adapter(net, mode=amode, block_config=json.load(open(os.path.join(PKG, "block_config", "MadNet_full.json"))), lr=1e-4, loss="proxy", ssim_th=1e9,
                     sample_mode="PROBABILITY", kitti_metrics=True)
        proxies = [m.compute(f[0], f[1]) for f in frames]
        outs = [m.new_output() for _ in range(3)]
        evs = [torch.cuda.Event() for _ in range(3)]
        torch.cuda.synchronize()
        for with_matcher in (False, True, False, True):
            np.random.seed(0)
            N, warm = 220, 20
            if with_matcher:
                with torch.cuda.stream(side):
                    m.compute(frames[0][0], frames[0][1], out=outs[0], stream=side.cuda_stream); evs[0].record(side)
            for k in range(N):
                if k == warm:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                f = frames[k % 8]
                if with_matcher:
                    nf = frames[(k + 1) % 8]
                    with torch.cuda.stream(side):              # the NEXT frame's labels, as the prefetcher computes them: they overlap this step
                        m.compute(nf[0], nf[1], out=outs[(k + 1) % 3], stream=side.cuda_stream); evs[(k + 1) % 3].record(side)
                    ad.stream.wait_event(evs[k % 3])
                    ad.step(f[0], f[1], f[2], proxy=outs[k % 3])
                else:
                    ad.step(f[0], f[1], f[2], proxy=proxies[k % 8])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / (N - warm)
            print("Adapter.step MADNet %-4s 320x1216 resident frames, %-44s %8.3f ms / step  (%.1f steps / s)"
                  % (amode, "matcher (scale %d) of the next frame alongside" % scale if with_matcher else "labels resident", dt * 1e3, 1.0 / dt)); sys.stdout.flush()

if mode == "script":
    import pathlib, tempfile
    from PIL import Image
    import Stereo_Continual_Adaptation as SCA
    from madnet_hip.adapter import Adapter
    H, W = 375, 1242
    tmp = pathlib.Path(tempfile.mkdtemp())
    rows = []
    for t in range(8):
        l, r, gt = S.make_pair(H, W, frame=t)
        names = [str(tmp / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d", "p")]
        Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
        Image.fromarray((gt[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
        px = gt[0, :, :, 0].copy(); px[::3] = 0
        Image.fromarray((px * 256).astype(np.uint16)).save(names[3])
        rows.append(";".join(names))
    lst = tmp / "list.csv"
    lst.write_text("\n".join(rows[i % 8] for i in range(220)) + "\n")
    stamps, real = [], Adapter.step

    def step(self, *a, **k):
        out = real(self, *a, **k)
        stamps.append(time.perf_counter())
        return out
    Adapter.step = step
    for rnd in range(2):
        for src in ("list", "sgm"):
            out = tmp / ("out_%s_%d" % (src, rnd))
            os.makedirs(out / "weights")
            del stamps[:]
            np.random.seed(0)
            SCA.main(SCA.build_parser().parse_args(["-l", str(lst), "-o", str(out), "--weights", "calibrated:1", "--modelName", "MADNet", "--mode", "MAD",
                                                    "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"), "--SSIMTh", "1000",
                                                    "--sampleMode", "PROBABILITY", "--proxies", src]))
            torch.cuda.synchronize()
            print("RESULT Stereo_Continual_Adaptation.py MADNet MAD 320x1216 --proxies %-4s  %.2f frames / s over the last 200 of %d steps   overall.csv %s"
                  % (src, 200.0 / (stamps[-1] - stamps[-201]), len(stamps), open(out / "overall.csv").read().split("\n")[1].replace("\t", " ")))
            sys.stdout.flush()
