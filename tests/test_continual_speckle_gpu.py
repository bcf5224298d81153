"""The continual loop with proxy labels from the on-device matcher behind its speckle filter (Stereo_Continual_Adaptation.py --proxies sgm --proxySpeckle N;
madnet_hip/proxy.py over mh_sgm_proxy_ex and mh_sgm_speckle).  List writing, frame size and weights are those of tests/test_continual_sgm8_gpu.py."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "real-time-self-adaptive-deep-stereo_amd")
H, W = 64, 128


def _make_list(tmp_path, frames):
    """synthetic frames, rows left;right;gt"""
    from PIL import Image
    from madnet_hip import synthetic as S
    rows = []
    for t in range(frames):
        l, r, gt = S.make_pair(H, W, frame=t)
        names = [str(tmp_path / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d")]
        Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
        Image.fromarray((gt[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
        rows.append(";".join(names))
    lst = tmp_path / "list.csv"
    lst.write_text("# left;right;gt\n" + "\n".join(rows) + "\n")
    return str(lst)


@pytest.mark.gpu
def test_continual_script_with_speckle_filter(hip, tmp_path):
    """a three-column list of 4 frames: exits clean, every step's loss is finite (all-invalid labels give NaN), the report holds finite numbers, and the
    matcher was built with the options the flags name: the filter's size and range, its own workspace, the matcher's workspace and parameters as without it"""
    import Stereo_Continual_Adaptation as SCA
    from madnet_hip import proxy
    from madnet_hip.adapter import Adapter
    lst = _make_list(tmp_path, 4)
    out = tmp_path / "out_speckle"
    os.makedirs(out / "disparities"); os.makedirs(out / "weights")
    argv = ["-l", lst, "-o", str(out), "--weights", "calibrated:1", "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"),
            "--imageShape", str(H), str(W), "--SSIMTh", "1000", "--sampleMode", "SEQUENTIAL", "--dumpOutputs", "--mode", "FULL", "--modelName", "MADNet",
            "--proxies", "sgm", "--proxySpeckle", "50", "--proxyMaxDisp", "64"]
    args = SCA.build_parser().parse_args(argv)
    assert args.proxySpeckle == 50 and args.proxySpeckleRange == 1.0 and args.proxyMaxDisp == 64 and args.proxyPaths == 4 and args.proxyMedian is False
    losses, built, real_step, real_init = [], [], Adapter.step, proxy.ProxyMatcher.__init__

    def step(self, *a, **k):
        res = real_step(self, *a, **k)
        losses.append(res["loss"])
        return res

    def init(self, *a, **k):
        real_init(self, *a, **k)
        built.append((self.speckle_size, self.speckle_range, self.speckle_ws.numel(), self.params["paths"], self.params["median"], self.max_disp, self.ws.numel()))
    Adapter.step, proxy.ProxyMatcher.__init__ = step, init
    try:
        np.random.seed(0)
        SCA.main(args)
    finally:
        Adapter.step, proxy.ProxyMatcher.__init__ = real_step, real_init
    lib = hip.lib
    assert built == [(50, 1.0, lib.sgm_speckle_ws_bytes(1, H, W), 4, False, 64, lib.sgm_ws_bytes(1, H, W, 64))], built
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    overall = open(out / "overall.csv").read().split("\n")
    assert overall[0] == "EPE\tD1" and all(np.isfinite(float(v)) for v in overall[1].split("\t"))
    series = open(out / "series.csv").read().strip().split("\n")
    assert len(series) == 5 and all(np.isfinite(float(v)) for row in series[1:] for v in row.split(" & "))


def test_parser_defaults_keep_the_speckle_filter_off():
    import Stereo_Continual_Adaptation as SCA
    d = SCA.build_parser().parse_args(["-l", "x", "-o", "y", "--weights", "z", "--blockConfig", "c"])
    assert d.proxies == "list" and d.proxySpeckle == 0 and d.proxySpeckleRange == 1.0
    assert d.proxyPaths == 4 and d.proxyMedian is False and d.proxyMaxDisp == 128
