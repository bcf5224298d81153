"""The continual loop with proxy labels from the on-device matcher at half resolution (Stereo_Continual_Adaptation.py --proxies sgm --proxyScale 2;
madnet_hip/proxy.py over mh_sgm_proxy_scaled).  List writing, frame size and weights are those of tests/test_continual_sgm8_gpu.py."""
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
def test_continual_script_at_half_resolution(hip, tmp_path):
    """a three-column list of 4 frames: exits clean, every step's loss is finite (all-invalid labels give NaN; the oracle gives 5176 .. 5292 valid labels per
    frame), the report holds finite numbers, and the matcher was built with scale 2 and a workspace of mh_sgm_ws_bytes_scaled bytes"""
    import Stereo_Continual_Adaptation as SCA
    from madnet_hip import proxy
    from madnet_hip.adapter import Adapter
    lst = _make_list(tmp_path, 4)
    out = tmp_path / "out_sgm_half"
    os.makedirs(out / "disparities"); os.makedirs(out / "weights")
    argv = ["-l", lst, "-o", str(out), "--weights", "calibrated:1", "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"),
            "--imageShape", str(H), str(W), "--SSIMTh", "1000", "--sampleMode", "SEQUENTIAL", "--dumpOutputs", "--mode", "FULL", "--modelName", "MADNet",
            "--proxies", "sgm", "--proxyScale", "2", "--proxyMaxDisp", "128"]
    args = SCA.build_parser().parse_args(argv)
    assert args.proxyScale == 2 and args.proxyMaxDisp == 128 and args.proxyPaths == 4 and args.proxyMedian is False and args.proxySpeckle == 0
    losses, built, real_step, real_init = [], [], Adapter.step, proxy.ProxyMatcher.__init__

    def step(self, *a, **k):
        res = real_step(self, *a, **k)
        losses.append(res["loss"])
        return res

    def init(self, *a, **k):
        real_init(self, *a, **k)
        built.append((self.scale, self.max_disp, self.params["paths"], self.params["median"], self.ws.numel()))
    Adapter.step, proxy.ProxyMatcher.__init__ = step, init
    try:
        np.random.seed(0)
        SCA.main(args)
    finally:
        Adapter.step, proxy.ProxyMatcher.__init__ = real_step, real_init
    lib = hip.lib
    assert built == [(2, 128, 4, False, lib.sgm_ws_bytes_scaled(1, H, W, 128, 4, 0, 2))], built
    assert 0 < built[0][4] < lib.sgm_ws_bytes(1, H, W, 128)
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    overall = open(out / "overall.csv").read().split("\n")
    assert overall[0] == "EPE\tD1" and all(np.isfinite(float(v)) for v in overall[1].split("\t"))
    series = open(out / "series.csv").read().strip().split("\n")
    assert len(series) == 5 and all(np.isfinite(float(v)) for row in series[1:] for v in row.split(" & "))


def test_parser_default_scale_is_1_and_scale_2_checks_the_range(capsys):
    import Stereo_Continual_Adaptation as SCA
    base = ["-l", "x", "-o", "y", "--weights", "z", "--blockConfig", "c"]
    d = SCA.build_parser().parse_args(base)
    assert d.proxies == "list" and d.proxyScale == 1 and d.proxyMaxDisp == 128 and d.proxyPaths == 4 and d.proxyMedian is False and d.proxySpeckle == 0
    for ok in (128, 256, 384):
        a = SCA.build_parser().parse_args(base + ["--proxies", "sgm", "--proxyScale", "2", "--proxyMaxDisp", str(ok)])
        assert a.proxyScale == 2 and a.proxyMaxDisp == ok
    assert SCA.build_parser().parse_args(base + ["--proxies", "sgm", "--proxyMaxDisp", "64"]).proxyMaxDisp == 64      # scale 1: as before
    for bad in (64, 192, 100):
        with pytest.raises(SystemExit):
            SCA.build_parser().parse_args(base + ["--proxies", "sgm", "--proxyScale", "2", "--proxyMaxDisp", str(bad)])
        err = capsys.readouterr().err
        assert "128, 256 and 384" in err, err
    with pytest.raises(SystemExit):
        SCA.build_parser().parse_args(base + ["--proxyScale", "3"])
    args = SCA.build_parser().parse_args(base + ["--proxies", "sgm", "--proxyScale", "2"])
    args.proxyMaxDisp = 64                                   # a caller's own namespace: main refuses it before any device work
    with pytest.raises(ValueError, match="128, 256 and 384"):
        SCA.main(args)
