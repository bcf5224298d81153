"""The continual loop with proxy labels from the on-device matcher (Stereo_Continual_Adaptation.py --proxies sgm; madnet_hip/proxy.py over mh_sgm_proxy).
List writing, frame size and weights are those of tests/test_continual_cli_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "real-time-self-adaptive-deep-stereo_amd")
H, W = 64, 128


def _make_list(tmp_path, frames, proxy_column):
    """synthetic frames, rows left;right;gt[;proxy] -- the proxy column as tests/test_continual_cli_gpu.py writes it: ground truth with holes"""
    from PIL import Image
    from madnet_hip import synthetic as S
    rows = []
    for t in range(frames):
        l, r, gt = S.make_pair(H, W, frame=t)
        names = [str(tmp_path / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d", "p")]
        Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
        Image.fromarray((gt[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
        if proxy_column:
            px = gt[0, :, :, 0].copy(); px[::3] = 0
            Image.fromarray((px * 256).astype(np.uint16)).save(names[3])
        rows.append(";".join(names if proxy_column else names[:3]))
    lst = tmp_path / "list.csv"
    lst.write_text("# left;right;gt%s\n" % (";proxy" if proxy_column else "") + "\n".join(rows) + "\n")
    return str(lst)


def _run(tmp_path, lst, name, extra):
    import Stereo_Continual_Adaptation as SCA
    out = tmp_path / name
    os.makedirs(out / "disparities"); os.makedirs(out / "weights")
    argv = ["-l", lst, "-o", str(out), "--weights", "calibrated:1", "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"),
            "--imageShape", str(H), str(W), "--SSIMTh", "1000", "--sampleMode", "SEQUENTIAL", "--dumpOutputs"] + extra
    args = SCA.build_parser().parse_args(argv)
    np.random.seed(0)
    SCA.main(args)
    return SCA, args, out


def test_matcher_tensor_through_the_prefetcher_equals_host_array(hip):
    """two Adapter(loss='proxy', mode='FULL') from the same weights: one takes the matcher's device tensor straight from the prefetcher (the step's input table
    names it, no copy; ordered by the slot's event alone), the other the same map as a host array.  Loss and disparity are identical after 3 steps."""
    import Nets
    from Data_utils import data_reader
    from madnet_hip import engine as E, synthetic as S
    from madnet_hip.adapter import Adapter
    from madnet_hip.proxy import ProxyMatcher
    wn = S.calibrated_weights(dict(E.madnet_manifest()), 1)
    pairs = [S.make_pair(H, W, frame=t) for t in range(3)]
    z = torch.zeros(1, H, W, 3, device="cuda")

    def make():
        net = Nets.get_stereo_net("MADNet", {"left_img": z, "right_img": z, "split_layers": [None], "sequence": True, "train_portion": "BEGIN", "bulkhead": False,
                                             "weights": wn})
        return net, Adapter(net, mode="FULL", lr=1e-3, loss="proxy", ssim_th=1e9)

    net_a, a = make()
    m = ProxyMatcher(a.lib, 1, H, W, max_disp=64, device="cuda")
    maps, res_a = [], []
    pf = data_reader.device_prefetcher([(l, r, g) for l, r, g in pairs], "cuda", depth=2, consumer_stream=a.stream, lib=a.lib, proxy_matcher=m)
    for left, right, gt, proxy in pf:
        assert proxy.data_ptr() % 16 == 0 and proxy.is_contiguous()
        out = a.step(left, right, gt[..., 0], proxy=proxy)
        assert a._tab is None or a._tab.tab.src[3] == proxy.data_ptr(), "the matcher's tensor did not go through the step's input table"
        res_a.append((out["loss"], out["disparity"].clone()))
        with torch.cuda.stream(a.stream):
            maps.append(proxy.clone())
    pf.close()
    torch.cuda.synchronize()
    assert all(int((p > 0).sum()) > 0 for p in maps)
    net_b, b = make()
    for t, (l, r, g) in enumerate(pairs):
        out = b.step(l, r, g[..., 0], proxy=maps[t].cpu().numpy())
        assert np.isfinite(out["loss"]) and out["loss"] == res_a[t][0], (t, out["loss"], res_a[t][0])
        assert torch.equal(out["disparity"], res_a[t][1])
    torch.cuda.synchronize()
    assert torch.equal(net_a.engine.params.w, net_b.engine.params.w)


def test_continual_script_with_sgm_proxies(hip, tmp_path):
    """--proxies sgm on a three-column list of 4 frames: exits clean, the report holds finite numbers and every step's loss is finite (a finite proxy loss
    means the matcher left valid pixels: all-invalid labels give NaN)"""
    from madnet_hip.adapter import Adapter
    lst = _make_list(tmp_path, 4, proxy_column=False)
    losses, real = [], Adapter.step

    def step(self, *a, **k):
        out = real(self, *a, **k)
        losses.append(out["loss"])
        return out
    Adapter.step = step
    try:
        SCA, args, out = _run(tmp_path, lst, "out_sgm", ["--mode", "FULL", "--modelName", "MADNet", "--proxies", "sgm"])
    finally:
        Adapter.step = real
    assert args.proxies == "sgm" and args.proxyMaxDisp == 128 and SCA.build_parser().parse_args(["-l", "x", "-o", "y", "--weights", "z", "--blockConfig", "c"]).proxies == "list"
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    overall = open(out / "overall.csv").read().split("\n")
    assert overall[0] == "EPE\tD1" and all(np.isfinite(float(v)) for v in overall[1].split("\t"))
    series = open(out / "series.csv").read().strip().split("\n")
    assert len(series) == 5 and all(np.isfinite(float(v)) for row in series[1:] for v in row.split(" & "))


def test_continual_script_list_proxies_unchanged(hip, tmp_path):
    """the default --proxies list on a four-column list writes the series.csv it wrote before the matcher existed: tests/golden/continual_sgm/series_list.csv was
    written by the parent commit's script (same list, same arguments: Dispnet, FULL) on an MI355X"""
    lst = _make_list(tmp_path, 3, proxy_column=True)
    SCA, args, out = _run(tmp_path, lst, "out_list", ["--mode", "FULL"])
    assert args.proxies == "list" and args.modelName == "Dispnet"
    want = open(os.path.join(HERE, "golden", "continual_sgm", "series_list.csv")).read()
    assert open(out / "series.csv").read() == want
