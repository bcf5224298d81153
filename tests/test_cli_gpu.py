"""BASELINE config 1 plumbing: the online-adaptation CLI over a list in example_list.csv format
(generated frames), modes NONE and MAD, writes stats.csv / series.csv / 16-bit disparity PNGs."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real-time-self-adaptive-deep-stereo_amd")


def _make_list(tmp_path, n, H, W):
    from PIL import Image
    from madnet_hip import synthetic as S
    rows = []
    for t in range(n):
        l, r, gt = S.make_pair(H, W, frame=t)
        names = [str(tmp_path / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d")]
        Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
        Image.fromarray((gt[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
        rows.append(",".join(names))
    p = tmp_path / "list.csv"
    p.write_text("\n".join(rows) + "\n")
    return str(p)


@pytest.mark.parametrize("mode", ["NONE", "MAD", "MAD2"])
def test_cli_end_to_end(hip, tmp_path, mode):
    """MAD2: --mode MAD --numBlocks 2 (two blocks trained per frame, Stereo_Online_Adaptation.py:181-189)"""
    two = mode == "MAD2"
    mode = "MAD" if two else mode
    import Stereo_Online_Adaptation as SOA
    lst = _make_list(tmp_path, 3, 96, 160)
    out = tmp_path / ("out_" + mode)
    os.makedirs(out / "disparities")
    argv = ["-l", lst, "-o", str(out), "--weights", "calibrated:1", "--modelName", "MADNet",
            "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"), "--mode", mode,
            "--sampleMode", "SEQUENTIAL", "--imageShape", "96", "160", "--logDispStep", "1", "--SSIMTh", "10"] + (["--numBlocks", "2"] if two else [])
    args = SOA.build_parser().parse_args(argv)
    np.random.seed(0)
    SOA.main(args)
    stats = open(out / "stats.csv").read()
    assert stats.startswith("Metrics,cumulative,average\nEPE,") and "FPS," in stats and "#resets,0" in stats
    series = open(out / "series.csv").read().strip().split("\n")
    assert series[0] == "Iteration,Time,EPE,bad3" and len(series) == 4
    assert all(np.isfinite(float(row.split(",")[2])) for row in series[1:])
    assert sorted(os.listdir(out / "disparities")) == ["disparity_%d.png" % t for t in range(3)]       # one file per frame, whatever --numBlocks
    from PIL import Image
    d = np.asarray(Image.open(out / "disparities" / "disparity_2.png"))
    assert d.dtype == np.uint16 and d.shape == (96, 160) and d.max() > 0
    if two:
        assert "fetch_counter,1,2,2,1,0" in stats          # SEQUENTIAL sampler, two blocks per frame: (0, 1), (1, 2), (2, 3)
    elif mode == "MAD":
        assert "fetch_counter,1,1,1,0,0" in stats          # SEQUENTIAL sampler over 3 frames
    else:
        # a20 (Stereo_Online_Adaptation.py:246-251, an INT path): the dumped 16-bit PNG is exactly (clip(d, 0, 256) * 256).astype(uint16) of the
        # step's disparity.  NONE mode never moves the weights, so the disparity of every frame can be recomputed: (1) by the engine itself on
        # the same frame -> the file must match BIT FOR BIT; (2) by the fp32 CPU oracle -> the engine's disparity is within ~1e-5 px of it
        # (2.6e-3 of a PNG step), so the two encodings may differ by one step where d * 256 sits on an integer, nowhere by more
        import torch
        from madnet_hip import engine as E, synthetic as S
        from oracle import madnet as OM
        wn = SOA.load_weights("calibrated:1", "MADNet")
        wt = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in wn.items()}
        for t in range(3):
            l, r, gt = S.make_pair(96, 160, frame=t)
            png = np.asarray(Image.open(out / "disparities" / ("disparity_%d.png" % t)))
            eng = E.MadNetEngine(hip.lib, 96, 160, B=1, device=hip.device, weights=wn)
            eng.set_inputs(l, r, gt[..., 0])
            eng.build_plan("NONE").run(hip.lib, 0)
            hip.sync()
            d_eng = eng.pred[0].cpu().numpy()
            assert np.array_equal(png, (np.clip(d_eng, 0, 256) * 256.0).astype(np.uint16)), "frame %d: PNG != encoding of the engine's disparity" % t
            with torch.no_grad():
                d_or = OM.forward(wt, torch.from_numpy(l), torch.from_numpy(r))[-1][0, ..., 0].numpy()
            exp = (np.clip(d_or, 0, 256) * 256.0).astype(np.uint16)
            diff = np.abs(png.astype(np.int32) - exp.astype(np.int32))
            assert diff.max() <= 1 and (diff == 0).mean() >= 0.98, (t, int(diff.max()), float((diff == 0).mean()))
            assert exp.max() > 256                          # a non-trivial map (> 1 px somewhere)


def test_continual_cli_end_to_end(hip, tmp_path):
    """Stereo_Continual_Adaptation.py plumbing: 4-column list with proxy labels, MAD + dilation 2,
    overall.csv / series.csv / histogram.csv, --saveWeights writes a TF checkpoint that reads back."""
    from PIL import Image
    from madnet_hip import synthetic as S
    import Stereo_Continual_Adaptation as SCA
    from Data_utils import tf_checkpoint
    rows = []
    for t in range(4):
        l, r, gt = S.make_pair(96, 160, frame=t)
        names = [str(tmp_path / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d", "p")]
        Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
        Image.fromarray((gt[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
        px = gt[0, :, :, 0].copy(); px[::3] = 0                       # proxy labels with holes
        Image.fromarray((px * 256).astype(np.uint16)).save(names[3])
        rows.append(";".join(names))
    lst = tmp_path / "list.csv"
    lst.write_text("# left;right;gt;proxy\n" + "\n".join(rows) + "\n")
    out = tmp_path / "out"
    os.makedirs(out / "disparities"); os.makedirs(out / "weights")
    argv = ["-l", str(lst), "-o", str(out), "--weights", "calibrated:1", "--modelName", "MADNet",
            "--blockConfig", os.path.join(PKG, "block_config", "MadNet_full.json"), "--mode", "MAD", "--sampleMode", "SEQUENTIAL",
            "--imageShape", "96", "160", "--logDispStep", "2", "--SSIMTh", "1000", "--dilation", "2", "--saveWeights",
            "--decay", "0.9", "--uf", "0.05"]
    args = SCA.build_parser().parse_args(argv)
    np.random.seed(0)
    SCA.main(args)
    overall = open(out / "overall.csv").read().split("\n")
    assert overall[0] == "EPE\tD1" and len(overall[1].split("\t")) == 2
    series = open(out / "series.csv").read().strip().split("\n")
    assert series[0] == "step\tEPE\tD1" and len(series) == 5
    assert open(out / "histogram.csv").read().startswith("Histogram\n[")
    assert os.path.exists(out / "disparities" / "disparity_2.png")
    ck = tf_checkpoint.latest_checkpoint(str(out / "weights"))
    assert ck and ck.endswith("model-4")
    r = tf_checkpoint.CheckpointReader(ck)
    from madnet_hip import engine as E
    names = [n for n, _ in E.madnet_manifest()]
    assert all(r.has_tensor(n) and r.has_tensor(n + "/Momentum") for n in names)


def test_adapter_dilation_updates_every_other_frame(hip):
    """--dilation K: the weights move only on frames with step % K == 0 (Stereo_Continual_Adaptation.py:205)."""
    import torch
    import Nets
    from madnet_hip import engine as E, synthetic as S
    from madnet_hip.adapter import Adapter
    H, W = 64, 128
    wn = S.calibrated_weights(dict(E.madnet_manifest()), 1)
    l, r, gt = S.make_pair(H, W)
    tl, tr, tg = (torch.from_numpy(a).cuda() for a in (l, r, gt[..., 0]))
    net = Nets.get_stereo_net("MADNet", {"left_img": tl, "right_img": tr, "split_layers": [None], "sequence": True,
                                         "train_portion": "BEGIN", "bulkhead": False, "weights": wn})
    ad = Adapter(net, mode="FULL", lr=1e-3, loss="proxy", dilation=2, ssim_th=1e9)
    px = tg.clone(); px[:, ::4] = 0
    moved = []
    for _ in range(4):
        w0 = net.engine.params.w.clone()
        out = ad.step(tl, tr, tg, proxy=px)
        assert np.isfinite(out["loss"])
        moved.append(not torch.equal(w0, net.engine.params.w))
    assert moved == [True, False, True, False]
    with pytest.raises(ValueError):
        ad.step(tl, tr, tg)                      # proxy labels are mandatory for loss='proxy'


def test_train_cli_end_to_end(hip, tmp_path):
    """Train.py plumbing: shuffled random-crop batches of 2, augmentation on, 3 steps of the multi-scale
    supervised loss + Adam in bf16 mode; train_log.csv and a TF checkpoint with the Adam slots that loads back as --weights."""
    import Train
    from Data_utils import tf_checkpoint
    lst = _make_list(tmp_path, 6, 140, 300)
    out = tmp_path / "train_out"
    os.makedirs(out)
    argv = ["--trainingSet", lst, "--validationSet", lst, "-o", str(out), "--weights", "calibrated:1", "--modelName", "MADNet",
            "--imageShape", "128", "256", "--batchSize", "2", "--numEpochs", "1", "--augment", "--lr", "1e-4",
            "--lossWeights", "1", "0.8", "0.6", "0.4", "0.2", "0.1"]
    Train.main(Train.build_parser().parse_args(argv))
    log = open(out / "train_log.csv").read().strip().split("\n")
    assert log[0] == "step,loss,EPE,bad3,val_EPE,val_bad3" and len(log) == 2 and log[1].startswith("0,")
    loss0 = float(log[1].split(",")[1])
    assert np.isfinite(loss0) and loss0 > 0 and log[1].split(",")[4] != ""
    ck = tf_checkpoint.latest_checkpoint(str(out)) or str(out / "weights.ckpt-3")
    rd = tf_checkpoint.CheckpointReader(ck)
    names = rd.get_variable_to_shape_map()
    assert int(rd.get_tensor("training_error/Variable")) == 3
    assert any(n.endswith("/Adam_1") for n in names)
    import Stereo_Online_Adaptation as SOA
    w = SOA.load_weights(ck, "MADNet")
    assert len(w) > 0 and all(np.isfinite(v).all() for v in w.values())

