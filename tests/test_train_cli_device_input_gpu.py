"""Train.py with the input prepared on the device: --prepareOn device --inputWorkers 2 --augment over 6 synthetic triples, the shapes of the Train case of
tests/test_cli_gpu.py (140x300 sources, 128x256 crops, batches of 2: 3 steps).  The raw 8-bit frames and the 16-bit disparities go up as they are;
mh_frame_prepare crops, augments and casts them on the prefetcher's copy stream; the validation batch takes the one-off form of the same call."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_train_cli_with_device_prepared_input(hip, tmp_path):
    import Train
    from Data_utils import tf_checkpoint
    from test_cli_gpu import _make_list
    lst = _make_list(tmp_path, 6, 140, 300)
    out = tmp_path / "train_out"
    os.makedirs(out)
    argv = ["--trainingSet", lst, "--validationSet", lst, "-o", str(out), "--weights", "calibrated:1", "--modelName", "MADNet",
            "--imageShape", "128", "256", "--batchSize", "2", "--numEpochs", "1", "--augment", "--lr", "1e-4",
            "--lossWeights", "1", "0.8", "0.6", "0.4", "0.2", "0.1", "--prepareOn", "device", "--inputWorkers", "2"]
    args = Train.build_parser().parse_args(argv)
    assert args.prepareOn == "device" and args.inputWorkers == 2
    Train.main(args)
    log = open(out / "train_log.csv").read().strip().split("\n")
    assert log[0] == "step,loss,EPE,bad3,val_EPE,val_bad3" and len(log) == 2 and log[1].startswith("0,")      # one row per 100 steps: step 0
    fields = log[1].split(",")
    assert all(np.isfinite(float(v)) for v in fields[1:]) and float(fields[1]) > 0                          # loss, EPE, bad3 and the validation pair
    ck = tf_checkpoint.latest_checkpoint(str(out)) or str(out / "weights.ckpt-3")
    rd = tf_checkpoint.CheckpointReader(ck)
    assert int(rd.get_tensor("training_error/Variable")) == 3                                               # 6 samples / batches of 2
    assert all(np.isfinite(rd.get_tensor(n)).all() for n in list(rd.get_variable_to_shape_map())[:8])
