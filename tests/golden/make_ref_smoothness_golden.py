"""Mints tests/golden/ref_smoothness.npz by EXECUTING the reference's own smoothness(x, y) (Losses/loss_factory.py:183-220, key 'smoothness' of its loss
table) under oracle/tf_shim's eager stand-in for tensorflow, on the seeded 36 x 52 recipe of make_ref_losses_golden.inputs(): its `left` as y, its last
prediction as x, and the gray mean of `left` as a one-channel y.  This script is its own child process: the child gets a module path of its own (the stand-in
and the reference in front, this repository's package out of the way) and imports the reference where it lies; nothing of the reference is restated here.
The stand-in lacks one constructor the function calls, tf.Variable(initial_value=, trainable=, dtype=): the child supplies it as a constant.

    python tests/golden/make_ref_smoothness_golden.py

ref_smoothness.npz: disp [1,H,W,1], image3 [1,H,W,3], image1 [1,H,W,1] (the inputs, so that a test needs no recipe), and
    loss_c3, grad_c3     smoothness(disp, image3) and its autograd gradient w.r.t. disp
    loss_c1, grad_c1     smoothness(disp, image1) likewise"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MADNET_REFERENCE_ROOT", "/root/reference")
PRED = "pred_5"          # the recipe's last prediction


def inputs():
    sys.path.insert(0, HERE)
    import make_ref_losses_golden as G
    z = G.inputs()
    assert z[PRED].shape == (1, 36, 52, 1)
    left = z["left"]
    return {"disp": z[PRED], "image3": left, "image1": left.mean(axis=-1, keepdims=True, dtype=np.float64).astype(np.float32)}


def check_inputs(z):
    """no pixel has 255 |gx| or 255 |gy| below 1e-3: the sign of every disparity gradient is decided in any arithmetic"""
    x = np.pad(z["disp"][0, :, :, 0].astype(np.float64), 1)
    H, W = x.shape[0] - 2, x.shape[1] - 2
    w = lambda i, j: x[i:i + H, j:j + W]
    gx = (w(0, 0) - w(0, 2)) + 2 * (w(1, 0) - w(1, 2)) + (w(2, 0) - w(2, 2))
    gy = (w(0, 0) + 2 * w(0, 1) - w(0, 2)) - (w(2, 0) + 2 * w(2, 1) + w(2, 2))
    assert min(np.abs(gx).min(), np.abs(gy).min()) >= 1e-3, "a pixel whose disparity gradient is within 1e-3 of zero"


def child(fin, fout):
    sys.dont_write_bytecode = True
    sys.path[:] = [os.path.join(ROOT, "oracle", "tf_shim"), REF] + [p for p in sys.path if p and os.path.abspath(p) not in (ROOT, HERE)
                                                                     and "real-time-self-adaptive-deep-stereo_amd" not in p]
    import torch
    import tensorflow as tf
    assert tf.__version__.endswith("shim") and tf.__file__.startswith(os.path.join(ROOT, "oracle"))
    tf.Variable = lambda initial_value=None, trainable=True, dtype=None: tf.constant(initial_value, dtype)       # (never trained: a constant)
    from Losses import loss_factory
    assert os.path.abspath(loss_factory.__file__).startswith(os.path.abspath(REF)), loss_factory.__file__
    assert loss_factory.SUPERVISED_LOSS["smoothness"] is loss_factory.smoothness
    z = np.load(fin)
    out = {}
    for tag in ("c3", "c1"):
        x = tf.constant(z["disp"], tf.float32)
        x.t.requires_grad_(True)
        loss = loss_factory.smoothness(x, tf.constant(z["image" + tag[1]], tf.float32))
        out["loss_" + tag] = np.float32(loss.t.detach().numpy())
        out["grad_" + tag] = torch.autograd.grad(loss.t, [x.t])[0].numpy()
    np.savez(fout, **out)


def run_reference(z):
    with tempfile.TemporaryDirectory() as td:
        fin, fout = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(fin, **z)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fin, fout], capture_output=True, text=True,
                            env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        if rc.returncode != 0:
            raise RuntimeError("the reference run failed:\n%s" % rc.stderr[-3000:])
        r = np.load(fout)
        return {k: r[k] for k in r.files}


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    z = inputs()
    check_inputs(z)
    ref = run_reference(z)
    ref.update(z)
    path = os.path.join(HERE, "ref_smoothness.npz")
    np.savez_compressed(path, **ref)
    print("%d arrays, %.1f KB; smoothness C = 3: %.9g, C = 1: %.9g" % (len(ref), os.path.getsize(path) / 1024.0, float(ref["loss_c3"]), float(ref["loss_c1"])))
