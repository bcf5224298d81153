"""mh_sgm_proxy_ex (eight-path aggregation and the 3x3 median of the label map) against tests/sgm8_oracle.py, the numpy restatement of the definition in
include/madnet_hip.h.

Pass rule without the median: that of tests/test_sgm_proxy.py -- the valid mask `out > 0` and floor(out) equal the oracle's exactly, `out` is within one float32
ulp of the oracle's value.  With the median: mask and floor are still exactly equal (floor is monotone, so it commutes with an order statistic), and
|delta| <= 2^-23 * 2^ceil(log2(max(m, 1))), m = the largest oracle label in the pixel's 3x3 window: an order statistic moves by at most the largest movement of
its inputs, and every input is within one ulp at its own magnitude <= m.  No pixel is excluded.

Frames come from madnet_hip.synthetic.make_pair (h > 20), smaller ones are windows of such a pair."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as FP
import sgm8_oracle
from madnet_hip import ops, synthetic as S

_frames, _ref = {}, {}

# name -> (B, H, W, D)
CASES = {
    "1x40x256_D128": (1, 40, 256, 128),                    # W > H: the diagonal lines are cut by top and bottom
    "2x23x131_D64": (2, 23, 131, 64),                      # odd sizes, two scenes: a wrong frame offset or a median across images shows
    "1x9x50_D64": (1, 9, 50, 64),                          # W < D, H just above the census window
    "1x60x11_D64": (1, 60, 11, 64),                        # H > W: the lines are cut by the sides
    "1x12x70_D192": (1, 12, 70, 192),                      # three disparities per lane
    "1x7x9_D64": (1, 7, 9, 64),                            # the smallest legal frame
}


def frames(name):
    """(left, right) uint8 [B,H,W,3] and gt [B,H,W] of a case, made once"""
    if name not in _frames:
        B, H, W, D = CASES[name]
        if name == "1x60x11_D64":
            pairs = [tuple(a[:, 2:62, 60:71] for a in S.make_pair(64, 128))]
        elif name == "1x12x70_D192":
            pairs = [tuple(a[:, :12, :70] for a in S.make_pair(23, 131, stream_id=0))]
        elif H > 20:
            pairs = [S.make_pair(H, W, stream_id=b) for b in range(B)]
        else:
            pairs = [tuple(a[:, 16:16 + H, 100:100 + W] for a in S.make_pair(40, 256))]
        l, r, g = (np.ascontiguousarray(np.concatenate([p[i] for p in pairs])) for i in range(3))
        assert l.shape == (B, H, W, 3)
        _frames[name] = (l.astype(np.uint8), r.astype(np.uint8), g[..., 0])
    return _frames[name]


def reference(name, paths, median):
    key = (name, paths)
    if key not in _ref:
        l, r, _ = frames(name)
        _ref[key] = sgm8_oracle.sgm_proxy(l, r, CASES[name][3], paths=paths, median=0)
        _ref[key].setflags(write=False)
    if not median:
        return _ref[key]
    if key + (1,) not in _ref:
        _ref[key + (1,)] = np.stack([sgm8_oracle.median3(o) for o in _ref[key]])
        _ref[key + (1,)].setflags(write=False)
    return _ref[key + (1,)]


def run(backend, l, r, D, paths, median, ws=None, **kw):
    dev = backend.device
    B, H, W, _ = l.shape
    lt, rt = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    ws = ops.sgm_proxy_ws(backend.lib, B, H, W, D, dev, paths=paths, median=median) if ws is None else ws
    out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
    ops.sgm_proxy(backend.lib, lt, rt, ws, out, D, paths=paths, median=median, **kw)
    backend.sync()
    return out.cpu().numpy(), ws


def check(got, ref, scale=None):
    """scale: the label whose magnitude sets the ulp (default: the oracle's value itself)"""
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got > 0, ref > 0), "valid masks differ at %d pixels" % np.count_nonzero((got > 0) != (ref > 0))
    assert np.all(got >= 0)
    assert np.array_equal(np.floor(got), np.floor(ref)), "integer disparities differ at %d pixels" % np.count_nonzero(np.floor(got) != np.floor(ref))
    scale = ref if scale is None else scale
    ulp = np.float64(2.0) ** -23 * 2.0 ** np.ceil(np.log2(np.maximum(scale.astype(np.float64), 1.0)))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("valid %d of %d, largest |delta| %.3g (bound there %.3g), pixels off at all: %d" % ((ref > 0).sum(), ref.size, d.max(), ulp.flat[d.argmax()], np.count_nonzero(d)))
    assert np.all(d <= ulp)


def check_case(got, name, paths, median):
    ref = reference(name, paths, median)
    if median:
        check(got, ref, scale=np.stack([sgm8_oracle.window_max(o) for o in reference(name, paths, 0)]))
    else:
        check(got, ref)


MODES = [(name, 8, m) for name in CASES for m in (0, 1)] + [("1x40x256_D128", 4, 1)]


@pytest.mark.parametrize("name,paths,median", MODES, ids=lambda v: str(v))
def test_sgm_proxy_ex_vs_oracle(backend, name, paths, median):
    l, r, _ = frames(name)
    got, _ = run(backend, l, r, CASES[name][3], paths, median)
    check_case(got, name, paths, median)


def test_sgm_median_takes_one_input_value():
    """the oracle's median on a hand-made map: rejected stays rejected, lower median of the valid neighbours, nothing from outside the frame"""
    m = np.array([[5, 0, 1], [0, 3, 9], [7, 0, 0]], np.float32)
    # (0,0): {3, 5} -> index 0;  (0,2) and (1,2): {1, 3, 9} -> index 1;  (1,1): {1, 3, 5, 7, 9} -> index 2;  (2,0): {3, 7} -> index 0
    want = np.array([[3, 0, 3], [0, 5, 3], [3, 0, 0]], np.float32)
    assert np.array_equal(sgm8_oracle.median3(m), want)


def test_sgm_ex_four_paths_no_median_is_mh_sgm_proxy(backend):
    """(4, 0) through the new entry: the same workspace size and the same bits as the old entry"""
    lib, dev = backend.lib, backend.device
    name = "2x23x131_D64"
    B, H, W, D = CASES[name]
    l, r, _ = frames(name)
    for shape in ((1, 7, 9, 64), (2, 23, 131, 64), (1, 375, 1242, 128), (3, 12, 129, 192)):
        assert lib.sgm_ws_bytes_ex(*shape, 4, 0) == lib.sgm_ws_bytes(*shape)
    lt, rt = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    outs = []
    for ex in (False, True):
        ws = ops.sgm_proxy_ws(lib, B, H, W, D, dev)
        out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        if ex:
            lib.sgm_proxy_ex(p(lt), p(rt), 1, p(ws), p(out), B, H, W, D, 10, 120, 95, 1, 4, 0, None)
        else:
            lib.sgm_proxy(p(lt), p(rt), 1, p(ws), p(out), B, H, W, D, 10, 120, 95, 1, None)
        backend.sync()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert (outs[0] > 0).any()


def test_sgm_ex_repeatable_and_dtype_independent(backend):
    """a second call into the same workspace gives the same bits; uint8 and float32 frames give the same bits"""
    name = "1x40x256_D128"
    l, r, _ = frames(name)
    D = CASES[name][3]
    got, ws = run(backend, l, r, D, 8, 1)
    again, _ = run(backend, l, r, D, 8, 1, ws=ws)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "a second call into the same workspace changed the result"
    asf, _ = run(backend, l.astype(np.float32), r.astype(np.float32), D, 8, 1, ws=ws)
    assert np.array_equal(asf.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("case", [(1, 7, 9, 64), (1, 9, 50, 64), (3, 12, 129, 192)], ids=lambda c: "x".join(map(str, c)))
def test_sgm_ex_exact_workspace(backend, case):
    """(8, 1) with ws of exactly mh_sgm_ws_bytes_ex bytes and guarded labels: guards intact, every label written; data as tests/test_workspace_guards.py makes it"""
    lib, dev = backend.lib, backend.device
    B, H, W, D = case
    rng = np.random.default_rng(sum(case))
    l = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    r = np.roll(l, -3, axis=2)
    r = np.ascontiguousarray(np.clip(r.astype(np.int32) + rng.integers(-6, 7, r.shape), 0, 255).astype(np.uint8))
    nbytes = lib.sgm_ws_bytes_ex(B, H, W, D, 8, 1)
    ws = FP.Guarded(nbytes, torch.uint8, dev)
    out = FP.Guarded(B * H * W, torch.float32, dev)
    assert ws.ptr() % 16 == 0
    ops.sgm_proxy(lib, torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev), ws.t, out.t, D, paths=8, median=True)
    backend.sync()
    ws.assert_guards("sgm ws %s (%d bytes)" % (case, nbytes))
    FP.assert_fully_written(out, B * H * W, "sgm labels %s" % (case,))
    raw = sgm8_oracle.sgm_proxy(l, r, D, paths=8, median=0)
    ref = np.stack([sgm8_oracle.median3(o) for o in raw])
    check(out.t.cpu().numpy().reshape(B, H, W), ref, scale=np.stack([sgm8_oracle.window_max(o) for o in raw]))


def test_sgm_ex_argument_checks(backend):
    lib, dev = backend.lib, backend.device
    B, H, W, D = 1, 9, 50, 64
    for paths in (4, 8):
        assert lib.sgm_ws_bytes_ex(0, H, W, D, paths, 1) == 0 and lib.sgm_ws_bytes_ex(B, -1, W, D, paths, 0) == 0
        assert lib.sgm_ws_bytes_ex(B, H, 0, D, paths, 0) == 0 and lib.sgm_ws_bytes_ex(B, H, W, 0, paths, 1) == 0
        for shape in ((B, H, W, D), (1, 7, 9, 64), (3, 11, 13, 192)):
            n0, n1 = lib.sgm_ws_bytes_ex(*shape, paths, 0), lib.sgm_ws_bytes_ex(*shape, paths, 1)
            assert n0 > 0 and n0 % 16 == 0 and n1 % 16 == 0 and n1 > n0, (shape, paths, n0, n1)
    assert lib.sgm_ws_bytes_ex(B, H, W, D, 8, 0) > lib.sgm_ws_bytes_ex(B, H, W, D, 4, 0)
    l = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
    ws = ops.sgm_proxy_ws(lib, B, H, W, D, dev, paths=8, median=True)
    out = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(left=p(l), right=p(l), u8=1, ws=p(ws), out=p(out), B=B, H=H, W=W, D=D, p1=10, p2=120, uniq=95, lr_tol=1, paths=8, median=1, stream=None)
    bad = [dict(paths=0), dict(paths=2), dict(paths=6), dict(paths=16), dict(median=-1), dict(median=2),
           dict(left=None), dict(right=None), dict(ws=None), dict(out=None), dict(B=0), dict(H=0), dict(W=0), dict(H=6), dict(W=8), dict(D=0), dict(D=256),
           dict(D=96), dict(p1=0), dict(p1=121), dict(p2=192, p1=10), dict(uniq=0), dict(uniq=101), dict(lr_tol=-1), dict(ws=C.c_void_p(ws.data_ptr() + 8))]
    for change in bad:
        a = dict(good, **change)
        rc = lib._raw_mh_sgm_proxy_ex(*a.values())
        assert rc != 0, change
        if "paths" in change or "median" in change:
            assert rc == -1, (change, rc)                # MH_ERR_ARG
        msg = lib.last_error().decode()
        assert msg.startswith("mh_sgm_proxy_ex: ") and len(msg) > len("mh_sgm_proxy_ex: "), (change, msg)
    backend.sync()
    assert bool((out == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_sgm_proxy_ex(*good.values()) == 0
    backend.sync()
    assert bool((out == 0).all())                       # flat frames: every cost ties, d1 = 0 everywhere -> rejected, and every element is written
    with pytest.raises(AssertionError):
        ops.sgm_proxy(lib, l, l, ops.sgm_proxy_ws(lib, B, H, W, D, dev), out, D, paths=8, median=True)      # a four-path workspace is too small


def _quality(out, gt):
    valid = out > 0
    both = valid & (gt > 0)
    err = np.abs(out - gt)[both]
    return valid.mean(), (err > 3).mean(), err.mean()


def test_sgm_oracle_eight_paths_and_median_improve_the_labels():
    """Asserted on the oracle only (no library, no backend); the equality tests above carry it over to the kernels.  128 x 416, D = 64, stream_id = 0; a numpy
    draft of the definition gave valid / bad3 / EPE  0.865 / 0.0129 / 0.602 (4 paths), 0.861 / 0.0090 / 0.529 (8), 0.861 / 0.0091 / 0.499 (8 + median).
    Conditions, not tolerances."""
    l, r, gt = S.make_pair(128, 416, stream_id=0)
    l, r, gt = l.astype(np.uint8), r.astype(np.uint8), gt[0, :, :, 0]
    o4 = sgm8_oracle.sgm_proxy(l, r, 64, paths=4)[0]
    o8 = sgm8_oracle.sgm_proxy(l, r, 64, paths=8)[0]
    o8m = sgm8_oracle.median3(o8)
    q4, q8, q8m = _quality(o4, gt), _quality(o8, gt), _quality(o8m, gt)
    for tag, q in (("4 paths", q4), ("8 paths", q8), ("8 paths + median", q8m)):
        print("%-17s valid %.3f  bad3 %.4f  EPE %.3f" % ((tag,) + q))
    assert q8[1] < q4[1]
    assert q8[0] >= q4[0] - 0.01
    assert q8m[2] < q8[2]
    assert q8m[0] == q8[0]
