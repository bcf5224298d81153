"""mh_sgm_proxy (census + four-path semi-global matching, the continual loop's proxy labels on the device) against tests/sgm_oracle.py, the numpy restatement
of the definition in include/madnet_hip.h.

Pass rule: the valid mask `out > 0` and floor(out) of the valid pixels equal the oracle's exactly (everything up to the sub-pixel step is integer arithmetic);
`out` itself is within one float32 ulp of the oracle's value, |delta| <= 2^-23 * 2^ceil(log2(max(out, 1))) -- derived, not measured: both sides do one
correctly rounded float32 division and one add of integers, the bound allows for a fused or reordered final add and nothing else.  No pixel is excluded.  A
second call into the same workspace gives the same bits.

Frames come from madnet_hip.synthetic.make_pair.  make_pair needs h > 20 (its rectangles), so the 9 x 50 case is a window of the 40 x 256 pair: same
generator, W < D and H barely above the census height as the case asks."""
import ctypes as C

import numpy as np
import pytest
import torch

import sgm_oracle
from madnet_hip import ops, synthetic as S

_frames, _ref = {}, {}


def frames(case):
    """(left, right) uint8 [B,H,W,3] and gt [B,H,W] of a case, made once"""
    if case not in _frames:
        B, H, W, D = case
        if H > 20:
            pairs = [S.make_pair(H, W, stream_id=b) for b in range(B)]       # frame 1 is another scene: a wrong batch offset shows
        else:
            l, r, g = S.make_pair(40, 256)
            pairs = [(l[:, 16:16 + H, 100:100 + W], r[:, 16:16 + H, 100:100 + W], g[:, 16:16 + H, 100:100 + W])]
        _frames[case] = tuple(np.ascontiguousarray(np.concatenate([p[i] for p in pairs])) for i in range(3))
        _frames[case] = (_frames[case][0].astype(np.uint8), _frames[case][1].astype(np.uint8), _frames[case][2][..., 0])
    return _frames[case]


def reference(case):
    if case not in _ref:
        l, r, _ = frames(case)
        _ref[case] = sgm_oracle.sgm_proxy(l, r, case[3])
        _ref[case].setflags(write=False)
    return _ref[case]


def run(backend, l, r, D, ws=None, **kw):
    dev = backend.device
    B, H, W, _ = l.shape
    lt, rt = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    ws = ops.sgm_proxy_ws(backend.lib, B, H, W, D, dev) if ws is None else ws
    out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
    ops.sgm_proxy(backend.lib, lt, rt, ws, out, D, **kw)
    backend.sync()
    return out.cpu().numpy(), ws


def check(got, ref):
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got > 0, ref > 0), "valid masks differ at %d pixels" % np.count_nonzero((got > 0) != (ref > 0))
    assert np.all(got >= 0)
    assert np.array_equal(np.floor(got), np.floor(ref)), "integer disparities differ at %d pixels" % np.count_nonzero(np.floor(got) != np.floor(ref))
    ulp = np.float64(2.0) ** -23 * 2.0 ** np.ceil(np.log2(np.maximum(ref.astype(np.float64), 1.0)))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("largest |delta| %.3g (bound there %.3g), pixels off at all: %d" % (d.max(), ulp.flat[d.argmax()], np.count_nonzero(d)))
    assert np.all(d <= ulp)


CASES = [(1, 40, 256, 128), (2, 23, 131, 64), (1, 9, 50, 64)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_sgm_proxy_vs_oracle(backend, case):
    l, r, _ = frames(case)
    ref = reference(case)
    got, ws = run(backend, l, r, case[3])
    check(got, ref)
    again, _ = run(backend, l, r, case[3], ws=ws)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "a second call into the same workspace changed the result"
    if case == CASES[0]:                                   # the same frame as float32 gives the identical result
        asf, _ = run(backend, l.astype(np.float32), r.astype(np.float32), case[3], ws=ws)
        assert np.array_equal(asf.view(np.uint32), got.view(np.uint32))


def test_sgm_oracle_is_a_usable_matcher():
    """asserted on the oracle only; the equality above carries it over to the kernels.  A numpy draft of the definition gave 0.675 / 0.052 on this fixture."""
    case = CASES[0]
    ref, gt = reference(case)[0], frames(case)[2][0]
    valid = ref > 0
    both = valid & (gt > 0)
    share, bad = valid.mean(), (np.abs(ref - gt)[both] > 3).mean()
    print("valid share %.3f, off by more than 3 px among valid pixels with ground truth %.3f (%d pixels)" % (share, bad, both.sum()))
    assert share >= 0.5
    assert both.sum() > 0 and bad <= 0.10


def test_sgm_float_frames_round_to_nearest(backend):
    """float32 frames that are not integers: u = clamp(floor(x + 0.5), 0, 255), as the oracle states it"""
    case = CASES[2]
    l, r, _ = frames(case)
    rng = np.random.default_rng(5)
    lf = (l.astype(np.float32) + rng.uniform(-0.7, 0.7, l.shape).astype(np.float32)) * np.float32(1.02) - np.float32(2)
    rf = (r.astype(np.float32) + rng.uniform(-0.7, 0.7, r.shape).astype(np.float32)) * np.float32(1.02) - np.float32(2)
    got, _ = run(backend, lf, rf, case[3])
    check(got, sgm_oracle.sgm_proxy(lf, rf, case[3]))


def test_sgm_parameters_reach_the_kernels(backend):
    """non-default penalties, uniqueness and tolerance, and D = 192 (three disparities per lane)"""
    l, r, _ = frames(CASES[1])
    l, r = l[:1, :12, :70], r[:1, :12, :70]
    l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
    for D, kw in ((192, {}), (64, dict(p1=3, p2=40, uniq=80, lr_tol=0))):
        got, _ = run(backend, l, r, D, **kw)
        check(got, sgm_oracle.sgm_proxy(l, r, D, **kw))


def test_sgm_argument_checks(backend):
    lib, dev = backend.lib, backend.device
    B, H, W, D = 1, 9, 50, 64
    assert lib.sgm_ws_bytes(B, H, W, D) == 2 * 8 * H * W + 4 * H * W * D + (H * W + 15) // 16 * 16 and lib.sgm_ws_bytes(0, H, W, D) == 0
    l = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev)
    ws = ops.sgm_proxy_ws(lib, B, H, W, D, dev)
    out = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(left=p(l), right=p(l), u8=1, ws=p(ws), out=p(out), B=B, H=H, W=W, D=D, p1=10, p2=120, uniq=95, lr_tol=1, stream=None)
    bad = [dict(left=None), dict(right=None), dict(ws=None), dict(out=None), dict(B=0), dict(H=0), dict(W=0), dict(H=6), dict(W=8), dict(D=0), dict(D=256),
           dict(D=96), dict(p1=0), dict(p1=121), dict(p2=192, p1=10), dict(uniq=0), dict(uniq=101), dict(lr_tol=-1), dict(ws=C.c_void_p(ws.data_ptr() + 8))]
    for change in bad:
        a = dict(good, **change)
        assert lib._raw_mh_sgm_proxy(*a.values()) != 0, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_sgm_proxy: ") and len(msg) > len("mh_sgm_proxy: "), (change, msg)
    backend.sync()
    assert bool((out == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_sgm_proxy(*good.values()) == 0
    backend.sync()
    assert bool((out == 0).all())                       # flat frames: every cost ties, d1 = 0 everywhere -> rejected, and every element is written
