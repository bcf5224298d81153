"""mh_sgm_speckle (the speckle filter behind the on-device SGM matcher: 4-connected components of the valid labels, the small ones set to 0) against
tests/sgm_speckle_oracle.py, a flood-fill restatement of the definition in include/madnet_hip.h.

Pass rule: the filter copies labels or writes 0 and counts pixels -- there is no arithmetic to round, so the output equals the oracle's bit for bit
(compared as int32).  The frame sizes (2, 67, 131) and (1, 130, 259) are no multiple of 32 and cross every tile up to 64 wide or high at least twice."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as FP
import sgm8_oracle
import sgm_oracle
import sgm_speckle_oracle as SO
from madnet_hip import ops, synthetic as S
from madnet_hip.proxy import ProxyMatcher

SHAPES = [(2, 67, 131), (1, 130, 259)]
MH_ERR_ARG, MH_ERR_ALIGN = -1, -2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run(backend, labels, max_size, max_diff=1.0, out_fill=float("nan"), ws_fill=None, inplace=False):
    """-> the filtered map as numpy; out prefilled with out_fill, ws (exactly the queried size) with the byte ws_fill"""
    dev = backend.device
    t = torch.from_numpy(np.array(labels, dtype=np.float32)).to(dev)            # a copy: the fixtures are read-only
    B, H, W = t.shape
    ws = ops.sgm_speckle_ws(backend.lib, B, H, W, dev)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    out = t if inplace else torch.full((B, H, W), out_fill, dtype=torch.float32, device=dev)
    ops.sgm_speckle(backend.lib, t, out, ws, max_size, max_diff)
    backend.sync()
    return out.cpu().numpy()


def check(backend, labels, max_size, max_diff=1.0, ref=None, **kw):
    ref = SO.speckle(labels, max_size, max_diff) if ref is None else ref
    got = run(backend, labels, max_size, max_diff, **kw)
    diff = bits(got) != bits(ref)
    assert not diff.any(), "%d pixels differ from the oracle (first at %s): max_size %d, max_diff %g" % (diff.sum(), np.argwhere(diff)[0].tolist(), max_size, max_diff)
    return ref


# ---- the hand-built maps, made once --------------------------------------------------------------------------------------------------------------
_maps = {}


def blobs(shape):
    """piecewise-constant blobs (a coarse grid of levels, stretched by 5 x 9) plus noise of a few quarter pixels, 30 % holes at exactly 0, a few negative and
    NaN pixels"""
    if ("blobs", shape) not in _maps:
        B, H, W = shape
        rng = np.random.default_rng(H * 1000 + W)
        coarse = rng.integers(2, 40, (B, H // 5 + 1, W // 9 + 1)).astype(np.float32)
        m = np.repeat(np.repeat(coarse, 5, axis=1), 9, axis=2)[:, :H, :W]
        m = m + rng.integers(-2, 3, m.shape).astype(np.float32) * np.float32(0.25)
        m[rng.random(m.shape) < 0.30] = 0.0
        bad = rng.random(m.shape)
        m[bad < 0.004] = -3.0
        m[(bad >= 0.004) & (bad < 0.008)] = np.nan
        m.setflags(write=False)
        _maps[("blobs", shape)] = m
    return _maps[("blobs", shape)]


def serpentine(H, W, vertical=False):
    """-> the pixel coordinates (y, x), in walking order, of a one-pixel-wide serpentine through the whole frame: every second row from end to end, joined to the
    next at alternating ends (vertical: the same along columns)"""
    if vertical:
        return [(y, x) for x, y in serpentine(W, H)]
    path = []
    for k, y in enumerate(range(0, H, 2)):
        xs = range(W) if k % 2 == 0 else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < H:
            path.append((y + 1, W - 1 if k % 2 == 0 else 0))
    return path


def paint(shape, path, value=7.5):
    m = np.zeros(shape, np.float32)
    ys, xs = zip(*path)
    m[0, list(ys), list(xs)] = value
    return m


# ---- 1. oracle equality --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_speckle_blobs_vs_oracle(backend, shape):
    m = blobs(shape)
    for max_size, max_diff in ((20, 1.0), (8, 0.25), (3, 2.0)):
        ref = check(backend, m, max_size, max_diff)
        valid = np.nan_to_num(m, nan=0.0) > 0
        kept = ref > 0
        print("blobs %s size %d range %g: %d valid, %d kept" % (shape, max_size, max_diff, valid.sum(), kept.sum()))
        assert 0 < kept.sum() < valid.sum(), "the fixture must have components on both sides of max_size"


@pytest.mark.parametrize("vertical", [False, True], ids=["rows", "columns"])
def test_speckle_long_chain_is_one_component(backend, vertical):
    """the serpentine is ONE component of about 17 000 pixels: kept at any max_size below its length, removed at its length"""
    shape = (1, 130, 259)
    path = serpentine(shape[1], shape[2], vertical)
    m = paint(shape, path)
    n = len(path)
    assert n > 16000 and len(SO.components(m[0])) == 1
    for max_size in (100, n - 1):
        ref = check(backend, m, max_size)
        assert np.array_equal(ref, m)
    ref = check(backend, m, n)
    assert not ref.any()


@pytest.mark.parametrize("vertical", [False, True], ids=["rows", "columns"])
def test_speckle_chain_cut_into_pieces_at_the_size_limit(backend, vertical):
    """the serpentine cut by single holes into pieces of exactly max_size pixels (removed) and max_size + 1 pixels (kept), alternately; a period of
    2 max_size + 3 = 77 pixels against tiles of 8 .. 64 puts pieces across tile borders and, at the serpentine's turns, across tile corners"""
    shape, max_size = (1, 130, 259), 37
    path = serpentine(shape[1], shape[2], vertical)
    m = np.zeros(shape, np.float32)
    want = np.zeros(shape, np.float32)
    i, k = 0, 0
    while i < len(path):
        n = max_size + (k & 1)
        piece = path[i:i + n]
        for j, (y, x) in enumerate(piece):
            m[0, y, x] = 5.0 + 0.5 * ((i + j) % 3)                      # neighbours differ by 0.5 or 1.0: connected at max_diff 1
            if len(piece) > max_size:
                want[0, y, x] = m[0, y, x]
        i += n + 1                                                      # one hole
        k += 1
    ref = check(backend, m, max_size)
    assert np.array_equal(ref, want), "the oracle departs from the construction"
    assert (want > 0).sum() > 4000 and ((m > 0) & (want == 0)).sum() > 4000


def test_speckle_no_wrap_between_rows_or_images(backend):
    """equal valid labels at (y, W - 1) and (y + 1, 0), and at the last pixel of image 0 and the first of image 1: four isolated pixels.  At max_size 1 a pixel
    that joined its wrap neighbour would survive; a genuine pair does"""
    B, H, W = 2, 67, 131
    m = np.zeros((B, H, W), np.float32)
    m[0, 10, W - 1] = m[0, 11, 0] = 4.0
    m[1, 63, W - 1] = m[1, 64, 0] = 4.0                                 # the same across a tile border of rows
    m[0, H - 1, W - 1] = m[1, 0, 0] = 6.0
    m[1, 30, 63] = m[1, 30, 64] = 9.0                                   # the control: a real pair
    want = np.zeros_like(m)
    want[1, 30, 63] = want[1, 30, 64] = 9.0
    ref = check(backend, m, 1)
    assert np.array_equal(ref, want)


def test_speckle_range_boundary(backend):
    """labels are multiples of 0.5, max_diff = 1.0: a difference of exactly 1.0 connects, 1.5 does not, a ramp of two steps of 1.0 is one component although
    its ends differ by 2.  Each figure once inside a tile and once across the borders of tiles 16, 32 and 64 wide or high"""
    B, H, W = 1, 67, 131
    m = np.zeros((B, H, W), np.float32)
    want1 = np.zeros_like(m)                                            # max_size 1: pairs and ramps survive
    want2 = np.zeros_like(m)                                            # max_size 2: ramps only
    for y0, x0 in ((3, 3), (15, 63), (31, 31), (40, 127)):
        m[0, y0, x0:x0 + 2] = (2.0, 3.0)                                # 1.0: connected
        want1[0, y0, x0:x0 + 2] = (2.0, 3.0)
        m[0, y0 + 2, x0:x0 + 2] = (2.0, 3.5)                            # 1.5: two single pixels
        m[0, y0 + 4, x0 - 1:x0 + 2] = (1.0, 2.0, 3.0)                   # a ramp along the row
        want1[0, y0 + 4, x0 - 1:x0 + 2] = want2[0, y0 + 4, x0 - 1:x0 + 2] = (1.0, 2.0, 3.0)
    for y0, x0 in ((14, 10), (30, 70), (62, 64)):
        m[0, y0:y0 + 3, x0] = (6.5, 5.5, 4.5)                           # a ramp down a column, across a row border
        want1[0, y0:y0 + 3, x0] = want2[0, y0:y0 + 3, x0] = (6.5, 5.5, 4.5)
        m[0, y0:y0 + 2, x0 + 2] = (8.0, 9.5)                            # 1.5 down a column
    assert np.array_equal(check(backend, m, 1), want1)
    assert np.array_equal(check(backend, m, 2), want2)


def test_speckle_degenerate_maps(backend):
    B, H, W = 2, 67, 131
    dead = np.zeros((B, H, W), np.float32)
    dead[0, ::3] = -1.0
    dead[1, :, ::5] = np.nan
    assert not check(backend, dead, 0).any()                            # all invalid: all zeros
    const = np.full((B, H, W), 3.25, np.float32)
    assert np.array_equal(check(backend, const, H * W - 1), const)      # a constant valid map comes back unchanged: each frame is one component of H W pixels
    m = blobs((B, H, W))
    ref = check(backend, m, 0)                                          # max_size 0: the valid labels, 0 elsewhere
    assert np.array_equal(bits(ref), bits(np.where(np.nan_to_num(m, nan=0.0) > 0, m, np.float32(0))))
    for big in (B * H * W, 2 ** 31 - 1):
        assert not check(backend, const, big).any()                     # max_size >= B H W: all zeros
        assert not check(backend, m, big).any()
    for shape in ((1, 1, 1), (1, 1, 300), (1, 300, 1)):                 # the smallest frame, one row, one column
        line = np.full(shape, 2.0, np.float32)
        n = line.size
        assert np.array_equal(check(backend, line, n - 1), line)
        assert not check(backend, line, n).any()
        if n > 1:
            line.reshape(-1)[[7, 130, 131, 200]] = (0.0, np.nan, 9.0, -2.0)          # pieces of 7, 122, (one pixel of 9), 68, 99
            ref = check(backend, line, 68)
            assert (ref > 0).sum() == 122 + 99


# ---- 2. every element written, and reproducible ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_speckle_writes_every_element_whatever_out_and_ws_held(backend, shape):
    m = blobs(shape)
    ref = SO.speckle(m, 20, 1.0)
    for out_fill, ws_fill in ((float("nan"), 0xFF), (1e30, 0x00), (float("nan"), 0x00), (1e30, 0xFF)):
        check(backend, m, 20, 1.0, ref=ref, out_fill=out_fill, ws_fill=ws_fill)
    check(backend, m.copy(), 20, 1.0, ref=ref, inplace=True, ws_fill=0xFF)      # out == labels


# ---- 3. exact guarded workspace --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_speckle_exact_guarded_workspace(backend, shape):
    lib, dev = backend.lib, backend.device
    B, H, W = shape
    m = blobs(shape) if shape in SHAPES else np.full(shape, 2.0, np.float32)
    nbytes = lib.sgm_speckle_ws_bytes(B, H, W)
    assert nbytes == 2 * FP.round_up(B * H * W * 4, 16)
    ws = FP.Guarded(nbytes, torch.uint8, dev)
    out = FP.Guarded(B * H * W, torch.float32, dev)
    assert ws.ptr() % 16 == 0
    t = torch.from_numpy(np.array(m)).to(dev)
    ops.sgm_speckle(lib, t, out.t, ws.t, 20, 1.0)
    backend.sync()
    ws.assert_guards("speckle ws %s (%d bytes)" % (shape, nbytes))
    FP.assert_fully_written(out, B * H * W, "speckle labels %s" % (shape,))
    assert np.array_equal(bits(out.t.cpu().numpy().reshape(shape)), bits(SO.speckle(m, 20, 1.0)))
    with pytest.raises(AssertionError, match="workspace too small"):
        ops.sgm_speckle(lib, t, out.t, ws.t[:nbytes - 1], 20, 1.0)


# ---- 4. argument checks ----------------------------------------------------------------------------------------------------------------------------
def test_speckle_argument_checks(backend):
    lib, dev = backend.lib, backend.device
    B, H, W = 1, 9, 50
    assert lib.sgm_speckle_ws_bytes(B, H, W) == 2 * FP.round_up(H * W * 4, 16)       # each part rounded up to 16 bytes
    for dims in ((0, H, W), (B, 0, W), (B, H, 0), (-1, H, W), (B, -3, W), (B, H, -2)):
        assert lib.sgm_speckle_ws_bytes(*dims) == 0
    lab = torch.full((B, H, W), 2.0, device=dev)
    ws = torch.empty(lib.sgm_speckle_ws_bytes(B, H, W) + 16, dtype=torch.uint8, device=dev)
    out = torch.full((B, H, W), -7.0, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(labels=p(lab), out=p(out), ws=p(ws), B=B, H=H, W=W, max_size=5, max_diff=1.0, stream=None)
    bad = [(dict(labels=None), MH_ERR_ARG), (dict(out=None), MH_ERR_ARG), (dict(ws=None), MH_ERR_ARG), (dict(B=0), MH_ERR_ARG), (dict(H=0), MH_ERR_ARG),
           (dict(W=0), MH_ERR_ARG), (dict(B=-1), MH_ERR_ARG), (dict(max_size=-1), MH_ERR_ARG), (dict(max_diff=-0.5), MH_ERR_ARG),
           (dict(max_diff=float("nan")), MH_ERR_ARG), (dict(max_diff=float("inf")), MH_ERR_ARG), (dict(ws=C.c_void_p(ws.data_ptr() + 8)), MH_ERR_ALIGN)]
    for change, code in bad:
        a = dict(good, **change)
        assert lib._raw_mh_sgm_speckle(*a.values()) == code, change
        msg = lib.last_error().decode()
        assert msg.startswith("mh_sgm_speckle: ") and len(msg) > len("mh_sgm_speckle: "), (change, msg)
    backend.sync()
    assert bool((out == -7.0).all()), "a refused call launched something"
    assert lib._raw_mh_sgm_speckle(*good.values()) == 0
    backend.sync()
    assert bool((out == 2.0).all())


# ---- 5. through ProxyMatcher -----------------------------------------------------------------------------------------------------------------------
FIX = (1, 40, 256, 128)                                                 # the fixture frame of tests/test_sgm_proxy.py
_fix = {}


def fixture_frames():
    if "frames" not in _fix:
        l, r, g = S.make_pair(FIX[1], FIX[2], stream_id=0)
        _fix["frames"] = (l.astype(np.uint8), r.astype(np.uint8), g[..., 0])
    return _fix["frames"]


def fixture_labels(paths=4, median=False):
    """the oracle matcher's labels on the fixture frame, made once"""
    key = ("labels", paths, median)
    if key not in _fix:
        l, r, _ = fixture_frames()
        o = sgm_oracle.sgm_proxy(l, r, FIX[3]) if (paths, median) == (4, False) else sgm8_oracle.sgm_proxy(l, r, FIX[3], paths=paths, median=int(median))
        o.setflags(write=False)
        _fix[key] = o
    return _fix[key]


def check_labels(got, ref):
    """the pass rule of tests/test_sgm_proxy.py for matcher labels (the sub-pixel step is one float32 division and one add: within one ulp), on top of
    identical valid masks -- the filter must have removed exactly the oracle's pixels"""
    assert np.array_equal(got > 0, ref > 0), "valid masks differ at %d pixels" % np.count_nonzero((got > 0) != (ref > 0))
    assert np.array_equal(np.floor(got), np.floor(ref))
    ulp = np.float64(2.0) ** -23 * 2.0 ** np.ceil(np.log2(np.maximum(ref.astype(np.float64), 1.0)))
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print("largest |delta| %.3g, pixels off at all: %d" % (d.max(), np.count_nonzero(d)))
    assert np.all(d <= ulp)


@pytest.mark.parametrize("paths,median", [(4, False), (8, True)], ids=["4paths", "8paths-median"])
def test_matcher_with_speckle_filter(backend, paths, median):
    lib, dev = backend.lib, backend.device
    l, r, _ = fixture_frames()
    lt, rt = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    plain = ProxyMatcher(lib, 1, FIX[1], FIX[2], max_disp=FIX[3], device=dev, paths=paths, median=median)
    m = ProxyMatcher(lib, 1, FIX[1], FIX[2], max_disp=FIX[3], device=dev, paths=paths, median=median, speckle_size=50)
    assert m.ws.numel() == plain.ws.numel() == lib.sgm_ws_bytes_ex(1, FIX[1], FIX[2], FIX[3], paths, int(median))
    assert m.params == plain.params and set(m.params) == {"p1", "p2", "uniq", "lr_tol", "paths", "median"}
    assert m.speckle_ws.numel() == lib.sgm_speckle_ws_bytes(1, FIX[1], FIX[2])
    raw = plain.compute(lt, rt)
    got = m.compute(lt, rt)
    backend.sync()
    raw, got = raw.cpu().numpy(), got.cpu().numpy()
    ref = SO.speckle(fixture_labels(paths, median), 50, 1.0)
    print("valid labels: %d unfiltered, %d filtered" % ((raw > 0).sum(), (got > 0).sum()))
    assert 0 < (ref > 0).sum() < (fixture_labels(paths, median) > 0).sum()
    check_labels(got, ref)
    assert np.array_equal(bits(got), bits(SO.speckle(raw, 50, 1.0))), "the filter of the device's own labels, bit for bit"


def test_matcher_default_runs_no_filter(backend):
    """speckle_size = 0 (the default): no workspace of the filter, the matcher's workspace unchanged, and the bits of ops.sgm_proxy"""
    lib, dev = backend.lib, backend.device
    l, r, _ = fixture_frames()
    lt, rt = torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)
    m = ProxyMatcher(lib, 1, FIX[1], FIX[2], max_disp=FIX[3], device=dev)
    assert m.speckle_ws is None and m.speckle_size == 0 and m.speckle_range == 1.0
    assert m.ws.numel() == lib.sgm_ws_bytes(1, FIX[1], FIX[2], FIX[3])
    calls, real = [], ops.sgm_speckle
    ops.sgm_speckle = lambda *a, **k: calls.append(a)
    try:
        got = m.compute(lt, rt)
    finally:
        ops.sgm_speckle = real
    direct = torch.full((1, FIX[1], FIX[2]), -7.0, dtype=torch.float32, device=dev)
    ops.sgm_proxy(lib, lt, rt, ops.sgm_proxy_ws(lib, 1, FIX[1], FIX[2], FIX[3], dev), direct, FIX[3])
    backend.sync()
    assert calls == []
    assert np.array_equal(bits(got.cpu().numpy()), bits(direct.cpu().numpy()))


# ---- 6. oracle quality conditions (oracle only: they keep the fixtures honest) -----------------------------------------------------------------------
def _quality(o, gt):
    valid = o > 0
    both = valid & (gt > 0)
    return valid.mean(), (np.abs(o - gt)[both] > 3).mean()


def test_speckle_oracle_removes_gross_errors():
    """conditions from the numbers measured on these scenes with the oracles (four paths, D = 128): 96 x 320, filter (100, 1.0): bad-3 0.021 -> 0.014, valid
    share 0.825 -> 0.814; 40 x 256, filter (50, 1.0): bad-3 0.052 -> 0.021"""
    l, r, gt = S.make_pair(96, 320)
    o = sgm_oracle.sgm_proxy(l.astype(np.uint8), r.astype(np.uint8), 128)
    f = SO.speckle(o, 100, 1.0)
    (v0, b0), (v1, b1) = _quality(o[0], gt[0, :, :, 0]), _quality(f[0], gt[0, :, :, 0])
    print("96x320: valid %.3f -> %.3f, bad3 %.4f -> %.4f" % (v0, v1, b0, b1))
    assert b1 < b0
    assert v0 - v1 <= 0.02
    o, gt = fixture_labels(), fixture_frames()[2]
    f = SO.speckle(o, 50, 1.0)
    (v0, b0), (v1, b1) = _quality(o[0], gt[0]), _quality(f[0], gt[0])
    print("40x256: valid %.3f -> %.3f, bad3 %.4f -> %.4f" % (v0, v1, b0, b1))
    assert b1 < 0.03 and b1 < b0
