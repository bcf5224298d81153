"""Data_utils/preprocessing.random_crop / augment: the reference's names and argument order (preprocessing.py:31-89) on device tensors, over mh_frame_prepare.
Runs on the CPU emulator (CPU tensors) and, marked gpu, on the product library."""
import numpy as np
import pytest
import torch

from Data_utils import data_reader, preprocessing
from test_frame_prepare import Fixed, augment64


@pytest.fixture
def pre(backend, monkeypatch):
    monkeypatch.setattr(preprocessing, "_lib", lambda: backend.lib)
    return backend


def _coded(H, W):
    """left codes its own coordinates (row, column, row + column), right = 255 - left, gt = 100 row + column"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    left = np.stack([yy, xx, yy + xx], -1).astype(np.uint8)
    return left, 255 - left, (100.0 * yy + xx).astype(np.float32)[..., None]


def test_random_crop_windows_are_aligned_within_bounds_and_never_the_last_offset(pre):
    H, W, ch, cw = 20, 30, 15, 22
    left, right, gt = _coded(H, W)
    t = [torch.from_numpy(a).to(pre.device) for a in (left, right, gt)]
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(40):
        l, r, g = preprocessing.random_crop([ch, cw], t, rng)
        assert l.dtype == torch.float32 and tuple(l.shape) == (ch, cw, 3) and tuple(r.shape) == (ch, cw, 3) and tuple(g.shape) == (ch, cw, 1)
        l, r, g = l.cpu().numpy(), r.cpu().numpy(), g.cpu().numpy()
        r0, c0 = int(l[0, 0, 0]), int(l[0, 0, 1])
        seen.add((r0, c0))
        # the reference's bounds: uniform in [0, H - ch - 1) x [0, W - cw - 1); the last admissible offsets H - ch = 5 and W - cw = 8 (and 4, 7) never come
        assert 0 <= r0 < H - ch - 1 and 0 <= c0 < W - cw - 1
        assert np.array_equal(l, left[r0:r0 + ch, c0:c0 + cw].astype(np.float32))
        assert np.array_equal(r, right[r0:r0 + ch, c0:c0 + cw].astype(np.float32)) and np.array_equal(g, gt[r0:r0 + ch, c0:c0 + cw])
    assert len({s[0] for s in seen}) > 1 and len({s[1] for s in seen}) > 1
    # the draw is the host path's: same generator state, same window
    a = preprocessing.random_crop([ch, cw], t, np.random.default_rng(8))[0].cpu().numpy()
    b = data_reader.random_crop([ch, cw], [left.astype(np.float32)], np.random.default_rng(8))[0]
    assert np.array_equal(a, b)
    # an image one row / column larger than the crop: the bound H - ch - 1 = 0 becomes 1, the origin is 0
    l = preprocessing.random_crop([H - 1, W - 1], t, rng)[0].cpu().numpy()
    assert np.array_equal(l, left[:H - 1, :W - 1].astype(np.float32))
    with pytest.raises(ValueError):
        preprocessing.random_crop([H + 1, W], t, rng)


def test_augment_applies_identical_parameters_to_both_views(pre):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (15, 22, 3), dtype=np.uint8)
    other = rng.integers(0, 256, (15, 22, 3), dtype=np.uint8)
    ti, to = torch.from_numpy(img).to(pre.device), torch.from_numpy(other).to(pre.device)
    draws = [[0.9, 0.1, 0.1, 0.1], 0.031, 0.87, 1.12]              # brightness, contrast and hue all active
    a, b = preprocessing.augment(ti, ti, Fixed(draws))
    assert a.dtype == torch.float32 and tuple(a.shape) == (15, 22, 3) and torch.equal(a, b)        # the same view twice: the same result
    assert not np.allclose(a.cpu().numpy(), img.astype(np.float32), atol=1.0)
    a2, c = preprocessing.augment(ti, to, Fixed(draws))
    assert torch.equal(a2, a)                                      # a view's result does not depend on the other view
    hl, hr = data_reader.augment(img.astype(np.float32), other.astype(np.float32), Fixed(draws))
    for got, host, src in ((a2, hl, img), (c, hr, other)):         # ... and is the host statement's with these parameters (rule of tests/test_frame_prepare.py)
        y = augment64(src, 7, *draws[1:])
        assert np.abs(got.cpu().numpy().astype(np.float64) - y).max() <= 2.0 * np.abs(host.astype(np.float64) - y).max()
    # nothing active: the cast alone; without contrast: the host's bits
    a, b = preprocessing.augment(ti, to, Fixed([[0.9, 0.9, 0.9, 0.9], 0.05, 1.2, 1.2]))
    assert np.array_equal(a.cpu().numpy(), img.astype(np.float32)) and np.array_equal(b.cpu().numpy(), other.astype(np.float32))
    d5 = [[0.9, 0.1, 0.9, 0.1], -0.02, 1.0, 0.85]
    a, b = preprocessing.augment(ti, to, Fixed(d5))
    hl, hr = data_reader.augment(img.astype(np.float32), other.astype(np.float32), Fixed(d5))
    assert np.array_equal(a.cpu().numpy(), hl) and np.array_equal(b.cpu().numpy(), hr)
    # a batch takes one set of parameters; the draws are the host path's (same generator state, same parameters)
    bl, br = preprocessing.augment(torch.stack([ti, to]), torch.stack([to, ti]), Fixed(d5))
    assert tuple(bl.shape) == (2, 15, 22, 3) and np.array_equal(bl[0].cpu().numpy(), hl) and np.array_equal(br[0].cpu().numpy(), hr) and torch.equal(bl[1], br[0])
    seeded = preprocessing.augment(ti, to, np.random.default_rng(1))[0].cpu().numpy()
    host = data_reader.augment(img.astype(np.float32), other.astype(np.float32), np.random.default_rng(1))[0]
    g = np.random.default_rng(1)
    act = g.uniform(0.0, 1.0, size=4)
    y = augment64(img, sum(1 << k for k in range(3) if act[k + 1] <= 0.5), g.uniform(-0.05, 0.05), g.uniform(0.8, 1.2), g.uniform(0.8, 1.2))
    assert np.abs(seeded.astype(np.float64) - y).max() <= 2.0 * np.abs(host.astype(np.float64) - y).max()
    with pytest.raises(ValueError):
        preprocessing.augment(ti.float() + 0.5, to, Fixed(d5))
