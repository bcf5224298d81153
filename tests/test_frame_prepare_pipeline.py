"""Train.py's input pipeline with the preparation on the device: dataset(prepare='device') -> device_prefetcher -> mh_frame_prepare against the host path
(dataset(prepare='host')), on the CPU with the emulator library and, marked gpu, on the product library.  Six small PNG triples with mixed source sizes and
16-bit ground truth.

Same seed => same samples, windows and parameters on both paths: the ground truth is identical, the images are identical without augmentation; with it they obey
the op-level rule of tests/test_frame_prepare.py -- the distance from the float64 restatement of the formula is at most 2x the fp32 host path's, per batch.
Measured (32x48 windows, seed 11, 9 batches; the same figures on the emulator and on the MI355X): host 2.0e-4 .. 4.3e-4, device 2.0e-4 .. 2.8e-4, device / host between 0.52 and 1.0."""
import numpy as np
import pytest

from Data_utils import data_reader
from test_frame_prepare import augment64

SIZES = [(40, 60), (44, 57), (40, 60), (38, 70), (50, 52), (41, 63)]


@pytest.fixture(scope="module")
def triples(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("triples")
    rng = np.random.default_rng(21)
    rows = []
    for t, (h, w) in enumerate(SIZES):
        names = [str(d / ("%s_%d.png" % (k, t))) for k in ("l", "r", "d")]
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(names[0])
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(names[1])
        Image.fromarray(rng.integers(0, 65536, (h, w), dtype=np.uint16)).save(names[2])
        rows.append(",".join(names))
    lst = d / "list.csv"
    lst.write_text("\n".join(rows) + "\n")
    return str(lst)


def _window(a, r0, c0, H, W):
    """numpy statement of the device's window: zeros outside the source"""
    out = np.zeros((H, W) + a.shape[2:], a.dtype)
    y0, y1, x0, x1 = max(r0, 0), min(r0 + H, a.shape[0]), max(c0, 0), min(c0 + W, a.shape[1])
    if y1 > y0 and x1 > x0:
        out[y0 - r0:y1 - r0, x0 - c0:x1 - c0] = a[y0:y1, x0:x1]
    return out


def _through_prefetcher(ds, backend):
    return [tuple(t.cpu().numpy().copy() for t in b) for b in data_reader.device_prefetcher(ds, backend.device, depth=2, lib=backend.lib)]


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_same_seed_host_and_device_paths_agree(backend, triples, augment):
    kw = dict(batch_size=2, crop_shape=(32, 48), num_epochs=3, augment=augment, is_training=True, shuffle=True, seed=11)
    host = list(data_reader.dataset(triples, **kw))
    raw = list(data_reader.dataset(triples, prepare='device', **kw))
    dev = _through_prefetcher(data_reader.dataset(triples, prepare='device', **kw), backend)
    assert len(host) == len(dev) == len(raw) == 9
    for (hl, hr, hg), (dl, dr, dg), rb in zip(host, dev, raw):
        assert dl.dtype == np.float32 and dl.shape == (2, 32, 48, 3) and dg.shape == (2, 32, 48, 1)
        assert rb.left[0].dtype == np.uint8 and rb.gt[0].dtype == np.uint16            # raw frames on the wire, 16-bit ground truth as it is
        assert np.array_equal(hg, dg)
        if not augment:
            assert rb.active == [0, 0] and np.array_equal(hl, dl) and np.array_equal(hr, dr)
            continue
        host_d = dev_d = 0.0
        for b in range(2):
            for raw_img, h_img, d_img in ((rb.left[b], hl[b], dl[b]), (rb.right[b], hr[b], dr[b])):
                y = augment64(_window(raw_img, rb.r0[b], rb.c0[b], 32, 48), rb.active[b], rb.delta[b], rb.contrast[b], rb.hue[b])
                host_d = max(host_d, float(np.abs(h_img.astype(np.float64) - y).max()))
                dev_d = max(dev_d, float(np.abs(d_img.astype(np.float64) - y).max()))
        print("batch (%s): active %s host %.3g device %.3g from the float64 statement" % (backend.name, rb.active, host_d, dev_d))
        assert dev_d <= 2.0 * host_d
    if augment:
        assert any(a for rb in raw for a in rb.active) and any(a & 2 for rb in raw for a in rb.active)      # the stream exercises the branches, contrast included


def test_worker_count_does_not_change_the_batches(triples):
    kw = dict(batch_size=2, crop_shape=(32, 48), num_epochs=3, augment=True, is_training=True, shuffle=True, seed=5)
    one = list(data_reader.dataset(triples, prepare='device', workers=1, **kw))
    four = list(data_reader.dataset(triples, prepare='device', workers=4, **kw))
    assert len(one) == len(four) == 9
    for a, b in zip(one, four):
        for name in ('r0', 'c0', 'active', 'delta', 'contrast', 'hue', 'crop'):
            assert getattr(a, name) == getattr(b, name), name
        for name in ('left', 'right', 'gt'):
            assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(getattr(a, name), getattr(b, name)))
    h1 = list(data_reader.dataset(triples, workers=1, **kw))
    h4 = list(data_reader.dataset(triples, workers=4, **kw))
    assert len(h1) == len(h4) == 9 and all(np.array_equal(x, y) for a, b in zip(h1, h4) for x, y in zip(a, b))


def test_defaults_are_the_host_path_with_one_worker(triples):
    """the new keywords exist and their defaults select today's loop: both calls below take dataset._load, the code of the parent commit, so equality here
    only pins the defaults.  That the drawn-ahead path (_draw + _load_drawn) reproduces _load is what h1 == h4 in the worker test above checks."""
    for kw in (dict(batch_size=2, crop_shape=(32, 48), num_epochs=2, augment=True, is_training=True, shuffle=True, seed=3),
               dict(batch_size=1, crop_shape=(42, 58), num_epochs=1)):
        default = list(data_reader.dataset(triples, **kw))
        explicit = list(data_reader.dataset(triples, prepare='host', workers=1, **kw))
        assert len(default) == len(explicit) > 0
        for a, b in zip(default, explicit):
            assert isinstance(a, tuple) and all(x.dtype == np.float32 and np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        data_reader.dataset(triples, prepare='gpu')


def test_centre_crop_and_pad_through_the_device_path(backend, triples):
    """is_training=False: 42x58 is larger than some sources on one axis, smaller on the other, and both for others -- the window origin states center_crop_or_pad"""
    kw = dict(batch_size=1, crop_shape=(42, 58), num_epochs=1)
    raw = list(data_reader.dataset(triples, prepare='device', **kw))
    dev = _through_prefetcher(data_reader.dataset(triples, prepare='device', workers=2, **kw), backend)
    assert len(raw) == len(dev) == 6
    for rb, (dl, dr, dg), (h, w) in zip(raw, dev, SIZES):
        assert rb.r0[0] == ((h - 42) // 2 if h >= 42 else -((42 - h) // 2)) and rb.c0[0] == ((w - 58) // 2 if w >= 58 else -((58 - w) // 2))
        g = (rb.gt[0].astype(np.float32) / 256.0)[..., None]
        for got, src in ((dl, rb.left[0].astype(np.float32)), (dr, rb.right[0].astype(np.float32)), (dg, g)):
            assert np.array_equal(got[0], data_reader.center_crop_or_pad(src, 42, 58))
    host = list(data_reader.dataset(triples, **kw))
    assert all(np.array_equal(x, y) for a, b in zip(host, dev) for x, y in zip(a, b))
