"""device_prefetcher(..., proxy_matcher=m): every slot's proxy map is computed on the prefetcher's upload stream behind that frame's upload and in front of the
slot's ready event.  Every yielded proxy equals m.compute of the same frame run afterwards on the default stream, bit for bit -- over a 3-frame data set with
prefetch depth 2, and over the same frames repeated until every ring slot (depth + 1 of them) has been handed out more than once."""
import numpy as np
import pytest
import torch

from Data_utils import data_reader
from madnet_hip import synthetic as S
from madnet_hip.proxy import ProxyMatcher

H, W, D = 24, 72, 64


def _frames(dtype):
    return [tuple(a.astype(dtype) for a in S.make_pair(H, W, stream_id=t)[:2]) + (S.make_pair(H, W, stream_id=t)[2],) for t in range(3)]


@pytest.mark.parametrize("repeat,dtype,cast", [(1, np.uint8, True), (3, np.float32, True), (3, np.uint8, False)], ids=["3frames", "9frames-float32", "9frames-uint8"])
def test_prefetched_proxy_is_the_matchers(backend, repeat, dtype, cast):
    lib, dev = backend.lib, backend.device
    base = _frames(dtype)
    data = [base[i % 3] + (np.float32(W),) for i in range(3 * repeat)]
    m = ProxyMatcher(lib, 1, H, W, max_disp=D, device=dev)
    got = []
    pf = data_reader.device_prefetcher(data, dev, depth=2, lib=lib, cast=cast, proxy_matcher=m)
    for item in pf:
        assert len(item) == 5
        left, right, gt, proxy, rw = item
        assert proxy.shape == (1, H, W) and proxy.dtype == torch.float32 and proxy.is_contiguous() and proxy.data_ptr() % 16 == 0
        assert left.dtype == (torch.uint8 if (dtype == np.uint8 and not cast) else torch.float32)
        got.append((left.clone(), right.clone(), proxy.clone(), rw.clone()))        # on the current stream, no synchronisation: the slot's event is the only order
    pf.close()
    assert len(got) == len(data)
    other = ProxyMatcher(lib, 1, H, W, max_disp=D, device=dev)                          # afterwards, on the default stream, a workspace of its own
    for i, (left, right, proxy, rw) in enumerate(got):
        assert float(rw) == W and np.array_equal(left.cpu().numpy(), data[i][0].astype(left.cpu().numpy().dtype))
        ref = other.compute(left, right)
        backend.sync()
        assert int((ref > 0).sum()) > 0
        assert torch.equal(ref.view(torch.int32), proxy.view(torch.int32)), "frame %d" % i


def test_matcher_refuses_other_shapes(backend):
    m = ProxyMatcher(backend.lib, 1, H, W, max_disp=D, device=backend.device)
    l = torch.zeros(1, H, W + 1, 3, dtype=torch.uint8, device=backend.device)
    with pytest.raises(AssertionError, match="ProxyMatcher"):
        m.compute(l, l)
    l, r, g = S.make_pair(H, W + 8)
    pf = data_reader.device_prefetcher([(l, r, g)], backend.device, depth=2, lib=backend.lib, proxy_matcher=m)
    with pytest.raises(ValueError, match="proxy_matcher"):
        list(pf)


def test_list_reader_without_proxy_column(tmp_path):
    """continual_data_reader.dataset(proxies=False): rows of three columns, a fourth is not read; proxies=True still insists on four"""
    from PIL import Image
    from Data_utils import continual_data_reader
    l, r, g = S.make_pair(H, W)
    names = [str(tmp_path / n) for n in ("l.png", "r.png", "d.png")]
    Image.fromarray(l[0].astype(np.uint8)).save(names[0]); Image.fromarray(r[0].astype(np.uint8)).save(names[1])
    Image.fromarray((g[0, :, :, 0] * 256).astype(np.uint16)).save(names[2])
    lst = tmp_path / "list.csv"
    lst.write_text(",".join(names) + "\n" + ",".join(names + [str(tmp_path / "no_such_proxy.png")]) + "\n")
    kw = dict(batch_size=1, crop_shape=[H, W], num_epochs=1, augment=False, is_training=False, shuffle=False)
    rows = list(continual_data_reader.dataset(str(lst), proxies=False, **kw))
    assert len(rows) == 2
    for left, right, gt, rw in rows:
        assert left.shape == (1, H, W, 3) and gt.shape == (1, H, W, 1) and rw == W and np.array_equal(left, l) and np.array_equal(right, r)
    with pytest.raises(Exception, match="left,right,gt,proxy"):
        continual_data_reader.dataset(str(lst), proxies=True, **kw)
