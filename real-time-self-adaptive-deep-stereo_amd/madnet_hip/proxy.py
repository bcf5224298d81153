"""Proxy labels for the continual loop from the frames themselves: census + four- or eight-path semi-global matching on the device (mh_sgm_proxy_ex), where the reference
reads a fourth list column of disparity maps an external matcher wrote (README.MD:59-61).  Runs outside the captured step, like mh_frame_prepare: through
Data_utils.data_reader.device_prefetcher(proxy_matcher=...) on the upload stream, a frame ahead of the step that consumes it."""
import torch

from . import ops


class ProxyMatcher(object):
    """Owns the matcher's workspace for one frame size.  compute(left, right) -> float32 [B,H,W] device tensor, 0 = no label; contiguous and 16-byte aligned, so
    Adapter.step takes it through the step's input table without a copy.  paths = 8 adds the four diagonal aggregation paths (fewer gross errors on frames of
    the workload's size, worse on frames a few dozen rows high: DESIGN.md), median = True a 3x3 median of the valid labels.  speckle_size > 0 ends with the
    speckle filter (mh_sgm_speckle): labels whose 4-connected component (neighbours within speckle_range) holds no more than speckle_size pixels become 0."""

    def __init__(self, lib, B, H, W, max_disp=128, device='cuda', p1=10, p2=120, uniq=95, lr_tol=1, paths=4, median=False, speckle_size=0, speckle_range=1.0):
        self.lib, self.shape, self.max_disp = lib, (int(B), int(H), int(W)), int(max_disp)
        self.params = dict(p1=int(p1), p2=int(p2), uniq=int(uniq), lr_tol=int(lr_tol), paths=int(paths), median=bool(median))
        self.device = torch.device(device)
        self.ws = ops.sgm_proxy_ws(lib, B, H, W, self.max_disp, self.device, paths=paths, median=median)
        self.speckle_size, self.speckle_range = int(speckle_size), float(speckle_range)
        assert self.speckle_size >= 0, "ProxyMatcher: speckle_size must not be negative"
        self.speckle_ws = ops.sgm_speckle_ws(lib, B, H, W, self.device) if self.speckle_size > 0 else None      # the filter's own; self.ws stays the matcher's

    def new_output(self):
        return torch.empty(self.shape, dtype=torch.float32, device=self.device)

    def compute(self, left, right, out=None, stream=None):
        """left, right: [B,H,W,3] device tensors, uint8 or float32 holding 0..255.  stream: a raw stream handle (default: the null stream); the workspace is
        used on whichever stream the call names, so calls on different streams must not overlap."""
        assert tuple(left.shape) == self.shape + (3,), "ProxyMatcher: built for %s, got %s" % (self.shape, tuple(left.shape))
        if out is None:
            out = self.new_output()
        ops.sgm_proxy(self.lib, left, right, self.ws, out, self.max_disp, stream=stream, **self.params)
        if self.speckle_size > 0:
            ops.sgm_speckle(self.lib, out, out, self.speckle_ws, self.speckle_size, self.speckle_range, stream=stream)      # in place, behind the median
        return out
