"""Proxy labels for the continual loop from the frames themselves: census + four- or eight-path semi-global matching on the device (mh_sgm_proxy_scaled), where the reference
reads a fourth list column of disparity maps an external matcher wrote (README.MD:59-61).  Runs outside the captured step, like mh_frame_prepare: through
Data_utils.data_reader.device_prefetcher(proxy_matcher=...) on the upload stream, a frame ahead of the step that consumes it."""
import torch

from . import ops


class ProxyMatcher(object):
    """Owns the matcher's workspace for one frame size.  compute(left, right) -> float32 [B,H,W] device tensor, 0 = no label; contiguous and 16-byte aligned, so
    Adapter.step takes it through the step's input table without a copy.  paths = 8 adds the four diagonal aggregation paths (fewer gross errors on frames of
    the workload's size, worse on frames a few dozen rows high: DESIGN.md), median = True a 3x3 median of the valid labels.  speckle_size > 0 ends with the
    speckle filter (mh_sgm_speckle): labels whose 4-connected component (neighbours within speckle_range) holds no more than speckle_size pixels become 0.
    scale = 2 matches the half-size gray frames over max_disp / 2 disparities and writes every label, doubled, to its 2 x 2 pixels (mh_sgm_proxy_scaled): an eighth
    of the volume, about twice the mean label error, clearly worse on frames a few dozen rows high.  max_disp stays the full-resolution range (128, 256
    or 384 at scale 2), p1 / p2 / uniq / lr_tol apply to the half frame unchanged.  The speckle filter still runs on the full-resolution map with the same
    speckle_size, and at scale 2 with max_diff = 2 * speckle_range: neighbouring upsampled labels differ by twice the half-resolution difference, so the range
    keeps its meaning as a slope tolerance and the size keeps counting full-resolution pixels."""

    def __init__(self, lib, B, H, W, max_disp=128, device='cuda', p1=10, p2=120, uniq=95, lr_tol=1, paths=4, median=False, speckle_size=0, speckle_range=1.0,
                 scale=1):
        self.lib, self.shape, self.max_disp = lib, (int(B), int(H), int(W)), int(max_disp)
        self.params = dict(p1=int(p1), p2=int(p2), uniq=int(uniq), lr_tol=int(lr_tol), paths=int(paths), median=bool(median))
        self.device = torch.device(device)
        self.scale = int(scale)
        assert self.scale in (1, 2), "ProxyMatcher: scale must be 1 or 2"
        assert self.scale == 1 or self.max_disp in (128, 256, 384), "ProxyMatcher: at scale 2 max_disp must be 128, 256 or 384"
        self.ws = ops.sgm_proxy_ws(lib, B, H, W, self.max_disp, self.device, paths=paths, median=median, scale=self.scale)
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
        ops.sgm_proxy(self.lib, left, right, self.ws, out, self.max_disp, stream=stream, scale=self.scale, **self.params)
        if self.speckle_size > 0:                                       # in place, behind the median and the upsampling
            ops.sgm_speckle(self.lib, out, out, self.speckle_ws, self.speckle_size, self.scale * self.speckle_range, stream=stream)
        return out
