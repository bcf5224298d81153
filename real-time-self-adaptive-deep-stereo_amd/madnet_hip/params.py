"""The flat parameter buffers both engines train: weights, momentum, gradients (+ the loss result behind them) in ONE layout."""
import numpy as np
import torch


class Params(object):
    """Flat fp32 weight / momentum / gradient buffers + name -> (offset, shape) manifest."""

    def __init__(self, manifest, device):
        self.manifest = manifest
        self.offset, self.shape = {}, {}
        off = 0
        for name, shp in manifest:
            self.offset[name], self.shape[name] = off, tuple(shp)
            off += (int(np.prod(shp)) + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.total = off
        self.w = torch.zeros(off, device=device)
        self.m = torch.zeros(off, device=device)
        # + 4 floats behind the gradients: the step's loss result lives there, so the shared-model mode all-reduces the
        # gradients AND the loss that drives the reward / reset logic with ONE collective (adapter.py)
        # + 4 more behind the loss: the KITTI report of the continual loop (mh_metrics_kitti), so that loss and report reach the host in one transfer
        store = torch.zeros(off + 8, device=device)
        self.g_loss = store[:off + 4]                          # [gradients | loss result (4 floats)]
        self.g = self.g_loss[:off]
        self.res_kitti = store[off + 4:off + 8]                # [EPE over gt > 0, D1-all, #valid, -]
        self.loss_kitti = store[off:off + 8]                   # loss result + report, contiguous
        self.w0 = None                                         # reset copy (restore target)

    def numel(self, name):
        return int(np.prod(self.shape[name]))

    def tensor(self, name, which="w"):
        buf = getattr(self, which)
        o = self.offset[name]
        return buf[o:o + self.numel(name)].view(self.shape[name])

    def load(self, weights):
        """weights: {name: ndarray / tensor} (HWIO); missing names keep their value."""
        for name, v in weights.items():
            if name in self.offset:
                self.tensor(name).copy_(torch.as_tensor(v, dtype=torch.float32).reshape(self.shape[name]))

    def export(self):
        return {name: self.tensor(name).detach().cpu().numpy().copy() for name, _ in self.manifest}

    def ranges(self, names):
        """Coalesced (offset, count) ranges covering the given variables."""
        spans = sorted((self.offset[n], (self.numel(n) + 3) // 4 * 4) for n in set(names))
        out = []
        for o, c in spans:
            if out and out[-1][0] + out[-1][1] == o:
                out[-1][1] += c
            else:
                out.append([o, c])
        return [(o, c) for o, c in out]
