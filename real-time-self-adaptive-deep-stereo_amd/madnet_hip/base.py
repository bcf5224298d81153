"""What MadNetEngine and DispNetEngine share apart from their networks: device set-up, padded geometry, the flat parameter buffers, the registry of
bf16 images, the deterministic twins, the Adam state."""
import ctypes as C

import torch

from . import ops
from .images import Bf16Images
from .params import Params


class EngineBase(object):
    def _init_base(self, lib, H, W, B, device, manifest, weights, precision, schedule):
        if precision not in ops.PRECISION_CODES:
            raise ValueError("precision must be one of %s" % sorted(ops.PRECISION_CODES))
        self.sched, self.precision, self.lib, self.dev = schedule, precision, lib, device
        _td = torch.device(device)
        if _td.type == "cuda" and hasattr(lib, "ensure_init"):
            with torch.cuda.device(_td):                  # the per-device set-up of the library, with THIS engine's device current (a process may drive several)
                lib.ensure_init(torch.cuda.current_device())
        ops.check_planes_rule(lib)
        self.B, self.H0, self.W0 = B, H, W
        self.Hp = H if H % 64 == 0 else (H // 64 + 1) * 64          # preprocessing.pad_image(., 64)
        self.Wp = W if W % 64 == 0 else (W // 64 + 1) * 64
        self.pt, self.pl = (self.Hp - H) // 2, (self.Wp - W) // 2
        self.params = Params(manifest, device)
        if weights is not None:
            self.params.load(weights)
        self.wsa = ops.WgradWorkspace(device)
        self.images = Bf16Images(device)
        # deterministic test mode (Schedule.DETERMINISTIC): float atomics accumulate into 64-bit fixed-point twins the plan flushes in front of their readers
        self.deterministic = schedule.DETERMINISTIC
        self.kitti_metrics = False                         # record mh_metrics_kitti next to mh_metrics (Adapter(kitti_metrics=True))
        self.res_kitti = self.params.res_kitti
        self._det_bases = []

    def _det_twins(self, *bases):
        """deterministic mode: one registered fixed-point twin per base tensor (the library's table holds 8 ranges per process)"""
        twins = [torch.zeros(b.numel(), dtype=torch.int64, device=self.dev) for b in bases]
        for base, twin in zip(bases, twins):
            self.lib.deterministic_add(C.c_void_p(base.data_ptr()), base.numel(), C.c_void_p(twin.data_ptr()))
            self._det_bases.append(base.data_ptr())
        return twins

    def close(self):
        """deterministic mode: un-register this engine's ranges"""
        for b in self._det_bases:
            self.lib.deterministic_remove(C.c_void_p(b))
        self._det_bases = []

    def __del__(self):
        try:
            # (never from inside a stream capture: un-registering synchronises the device, which would invalidate the capture -- call close() explicitly)
            if self._det_bases and not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
                self.close()
        except Exception:
            pass

    def all_vars(self):
        return [n for n, _ in self.params.manifest]

    def set_inputs(self, left, right, gt=None, proxy=None):
        for name, src in (("left", left), ("right", right), ("gt", gt), ("proxy", proxy)):
            if src is not None:
                dst = getattr(self, name)
                dst.copy_(torch.as_tensor(src, dtype=torch.float32).reshape(dst.shape))

    # validity masks of the reprojection losses (rectified frames: Rectifier.valid_masks) ----------------------------------------------------
    valid = None                    # (valid_l, valid_r) once set_valid_masks was called: every LOSS record carries MH_LOSS_MASKED
    _loss_recorded = False          # a reprojection loss was recorded (without masks, if valid is None)
    LOSS_WORKSPACES = ("loss_ws", "loss_ws_k")      # the full-resolution loss's and the MAD blocks'

    def _loss_valid(self):
        """`valid` of the reprojection loss being recorded"""
        self._loss_recorded = True
        return self.valid

    def set_valid_masks(self, valid_l, valid_r):
        """which pixels of the frames exist: uint8 [B,H,W] (or [H,W] for B = 1), non-zero = valid.  The reprojection losses recorded from now on run over the valid
        pixels only (mh_reprojection_loss_masked); the masks are copied, on the CURRENT stream, into every loss workspace of this engine.  The first call must
        come before the first plan is built (a recorded LOSS op either carries the flag or does not); later calls only rewrite the bytes -- also between two
        replays of a captured plan."""
        if getattr(self, "loss_kind", "reprojection") != "reprojection":
            raise ValueError("validity masks need loss_kind 'reprojection' (the label losses have their own valid set)")
        if getattr(self, "rscale", 1) != 1:
            raise NotImplementedError("validity masks with a reprojection scale != 1: the blocks' losses run on resized frames")
        if self.valid is None and self._loss_recorded:
            raise RuntimeError("set_valid_masks: the first call must come before the first plan is built")
        shape = (self.B, self.H0, self.W0)
        masks = []
        for m in (valid_l, valid_r):
            m = torch.as_tensor(m)
            if m.dtype != torch.uint8 or m.numel() != self.B * self.H0 * self.W0:
                raise ValueError("validity masks: uint8 tensors of shape %s" % (shape,))
            masks.append(m.to(self.dev).reshape(shape).contiguous())
        if self.valid is None:
            self.valid = tuple(torch.empty(shape, dtype=torch.uint8, device=self.dev) for _ in masks)
        for dst, m in zip(self.valid, masks):
            dst.copy_(m)
        for name in self.LOSS_WORKSPACES:
            if getattr(self, name, None) is not None:
                ops.loss_set_valid(self.lib, getattr(self, name), *self.valid)

    def record_metrics(self, r):
        """EPE / bad3 of the step's disparity (Stereo_Online_Adaptation.py:74-82) and, with kitti_metrics, the continual loop's report -- EPE over gt > 0 and
        KITTI D1-all (Stereo_Continual_Adaptation.py:245-249) -- on the same lane, into params.res_kitti"""
        ops.metrics(r, self.pred, self.gt, self.met_ws, self.res_met, 3.0)
        if self.kitti_metrics:
            if getattr(self, "kitti_ws", None) is None:
                self.kitti_ws = torch.zeros(self.lib.metrics_kitti_ws_floats(self.B, self.H0, self.W0), device=self.dev)
            ops.metrics_kitti(r, self.pred, self.gt, self.kitti_ws, self.res_kitti)

    def _ensure_adam(self):
        """second Adam moment + the beta powers, on first use; True: created by this call (the caller adds its own training buffers)"""
        if getattr(self, "adam_state", None) is not None:
            return False
        self.params.v = torch.zeros(self.params.total, device=self.dev)
        self.adam_state = torch.tensor([0.9, 0.999], device=self.dev)
        return True

    def record_adam_all(self, r, lr, grad_scale):
        """Adam over the whole parameter buffer as one launch + the advance of the beta powers"""
        P = self.params
        ops.adam(r, P.w, P.m, P.v, P.g, self.adam_state, lr, grad_scale=grad_scale, n=P.total)
        ops.adam_advance(r, self.adam_state)
