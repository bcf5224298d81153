"""DispNet-C executor for MI355X (Nets/DispNet.py:45-152), modes NONE / FULL.

Same machinery as engine.MadNetEngine (static HBM buffers, recorded plans, flat parameter / momentum /
gradient buffers) but the graph is described once as a list of ops over *nodes* (= channel slices of
storages) and the backward plan is derived mechanically from it:

  * every tf.concat of the reference (DispNet.py:55,91) is a storage whose slices are written directly by
    the producing kernels ([skip | deconv | up_predict], [corr | conv_redir]) -- no copy kernels;
  * gradient storages mirror the forward ones; a node's gradient accumulates the contributions of its
    consumers in reverse order; the leaky-ReLU gradient of a node is fused into the epilogue of its LAST
    contributor (channel-range mask for concat gradients) or applied by a small kernel when that
    contributor is not a convolution (correlation gradient).

MAD is not offered for DispNet: the shipped block_config/dispnet_full.json has 5 groups for 6
predictions, so the reference's own assert fails (Stereo_Online_Adaptation.py:97).
"""
import ctypes as C
import os

import torch

from . import ops
from .base import EngineBase
from .netdef import _merge_ranges
from .plan import Recorder
from .schedule import DispNetSchedule

MAX_DISP = 40
ALPHA = 0.1     # default leaky slope of sharedLayers.conv2d / conv2d_transpose (sharedLayers.py:54,80)

# (the scheduling switches live in madnet_hip/schedule.py: an immutable DispNetSchedule per engine, self.sched)


def _r8(c):
    return (c + 7) // 8 * 8

UP_BLOCKS = (("up5", 1024, 512, 512), ("up4", 512, 256, 512), ("up3", 256, 128, 256),
             ("up2", 128, 64, 128), ("up1", 64, 32, 64))       # name, Cin(bottom), Cout, Cskip


def dispnet_manifest():
    """Ordered [(TF variable name, shape)] (bias name is 'bias')."""
    out = []

    def conv(name, k, ci, co):
        out.append(("model/%s/weights" % name, (k, k, ci, co)))
        out.append(("model/%s/bias" % name, (co,)))

    def deconv(name, co, ci):
        out.append(("model/%s/weights" % name, (4, 4, co, ci)))
        out.append(("model/%s/bias" % name, (co,)))

    conv("conv1", 7, 3, 64); conv("conv2", 5, 64, 128); conv("conv_redir", 1, 128, 64)
    conv("conv3", 5, 2 * MAX_DISP + 1 + 64, 256); conv("conv3/1", 3, 256, 256)
    conv("conv4", 3, 256, 512); conv("conv4/1", 3, 512, 512)
    conv("conv5", 3, 512, 512); conv("conv5/1", 3, 512, 512)
    conv("conv6", 3, 512, 1024); conv("conv6/1", 3, 1024, 1024)
    for name, cin, cout, skip in UP_BLOCKS:
        deconv(name + "/deconv", cout, cin)
        conv(name + "/predict", 3, cin, 1)
        deconv(name + "/up_predict", 1, 1)
        conv(name + "/concat", 3, cout + skip + 1, cout)
    conv("prediction", 3, 32, 1)
    return out


class Storage(object):
    def __init__(self, B, H, W, ld, device, grad=True):
        self.B, self.H, self.W, self.ld = B, H, W, ld
        self.t = torch.zeros(B, H, W, ld, device=device)
        self.g = torch.zeros(B, H, W, ld, device=device) if grad else None


class Node(object):
    """Channels [c0, c0+C) of a storage.  alpha = leaky slope of the op that produced it (None: linear /
    not an activation).  members: sub-nodes when this node is a whole concat."""

    def __init__(self, st, c0, C, alpha=None, members=None, name=""):
        self.st, self.c0, self.C, self.alpha, self.members, self.name = st, c0, C, alpha, members, name
        self.consumers = 0
        self.remaining = 0
        self.written = False

    def view(self):
        s = self.st
        return ops.View(s.t, s.B, s.H, s.W, self.C, s.ld, coff=self.c0)

    def gview(self):
        s = self.st
        return ops.View(s.g, s.B, s.H, s.W, self.C, s.ld, coff=self.c0)

    def leaves(self):
        return self.members if self.members else [self]


class DispNetEngine(EngineBase):
    def __init__(self, lib, H, W, B=1, device="cuda", weights=None, precision="fp32", schedule=None):
        """schedule: a madnet_hip.schedule.DispNetSchedule (immutable): how this engine's plans are recorded"""
        self._init_base(lib, H, W, B, device, dispnet_manifest(), weights, precision, schedule if schedule is not None else DispNetSchedule())
        z = lambda *s: torch.zeros(*s, device=device)
        self.left = z(B, H, W, 3); self.right = z(B, H, W, 3); self.gt = z(B, H, W)
        self.pred = z(B, H, W); self.dpred = z(B, H, W)
        # continual-adaptation variant (loss_kind = 'proxy'): proxy labels + the mean_l1 loss workspace
        self.proxy = z(B, H, W); self.proxy_ws = z(lib.proxy_ws_floats(B, H, W))
        self.loss_kind = "reprojection"
        self.proxy_loss = "mean_l1"       # loss_kind 'proxy': which of _ffi.LABEL_LOSS goes on the labels (Adapter(proxy_loss=))
        self.smoothness = 0.0             # loss_kind 'reprojection': weight of the edge-aware smoothness term in the LOSS record (Adapter(smoothness=)); 0 = none
        self.loss_ws = z(lib.loss_ws_floats(B, H, W)); self.met_ws = z(lib.metrics_ws_floats(B, H, W))
        self.res_loss = self.params.g_loss[self.params.total:self.params.total + 4]; self.res_met = z(4)   # (loss result behind the gradients: one collective carries both)
        self.ops = []
        self.nodes = {}
        # bf16 backward: the filter gradients of the 3x3 layers (conv3/1 .. conv6/1, conv4 / 5 / 6 at stride 2, the up-sampling blocks' 3x3 convs and
        # predictions) run on the streaming kernel (mh_wgrad_stream) from bf16 shadows cast per batch; MH_WGRAD_STREAM=0 keeps the tiled kernels
        self.use_stream = precision in ("mixed", "bf16") and os.environ.get("MH_WGRAD_STREAM", "1") != "0"
        self.banks_f, self.banks_b = {}, {}  # weight name -> fragment bank in the 32x32x16 image (forward: trans 2; input gradient: trans 3)
        self.use_planes = self.sched.USE_PLANES and precision in ("mixed", "bf16") and str(device).startswith(("cuda", "cpu"))
        # deterministic test mode: the bias-gradient atomics accumulate into a fixed-point twin of the flat gradient buffer
        if self.deterministic:
            self.det_g, = self._det_twins(self.params.g)
        self._build()

    # ---- graph construction -----------------------------------------------------------------------
    def _st(self, H, W, ld, grad=True):
        return Storage(self.B, H, W, ld, self.dev, grad)

    def _node(self, name, st, c0, C, alpha=None, members=None):
        n = Node(st, c0, C, alpha, members, name)
        self.nodes[name] = n
        return n

    def _use(self, node):
        for m in node.leaves():
            m.consumers += 1

    def _conv(self, x, wname, out, stride=1, alpha=ALPHA, x_grad=True):
        self._use(x)
        self.ops.append(("conv", x, wname, out, stride, alpha, x_grad))

    def _deconv(self, x, wname, out, alpha):
        self._use(x)
        self.ops.append(("deconv", x, wname, out, alpha))

    def _build(self):
        B, Hp, Wp = self.B, self.Hp, self.Wp
        h2, w2, h4, w4, h8, w8 = Hp // 2, Wp // 2, Hp // 4, Wp // 4, Hp // 8, Wp // 8
        h16, w16, h32, w32, h64, w64 = Hp // 16, Wp // 16, Hp // 32, Wp // 32, Hp // 64, Wp // 64
        self.X0L = self._st(Hp, Wp, 4, grad=False); self.X0R = self._st(Hp, Wp, 4, grad=False)
        xl = self._node("inL", self.X0L, 0, 3); xr = self._node("inR", self.X0R, 0, 3)
        # concat storages [skip | deconv | up_predict] of the five up-sampling blocks
        cat = {}
        dims = {"up5": (h32, w32), "up4": (h16, w16), "up3": (h8, w8), "up2": (h4, w4), "up1": (h2, w2)}
        for name, cin, cout, skip in UP_BLOCKS:
            h, w = dims[name]
            cat[name] = self._st(h, w, _r8(skip + cout + 1))            # rows of 8 k floats: mh_conv2d_planes_bwd stores 8 columns per lane
        N = self._node
        c1a = N("conv1a", cat["up1"], 0, 64, ALPHA); c1b = N("conv1b", self._st(h2, w2, 64), 0, 64, ALPHA)
        c2a = N("conv2a", cat["up2"], 0, 128, ALPHA); c2b = N("conv2b", self._st(h4, w4, 128), 0, 128, ALPHA)
        x3 = self._st(h4, w4, _r8(2 * MAX_DISP + 1 + 64))            # (rows of 8 k floats: conv3's input gradient runs the parity-class plane kernel, 8 columns per lane -- round 6)
        corr = N("corr", x3, 0, 2 * MAX_DISP + 1); redir = N("conv_redir", x3, 2 * MAX_DISP + 1, 64, ALPHA)
        x3n = N("corr|redir", x3, 0, 2 * MAX_DISP + 1 + 64, members=[corr, redir])
        c3 = N("conv3", self._st(h8, w8, 256), 0, 256, ALPHA); c31 = N("conv3/1", cat["up3"], 0, 256, ALPHA)
        c4 = N("conv4", self._st(h16, w16, 512), 0, 512, ALPHA); c41 = N("conv4/1", cat["up4"], 0, 512, ALPHA)
        c5 = N("conv5", self._st(h32, w32, 512), 0, 512, ALPHA); c51 = N("conv5/1", cat["up5"], 0, 512, ALPHA)
        c6 = N("conv6", self._st(h64, w64, 1024), 0, 1024, ALPHA); c61 = N("conv6/1", self._st(h64, w64, 1024), 0, 1024, ALPHA)
        self._conv(xl, "conv1", c1a, 2, x_grad=False); self._conv(xr, "conv1", c1b, 2, x_grad=False)
        self._conv(c1a, "conv2", c2a, 2); self._conv(c1b, "conv2", c2b, 2)
        self._conv(c2a, "conv_redir", redir)
        self._use(c2a); self._use(c2b)
        self.ops.append(("corr", c2a, c2b, corr, x3n))
        self._conv(x3n, "conv3", c3, 2); self._conv(c3, "conv3/1", c31)
        self._conv(c31, "conv4", c4, 2); self._conv(c4, "conv4/1", c41)
        self._conv(c41, "conv5", c5, 2); self._conv(c5, "conv5/1", c51)
        self._conv(c51, "conv6", c6, 2); self._conv(c6, "conv6/1", c61)
        bottom = c61
        skips = {"up5": c51, "up4": c41, "up3": c31, "up2": c2a, "up1": c1a}
        self.predict = {}
        for name, cin, cout, skip in UP_BLOCKS:
            st = cat[name]
            h, w = dims[name]
            dec = N(name + "/deconv", st, skip, cout, ALPHA)
            pr = N(name + "/predict", self._st(h // 2, w // 2, 1), 0, 1)
            upp = N(name + "/up_predict", st, skip + cout, 1)
            catn = N(name + "/cat", st, 0, skip + cout + 1, members=[skips[name], dec, upp])
            outn = N(name + "/concat", self._st(h, w, cout), 0, cout)
            self._deconv(bottom, name + "/deconv", dec, ALPHA)
            self._conv(bottom, name + "/predict", pr, 1, alpha=1.0)
            self._deconv(pr, name + "/up_predict", upp, 1.0)
            self._conv(catn, name + "/concat", outn, 1, alpha=1.0)
            self.predict[name] = pr
            bottom = outn
        self.prediction = N("prediction", self._st(h2, w2, 1), 0, 1)
        self._conv(bottom, "prediction", self.prediction, 1, alpha=1.0)
        self._use(self.prediction)
        self.ops.append(("final", self.prediction))

    def W_(self, n, which="w"):
        return self.params.tensor("model/%s/weights" % n, which)

    def b_(self, n, which="w"):
        return self.params.tensor("model/%s/bias" % n, which)

    # 'mixed': the layers whose bf16 rounding moves the final disparity by <= 1e-4 px each (3.3e-4 px together) run plain bf16 in the forward pass
    # too -- conv_redir, conv3 .. conv6/1 and the three coarsest up-blocks (profiles/r02_precision_map_dispnet.txt: rounding ONE group's operands to
    # bf16, everything else fp32); conv1 (6.9e-3), conv2 (9.7e-4), up2 (1.0e-3), up1 (5.7e-3) and prediction (9.1e-3) keep split-bf16 / exact fp32
    MIXED_BF16_FWD = ("conv_redir", "conv3", "conv4", "conv5", "conv6", "up5", "up4", "up3")
    WGRAD_TARGET_PCT = 150       # scale of the filter-gradient pixel-split targets while a plan is recorded (_build_plan)

    def _fwd_code(self, wn):
        if self.precision != "mixed":
            return None
        head = wn.split("/")[0]
        return 1 if head in self.MIXED_BF16_FWD else None

    # ---- forward --------------------------------------------------------------------------------------
    # ---- bf16-plane path of the stride-1 3x3 layers ---------------------------------------------------------------------------------------------
    def _planes_fwd_kind(self, op):
        """0: not on mh_conv2d_planes; 1: plain bf16 (one plane); 2: split-bf16 (hi + lo)"""
        _, x, wn, out, stride, alpha, _ = op
        w = self.W_(wn)
        # stride 1: the 3x3 layers; stride 2 (round 6, Schedule.PLANES_S2): the 5x5 conv2 of both towers (Nets/DispNet.py:80-84 -- 25 GFLOP that ran in exact fp32)
        shape_ok = (stride == 1 and tuple(w.shape[:2]) == (3, 3)) or (stride == 2 and self.sched.PLANES_S2 and w.shape[0] == w.shape[1] and (w.shape[2] <= 128 or self.sched.PLANES_S2_CONV3))
        if not self.use_planes or not shape_ok or x.st.H * x.st.W < self.sched.PLANES_MIN_PIX or x.c0 != 0 or w.shape[3] % 8:
            return 0
        code = self._fwd_code(wn)
        if code is None:
            code = ops.PRECISION_CODES[self.precision][0]
        if code not in (1, 2):
            return 0
        return code if ops.conv2d_planes_ok(self.lib, x.view(), w, 1, bf16=(code == 1), stride=stride) else 0

    def _planes_bwd_ok(self, op):
        _, x, wn, out, stride, alpha, x_grad = op
        w = self.W_(wn)
        shape_ok = (stride == 1 and tuple(w.shape[:2]) == (3, 3)) or (stride == 2 and self.sched.PLANES_S2 and tuple(w.shape[:2]) == (5, 5))      # (round 6: conv2's parity-class form)
        if not (self.use_planes and x_grad and shape_ok and x.st.H * x.st.W >= self.sched.PLANES_MIN_PIX and x.c0 == 0):
            return False
        return ops._bwd_precision() == 1 and x.st.ld >= _r8(x.C) and ops.conv2d_planes_bwd_ok(self.lib, x.gview(), w, 1, stride=stride)

    def _record_banks(self, r, backward):
        """one mh_pack_weights launch at the head of the step: the banks of every layer on the plane kernels (re-packed every step: the weights move)"""
        todo = []
        packed = set()                        # (the two towers' conv2 share one variable: one bank, packed once)
        for op in self.ops:
            if op[0] != "conv":
                continue
            wn = op[2]
            w = self.W_(wn)
            kind = self._planes_fwd_kind(op)
            if kind:
                if wn not in self.banks_f or self.banks_f[wn][1] != kind:
                    self.banks_f[wn] = (torch.zeros(ops.pack_bytes(w, kind, 2) // 4, device=self.dev), kind)
                if (wn, "f") not in packed:
                    todo.append((w, self.banks_f[wn][0], kind, 2))
                    packed.add((wn, "f"))
            if backward and self._planes_bwd_ok(op):
                if wn not in self.banks_b:
                    self.banks_b[wn] = torch.zeros(ops.pack_bytes(w, 1, 3) // 4, device=self.dev)
                if (wn, "b") not in packed:
                    todo.append((w, self.banks_b[wn], 1, 3))
                    packed.add((wn, "b"))
        ops.pack_weights(r, todo, self.dev, r.keep)

    def record_forward(self, r, backward=True):
        B = self.B
        im = self.images
        im.begin_plan()
        if self.use_planes:
            self._record_banks(r, backward)
        # DispNet._preprocess_inputs (DispNet.py:59-73): x/255 - 100/255, reflect pad to a multiple of 64
        ops.pad_reflect(r, self.left, self.X0L.t, self.pt, self.pl, div=255.0, sub=100.0 / 255)
        ops.pad_reflect(r, self.right, self.X0R.t, self.pt, self.pl, div=255.0, sub=100.0 / 255)
        # (round 6) a conv whose result is -- whole -- the input of a split-bf16 plane layer writes the hi / lo planes in its own epilogue (mh_conv2d_sh4) instead of a
        # plane_split launch in front of the consumer: conv1 -> conv2 of both towers (2 x 12 us at 1242x375)
        plane_consumers = {}
        if self.sched.PLANES_S2:
            for op2 in self.ops:
                if op2[0] == "conv" and self._planes_fwd_kind(op2) == 2:
                    plane_consumers[im.key(op2[1].view())] = True
        # activations whose bf16 shadow a later launch of this plan reads: input of a one-plane forward layer, of a streamed filter gradient (3x3, stride 1), leaky mask of
        # a plane input gradient -- their producer writes the shadow
        shadow_readers = set()
        if self.use_planes and self.sched.PRODUCER_SHADOWS:
            for op2 in self.ops:
                if op2[0] != "conv":
                    continue
                _, x2, wn2, _, stride2, _, x_grad2 = op2
                w2 = self.W_(wn2)
                streamed = backward and self.use_stream and ops._bwd_precision() == 1 and tuple(w2.shape[:2]) == (3, 3) and stride2 == 1
                masked = backward and x_grad2 and x2.alpha is not None and self._planes_bwd_ok(op2)
                if self._planes_fwd_kind(op2) == 1 or streamed or masked:
                    shadow_readers.add(im.key(x2.view()))
        for op in self.ops:
            kind = op[0]
            if kind == "conv":
                _, x, wn, out, stride, alpha, _ = op
                kind = self._planes_fwd_kind(op)
                if kind:
                    # x -> bf16 plane(s) once (the hi plane is the shadow the streamed filter gradient reads: no cast in the backward pass)
                    xv = x.view()
                    if kind == 2:
                        xp = im.planes(xv)
                        if not im.fresh_planes(xv):
                            ops.plane_split(r, [(xv, xp)], self.dev, r.keep)
                    else:
                        casts = []
                        xp = im.queue_cast(xv, casts)
                        ops.shadow_cast(r, casts, self.dev, r.keep)        # (no launch when a producer of this plan wrote the shadow)
                    im.mark(xv)
                    ov = out.view()
                    okey = im.key(ov)
                    outp = None
                    if ov.C % 8 == 0 and okey in plane_consumers:
                        outp = im.planes(ov)
                        im.mark(ov, lo=True)
                    elif ov.C % 8 == 0 and okey in shadow_readers:
                        outp = im.shadow(ov)
                        im.mark(ov)
                    ops.conv2d_planes(r, xp, self.W_(wn), self.banks_f[wn][0], self.b_(wn), out=ov, out_planes=outp, alpha=alpha, bf16=(kind == 1), stride=stride)
                    continue
                ov = out.view()
                okey = im.key(ov)
                osh = opl = None
                if okey in plane_consumers and ov.C % 8 == 0:        # (the fp32 result may be a slice of a concat buffer -- conv1a is a skip connection --: the planes are the view's own)
                    opl = im.planes(ov)
                    im.mark(ov, lo=True)
                elif okey in shadow_readers and ov.C % 8 == 0:
                    osh = im.shadow(ov)
                    im.mark(ov)
                ops.conv2d_fwd(r, x.view(), self.W_(wn), self.b_(wn), ov, stride=stride, alpha=alpha, precision=self._fwd_code(wn), shadow=osh, out_planes=opl)
            elif kind == "deconv":
                _, x, wn, out, alpha = op
                ops.conv2d_transpose_fwd(r, x.view(), self.W_(wn), self.b_(wn), out.view(), stride=2, alpha=alpha, precision=self._fwd_code(wn))
            elif kind == "corr":
                _, L, R, out, whole = op
                # 'mixed': the 81-shift volume on plain bf16 MFMA -- rounding ITS operands to bf16 moves the final disparity by 1.3e-6 px
                # (profiles/r02_precision_map_dispnet.txt), and conv3, which reads it, runs bf16 anyway
                ops.corr_fwd(r, L.view(), R.view(), whole.view(), MAX_DISP, 1, coff=0, precision=self._fwd_code("conv3"))
            elif kind == "final":
                # rescaled_prediction = crop(resize(prediction) * 2)  (DispNet.py:149-151; no relu)
                ops.resize_fwd(r, op[1].st.t.view(B, op[1].st.H, op[1].st.W), self.pred, self.Hp, self.Wp, self.pt, self.pl,
                               mul=2.0, mode=0)

    def record_make_disp(self, r, name, out):
        """DispNet._make_disp (DispNet.py:39-43): crop(resize(relu(op * W_in/W_op)))."""
        n = self.prediction if name == "prediction" else self.predict[name]
        ops.resize_fwd(r, n.st.t.view(self.B, n.st.H, n.st.W), out, self.Hp, self.Wp, self.pt, self.pl,
                       mul=float(self.Wp) / float(n.st.W), mode=1)

    def record_loss_metrics(self, r, with_grad):
        """full-resolution reprojection loss -- or, loss_kind 'proxy', full_proxy_loss of the continual variant (Stereo_Continual_Adaptation.py:75: self.proxy_loss, default mean_l1, against the
        proxy labels, weight 0.01; of the reduced multi-scale sum only the last prediction contributes) -- + EPE / bad3"""
        if self.loss_kind not in ("reprojection", "proxy"):
            raise ValueError("loss_kind must be 'reprojection' or 'proxy'")
        if self.loss_kind == "proxy":
            ops.proxy_loss(r, self.pred, self.proxy, self.proxy_ws, self.res_loss, self.dpred if with_grad else None, weight=0.01, loss=self.proxy_loss)
        else:
            ops.reprojection_loss(r, self.left, self.right, self.pred, self.loss_ws, self.res_loss, self.dpred if with_grad else None, smoothness=self.smoothness, valid=self._loss_valid())
        self.record_metrics(r)

    # ---- backward (derived from the op list) ------------------------------------------------------------
    def _contribute(self, node):
        """Bookkeeping for ONE contribution into `node` (or all members of a concat).  Returns
        (accumulate, masks) where masks = [(leaf, is_last)] for leaves with a leaky gradient."""
        leaves = node.leaves()
        acc = any(m.written for m in leaves)
        if acc and not all(m.written for m in leaves):
            raise RuntimeError("partial concat gradient for %s" % node.name)
        last_masks = []
        for m in leaves:
            m.written = True
            m.remaining -= 1
            if m.remaining == 0 and m.alpha is not None:
                last_masks.append(m)
        return acc, last_masks

    def record_backward(self, r, heads=(), early_update=None):
        """heads (offline training): [(prediction node, d loss / d make_disp(node))] -- every _make_disp output carries its own
        loss term (Train.py:100); each is one more consumer of its node and is injected before the op list is walked.
        early_update = (lr, momentum, grad_scale): see self.sched.EARLY_UPDATE; returns the sorted disjoint [first, end) parameter ranges updated here"""
        lib, B, P, im = r, self.B, self.params, self.images
        upd_fresh, upd_done = [], []
        ops.fill(lib, P.g, 0, P.total)
        for n in self.nodes.values():
            n.remaining, n.written = n.consumers, False
        for n, _ in heads:
            n.remaining += 1
        for n, gbuf in heads:
            acc, _ = self._contribute(n)
            ops.resize_bwd(lib, gbuf, n.st.t.view(B, n.st.H, n.st.W), n.st.g.view(B, n.st.H, n.st.W), self.Hp, self.Wp, self.pt, self.pl,
                           mul=float(self.Wp) / float(n.st.W), mode=1, accumulate=acc)
        # filter gradients: atomic-free partial sums + one reduction launch, deferred in batches onto side lanes
        # (see engine.MadNetEngine.record_backward); a weight shared by two convs (conv1/conv2 of the two towers)
        # puts its second use into a second, accumulating reduction
        segs, segs2, pending, nflush = [], [], [], [0]
        pending_bias = []                     # (dz view, bias gradient) of the transposed convs: column sums without atomics, issued with their layer's batch
        seen_dst = set()
        uses = {}
        for op in self.ops:                   # weights used by two convs (the towers' conv1 / conv2) must not be written directly
            if op[0] in ("conv", "deconv"):
                uses[op[2]] = uses.get(op[2], 0) + 1
        shared_dw = set(self.W_(wn, "g").data_ptr() for wn, c in uses.items() if c > 1)

        def wgrad(xv, dzv, dw, db, stride, db_t=None):
            pending.append((xv, dzv, dw, db, stride))
            if early_update is not None and dw.data_ptr() not in shared_dw:
                for t in (dw, db if db is not None else db_t):
                    if t is None:
                        continue
                    a = (t.data_ptr() - P.g.data_ptr()) // 4
                    assert 0 <= a and a + t.numel() <= P.total
                    upd_fresh.append((a, min((a + t.numel() + 3) & ~3, P.total)))      # (+ the tensor's alignment padding: zero gradient, zero momentum)

        def flush(force=False):
            if not pending or (len(pending) < self.sched.FLUSH_MIN and not force):
                return
            lib.lane = 1 + nflush[0] % self.sched.SIDE_LANES
            nflush[0] += 1
            try:
                batch = []
                todo = list(pending)
                if self.use_stream and ops._bwd_precision() == 1:
                    items, casts, todo = [], [], []
                    for xv, dzv, dw, db, stride in pending:
                        if ops.wgrad_stream_ok(xv, dzv, dw, stride, 1) and dw.data_ptr() not in shared_dw:
                            items.append((im.queue_cast(xv, casts), im.queue_cast(dzv, casts), dw, db, 1))
                        else:
                            todo.append((xv, dzv, dw, db, stride))
                    ops.shadow_cast(lib, casts, self.dev, r.keep)
                    ops.wgrad_stream(lib, self.lib, self.wsa, batch, items, self.dev, r.keep, nwaves=(4 if self.B == 1 else 8))
                for dzv, dbt in pending_bias:
                    ops.bias_grad_partial(lib, self.lib, self.wsa, batch, dzv, dbt)
                del pending_bias[:]
                for xv, dzv, dw, db, stride in todo:
                    dup = dw.data_ptr() in seen_dst
                    seen_dst.add(dw.data_ptr())
                    shared = dw.data_ptr() in shared_dw
                    # un-shared weights: reduced right here on the lane; the two uses of a shared weight wait for the final pair
                    ops.conv2d_wgrad_partial(lib, self.lib, self.wsa, (segs2 if dup else segs) if shared else batch, xv, dzv, dw, db,
                                             stride=stride, direct_ok=not shared)
                ops.wgrad_reduce(lib, batch, self.dev, r.keep)
                if early_update is not None:
                    lr_, mom_, gs_ = early_update
                    for a, b in _merge_ranges(upd_fresh):
                        ops.momentum(lib, P.w[a:b], P.m[a:b], P.g[a:b], lr_, mom_, gs_)
                        upd_done.append((a, b))
            finally:
                lib.lane = 0
                del pending[:]
                del upd_fresh[:]

        # gradient maps whose bf16 shadow a later launch reads as its dz: the plane input gradient / the streamed filter gradient of the layer that produced the node
        grad_readers = set()
        if self.use_planes and self.sched.PRODUCER_SHADOWS and ops._bwd_precision() == 1:
            for op2 in self.ops:
                if op2[0] == "conv":
                    _, x2, wn2, out2, stride2, _, x_grad2 = op2
                    w2 = self.W_(wn2)
                    if (self.use_stream and tuple(w2.shape[:2]) == (3, 3) and stride2 == 1) or self._planes_bwd_ok(op2):
                        grad_readers.add(out2.name)

        def conv_like_dgrad(emit, xnode):
            """emit(dx_view, accumulate, mask_ref, mask_alpha, mask_range, shadow); handles the leaky-mask fusion.  shadow: the Shadow of dx when this contribution
            COMPLETES the gradient map of a plain node whose shadow a later launch reads -- the emitting kernel writes it with its final values"""
            acc, masks = self._contribute(xnode)
            fused = masks[0] if masks else None
            sh = None
            if (not xnode.members and xnode.remaining == 0 and len(masks) <= 1 and xnode.name in grad_readers and xnode.C % 8 == 0
                    and (fused is None or fused is xnode)):
                sh = im.shadow(xnode.gview())
                im.mark(xnode.gview())
            if fused is not None:
                rng = (fused.c0 - xnode.c0, fused.c0 - xnode.c0 + fused.C)
                ref = ops.View(xnode.st.t, B, xnode.st.H, xnode.st.W, xnode.C, xnode.st.ld, coff=xnode.c0)
                emit(xnode.gview(), acc, ref, fused.alpha, rng, sh)
            else:
                emit(xnode.gview(), acc, None, 1.0, (0, 0), sh)
            for m in masks[1:]:
                ops.leaky_bwd(lib, m.gview(), m.view(), m.alpha)

        for op in reversed(self.ops):
            kind = op[0]
            if kind == "final":
                n = op[1]
                g3 = n.st.g.view(B, n.st.H, n.st.W)
                acc, _ = self._contribute(n)
                ops.resize_bwd(lib, self.dpred, n.st.t.view(B, n.st.H, n.st.W), g3, self.Hp, self.Wp, self.pt, self.pl,
                               mul=2.0, mode=0, accumulate=acc)
            elif kind == "conv":
                _, x, wn, out, stride, alpha, x_grad = op
                assert out.written and out.remaining == 0, "gradient of %s incomplete" % out.name
                dz = out.gview()
                wgrad(x.view(), dz, self.W_(wn, "g"), self.b_(wn, "g"), stride)
                if x_grad:
                    w = self.W_(wn)

                    def emit_dgrad(dx, acc, ref, ma, rng, sh, op=op, dz=dz, w=w, wn=wn, stride=stride):
                        if (not acc or stride == 2) and wn in self.banks_b and self._planes_bwd_ok(op):          # (the stride-2 5x5 form accumulates: conv1a is a skip connection)
                            # dz (and the activation whose sign is the mask) as bf16 planes -- the casts the streamed filter gradient of this very
                            # layer would queue on its side lane anyway -- then the one-plane walk over dz (mh_conv2d_planes_bwd)
                            casts = []
                            dzs = im.queue_cast(dz, casts)
                            ms = im.queue_cast(ref, casts) if ref is not None else None
                            for v in (dz, ref):
                                if v is not None:
                                    im.mark(v)
                            ops.shadow_cast(lib, casts, self.dev, r.keep)
                            ops.conv2d_planes_bwd(lib, dzs, w, self.banks_b[wn], dx=dx, dx_shadow=sh, mask_shadow=ms, mask_alpha=ma, mask_range=rng, stride=stride, accumulate=acc)
                            return
                        ops.conv2d_dgrad(lib, dz, w, dx, stride=stride, accumulate=acc, mask_ref=ref, mask_alpha=ma, mask_range=rng, shadow=sh)
                    conv_like_dgrad(emit_dgrad, x)
            elif kind == "deconv":
                _, x, wn, out, alpha = op
                assert out.written and out.remaining == 0, "gradient of %s incomplete" % out.name
                dz = out.gview()
                # y = conv2d_transpose(x, w[kh,kw,Cout,Cin]) is the input-gradient of the SAME conv F with HWIO = w:
                # dw = filter-gradient of F with (input = dz, output-gradient = x); db = sum(dz); dx = F(dz)
                pending_bias.append((dz, self.b_(wn, "g")))         # BiasAddGrad: per-workgroup partial sums + a segment of the batch's reduction (no float atomics)
                wgrad(dz, x.view(), self.W_(wn, "g"), None, 2, db_t=self.b_(wn, "g"))
                w = self.W_(wn)
                conv_like_dgrad(lambda dx, acc, ref, ma, rng, sh: ops.conv2d_fwd(lib, dz, w, None, dx, stride=2, alpha=1.0, accumulate=acc,
                                                                                  mask_ref=ref, mask_alpha=ma, mask_range=rng, shadow=sh), x)
            elif kind == "corr":
                _, L, R, out, whole = op
                assert out.written
                accL, mL = self._contribute(L)
                accR, mR = self._contribute(R)
                ops.corr_bwd(lib, whole.gview(), L.view(), R.view(), L.gview(), R.gview(), MAX_DISP, 1, coff=0,
                             acc_l=accL, acc_r=accR, copy_left=False)
                for m in mL + mR:
                    ops.leaky_bwd(lib, m.gview(), m.view(), m.alpha)
            flush()
        flush(force=True)
        r.join_next = True
        ops.wgrad_reduce(lib, segs, self.dev, r.keep)
        ops.wgrad_reduce(lib, segs2, self.dev, r.keep, accumulate=True)
        if self.deterministic:
            assert not upd_done
            lib.det_flush(C.c_void_p(P.g.data_ptr()), C.c_void_p(self.det_g.data_ptr()), P.total, None)
        return _merge_ranges(upd_done)

    def record_update(self, r, lr, momentum=0.9, grad_scale=1.0, done=()):
        """MomentumOptimizer apply on every parameter; done: sorted disjoint [first, end) ranges record_backward(early_update=...) has updated already"""
        P = self.params
        a = 0
        for d0, d1 in list(done) + [(P.total, P.total)]:
            if d0 > a:
                ops.momentum(r, P.w[a:d0], P.m[a:d0], P.g[a:d0], lr, momentum, grad_scale, n=d0 - a)
            a = max(a, d1)

    # ---- offline training (Train.py) -----------------------------------------------------
    def _ensure_train_buffers(self):
        if self._ensure_adam():
            z = lambda *shape: torch.zeros(*shape, device=self.dev)
            self.head_names = ["prediction"] + [u[0] for u in UP_BLOCKS[::-1]]     # disparities[-2], [-3] (up1) ... [-7] (up5)
            self.disp_ms = {k: z(self.B, self.H0, self.W0) for k in self.head_names}
            self.ddisp_ms = {k: z(self.B, self.H0, self.W0) for k in self.head_names}
            self.res_loss_ms = z(1 + len(self.head_names), 4)                      # rows: rescaled_prediction, then head_names
            self.sup_ws = z(self.lib.proxy_ws_floats(self.B, self.H0, self.W0))

    def _build_train_plan(self, r, lr, grad_scale, update, part, loss_weights, max_disp):
        """Train.py:94-102 for DispNet: loss = sum_i w_i * mean_l1(disparities[-(i+1)], gt, valid) over the 7 predictions
        (rescaled_prediction, _make_disp(prediction), _make_disp(up1/predict) ... _make_disp(up5/predict)), Adam(lr, 0.9)."""
        self._ensure_train_buffers()
        lw = list(loss_weights) if loss_weights is not None else [1.0] * 10
        if part in ("all", "grad"):
            self.record_forward(r)
            ops.supervised_loss(r, self.pred, self.gt, self.sup_ws, self.res_loss_ms[0], self.dpred, weight=lw[0], max_disp=max_disp)
            heads = []
            for i, name in enumerate(self.head_names):
                self.record_make_disp(r, name, self.disp_ms[name])
                ops.supervised_loss(r, self.disp_ms[name], self.gt, self.sup_ws, self.res_loss_ms[i + 1], self.ddisp_ms[name],
                                    weight=lw[i + 1], max_disp=max_disp)
                heads.append((self.prediction if name == "prediction" else self.predict[name], self.ddisp_ms[name]))
            self.record_metrics(r)
            self.record_backward(r, heads=heads)
        if update and part in ("all", "update"):
            self.record_adam_all(r, lr, grad_scale)
        return r.compile()

    def build_plan(self, mode, lr=1e-4, grad_scale=1.0, update=True, part="all", loss_weights=None, max_disp=192.0,
                   optimizer="momentum", momentum=0.9, inputs=None, **_):
        """inputs: an ops.InputTable -- the plan's first op fills left / right / gt / proxy from the device tensors the table names (engine.MadNetEngine.build_plan)"""
        r = Recorder()
        if inputs is not None and part != "update":
            ops.fetch_inputs(r, inputs.ptr, [self.left, self.right, self.gt] + ([self.proxy] if self.loss_kind == "proxy" else []))
        r.wgrad_group_max_m = 0      # per-plan cap of the grouped filter gradients (0 = library default; 4096 and 16384 measure the same here)
        self.wsa.reset()
        # DispNet's filter gradients (few pixels, 256-1024 channels) keep the round-1 pixel-split targets: 3.99 vs 4.08 ms (the split counts are resolved
        # while the plan is recorded and stored in it)
        # (a process-wide hook: recorded under a lock, and what another caller had set is restored -- ADVICE r02)
        with ops.TUNE_LOCK, ops.precision_scope(self.precision):
            prev = self.lib.tune_wgrad_target_pct(self.WGRAD_TARGET_PCT)
            try:
                if mode == "TRAIN":
                    return self._build_train_plan(r, lr, grad_scale, update, part, loss_weights, max_disp)
                return self._build_plan(r, mode, lr, grad_scale, update, part, optimizer, momentum)
            finally:
                self.lib.tune_wgrad_target_pct(prev)

    def _build_plan(self, r, mode, lr, grad_scale, update, part, optimizer="momentum", momentum=0.9):
        if optimizer not in ("momentum", "adam"):
            raise ValueError("optimizer must be 'momentum' or 'adam'")
        do_grad = part in ("all", "grad")
        do_upd = update and part in ("all", "update")
        if mode not in ("NONE", "FULL"):
            raise ValueError("DispNet supports modes NONE and FULL (the reference's MAD assert fails for it)")
        if do_grad:
            self.record_forward(r, backward=(mode == "FULL"))
            self.record_loss_metrics(r, with_grad=(mode == "FULL"))
            done = ()
            if mode == "FULL":
                eu = (lr, momentum, grad_scale) if (self.sched.EARLY_UPDATE and do_upd and part == "all" and optimizer == "momentum" and not self.deterministic) else None
                done = self.record_backward(r, early_update=eu) or ()
        else:
            done = ()
        if mode == "FULL" and do_upd:
            if optimizer == "adam":                       # the live demo's FULL mode (Demo/demo_model.py:148-149,164)
                self._ensure_train_buffers()
                self.record_adam_all(r, lr, grad_scale)
            else:
                self.record_update(r, lr, momentum=momentum, grad_scale=grad_scale, done=done)
        return r.compile()
