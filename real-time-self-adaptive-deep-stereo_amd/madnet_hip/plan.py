"""Plan recording / replay: the host compiles a network ONCE into an array of mh_op records
(include/madnet_hip.h); libmadnet_hip.so's native executor replays it with one FFI call, or
captures it into a hipGraph.  This replaces TF1's graph + Session.run machinery for the path
(Stereo_Online_Adaptation.py:208) -- there is no tracing compiler.

`Recorder` exposes the same call surface as `_ffi.Lib`, so the wrappers in ops.py are reused
verbatim to *record* instead of *launch*.  Which value goes into which slot of an op is stated in
oplayout.py (and read back by run_op() in csrc/lib.hip); the methods below hand over their arguments by name.
"""
import ctypes as C
import struct

from . import _ffi, oplayout


class Recorder(object):
    def __init__(self):
        self.ops = []
        self.keep = []          # python objects (tensors) that must outlive the plan
        # algorithmic work of the recorded step (SURVEY 8(d) definitions): conv = forward + input-gradient launches,
        # wgrad = filter gradients; *_bytes = each operand read / result written once; wgrad_ws_bytes = split-K partial sums
        self.stats = {"conv_flops": 0.0, "conv_bytes": 0.0, "wgrad_flops": 0.0, "wgrad_bytes": 0.0, "wgrad_ws_bytes": 0.0,
                      "grad_bytes": 0.0, "conv_launches": 0, "wgrad_launches": 0}
        self.lane = 0           # scheduling lane of the ops recorded next (the scheduling word: oplayout.sched_word)
        self.join_next = False  # next op: lane 0 first waits for the side lanes
        self.join_lanes_next = 0  # next op: lane 0 first waits for exactly the side lanes of this bit mask (bit l = lane l)
        self.nodefer = False      # side-lane ops recorded now are launched at once (MH_OP_NODEFER)
        self.wgrad_group_max_m = 0  # grouped filter-gradient launches: pixel cap of this plan's layers (0 = library default)
        self.label_loss = 0         # the `loss` slot of the PROXY_LOSS / PROXY_LOSS_SCALED ops recorded next (_ffi.LABEL_LOSS; 0 = mean_l1, today's entry points)
        self.smoothness = 0.0       # the `smooth_weight` slot of the LOSS ops recorded next: weight of the edge-aware smoothness term (0 = the reprojection loss alone)
        self.loss_masked = False    # True: the LOSS ops recorded next carry oplayout.LOSS_MASKED in their `phase` slot (validity masks in their workspace: ops.loss_set_valid)
        self.work = {}              # op index -> (algorithmic flops, bytes) of the multi-layer ops (a streamed filter-gradient batch)
        self._pending_work = [0.0, 0.0]
        self.cuts = []              # op indices where compile_parts() splits the recording (a collective goes between the parts)
        self.refs = []              # (op index, data pointer, bytes): tensors an op reaches through a DEVICE TABLE (segment tables of casts / splits /
                                    # streamed filter gradients) -- invisible in the op's own pointer fields, seen by the dead-store post-passes
        self.elided = []            # [(pointer, bytes)] of fp32 buffers the recorded step no longer writes (elision._note_elided)

    def note_refs(self, pairs):
        """pairs: [(data pointer, bytes)] read or written through the device table of the op recorded NEXT"""
        self.refs += [(len(self.ops), int(a), int(nb)) for a, nb in pairs if a]

    def cut(self):
        """Mark a split point: every op recorded so far forms one part (mh_plan_run joins the side lanes at the end of a plan, so
        a part ends with all of its work ordered before whatever the caller enqueues next on the stream)."""
        if len(self.ops) and (not self.cuts or self.cuts[-1] != len(self.ops)):
            self.cuts.append(len(self.ops))

    # -- helpers ---------------------------------------------------------------------------
    def _op(self, kind, vals, **over):
        """Record one op: the slots of `kind` (oplayout) by name from `vals` -- a recorder method hands over its own locals() -- and `over`."""
        if over:
            vals = dict(vals, **over)
        self.ops.append(oplayout.pack(kind, vals, oplayout.sched_word(self.lane, self.join_next, self.join_lanes_next, self.nodefer)))
        self.join_next = False
        self.join_lanes_next = 0

    def _desc_op(self, kind, dref, vals, **over):
        """_op for the kinds that carry a descriptor: its fields are slots by their own names"""
        d = dref._obj
        v = {name: getattr(d, name) for name, _ in d._fields_}
        v.update(vals)
        self._op(kind, v, **over)

    # -- same names / argument order as _ffi.Lib (minus the 'mh_' prefix) --------------------
    def _tally(self, d, kind, splits=0):
        taps = d.kh * d.kw
        if kind == "conv":          # mode 0: in = x, out = y ; mode 1: in = dz (Hi x Wi), out = dx
            flops = 2.0 * d.B * (d.Ho * d.Wo if d.mode == 0 else d.Hi * d.Wi) * taps * d.K * d.N
            byts = 4.0 * (d.B * d.Hi * d.Wi * d.K + d.B * d.Ho * d.Wo * d.N + taps * d.K * d.N)
            self.stats["conv_flops"] += flops; self.stats["conv_bytes"] += byts; self.stats["conv_launches"] += 1
        else:
            flops = 2.0 * d.B * d.Ho * d.Wo * taps * d.K * d.N
            byts = 4.0 * (d.B * d.Hi * d.Wi * d.K + d.B * d.Ho * d.Wo * d.N + taps * d.K * d.N)
            self.stats["wgrad_flops"] += flops; self.stats["wgrad_bytes"] += byts; self.stats["wgrad_launches"] += 1
            self.stats["grad_bytes"] += 4.0 * taps * d.K * d.N
            if splits > 1:
                self.stats["wgrad_ws_bytes"] += 2 * 4.0 * splits * taps * d.K * d.N      # written by the splits, read by the reduction

    def _conv2d(self, dref, inp, w, bias, out, mask, wb=None, shadow=None, in_shadow=None, flags=0):
        """the six mh_conv2d* forms are ONE op kind (oplayout: OP_CONV)"""
        self._tally(dref._obj, "conv")
        self._desc_op(_ffi.OP_CONV, dref, locals())

    def conv2d(self, dref, inp, w, bias, out, mask, stream):
        self._conv2d(dref, inp, w, bias, out, mask)

    def conv2d_wb(self, dref, inp, w, wb, bias, out, mask, stream):
        self._conv2d(dref, inp, w, bias, out, mask, wb)

    def conv2d_sh(self, dref, inp, w, wb, bias, out, mask, shadow, stream):
        self._conv2d(dref, inp, w, bias, out, mask, wb, shadow)

    def conv2d_sh4(self, dref, inp, w, wb, bias, out, mask, out_hi, out_lo, stream):
        self._conv2d(dref, inp, w, bias, out, mask, wb, shadow=out_hi, in_shadow=out_lo, flags=oplayout.CONV_OUT_PLANES)

    def conv2d_sh2(self, dref, inp, in_shadow, w, wb, bias, out, mask, shadow, stream):
        self._conv2d(dref, inp, w, bias, out, mask, wb, shadow, in_shadow, oplayout.CONV_IN_SHADOW)

    def conv2d_sh3(self, dref, inp, in_shadow, w, wb, bias, out, mask, mask_shadow, shadow, flags, stream):
        assert bias is None         # (input gradients carry no bias: the slot holds the mask's shadow)
        bits = ((oplayout.CONV_IN_SHADOW if in_shadow is not None else 0) | (oplayout.CONV_MASK_SHADOW if mask_shadow is not None else 0)
                | (oplayout.CONV_SHADOW_ONLY if flags & 1 else 0))
        self._conv2d(dref, inp, w, mask_shadow, out, mask, wb, shadow, in_shadow, bits)

    def conv2d_planes(self, dref, in_hi, in_lo, in_pld, wb32, bias, out, out_hi, out_lo, out_pld, stream):
        self._tally(dref._obj, "conv")
        self._desc_op(_ffi.OP_CONV_PLANES, dref, locals(), precision=(1 if dref._obj.precision == 1 else 2))

    def stamp(self, slot, stream):
        self._op(_ffi.OP_STAMP, locals())

    def det_flush(self, dst, twin, n, stream):
        self._op(_ffi.OP_DET_FLUSH, locals())

    def conv2d_planes_bwd(self, dref, dz_hi, dz_pld, wb32t, mask_hi, mask_pld, dx, dx_hi, dx_pld, stream):
        d = dref._obj
        # (tallied as the input-gradient launch it is: flops of the layer, dz in, dx out)
        flops = 2.0 * d.B * d.Hi * d.Wi * 9 * d.K * d.N
        self.stats["conv_flops"] += flops; self.stats["conv_bytes"] += 4.0 * (d.B * d.Hi * d.Wi * (d.K + d.N) + 9 * d.K * d.N); self.stats["conv_launches"] += 1
        self._desc_op(_ffi.OP_CONV_PLANES_BWD, dref, locals(), precision=1)

    def plane_split(self, segs, nseg, nblocks, stream):
        self._op(_ffi.OP_PLANE_SPLIT, locals())

    def pack_weights(self, segs, nseg, nblocks, stream):
        self._op(_ffi.OP_PACK_W, locals())

    def conv2d_wgrad(self, dref, inp, dout, dout_ld, dw, db, stream):
        self._tally(dref._obj, "wgrad")
        self._desc_op(_ffi.OP_WGRAD, dref, locals())

    def conv2d_wgrad_partial(self, dref, inp, dout, dout_ld, ws, splits_ref, db, stream):
        splits = splits_ref._obj.value
        self._tally(dref._obj, "wgrad", splits if ws is not None else 0)
        self._desc_op(_ffi.OP_WGRAD_PARTIAL, dref, locals(), group_max_m=self.wgrad_group_max_m)

    def shadow_cast(self, segs, nseg, nblocks, stream):
        self._op(_ffi.OP_SHADOW_CAST, locals())

    def wgrad_stream(self, layers, nlayers, nblocks, nwaves, max_dil, stream):
        self.work[len(self.ops)] = tuple(self._pending_work)
        self._pending_work = [0.0, 0.0]
        self._op(_ffi.OP_WGRAD_STREAM, locals())

    def tally_wgrad(self, B, H, W, K, N, taps, splits):
        """work of one layer of a streamed filter-gradient batch (the batch is ONE op)"""
        self.stats["wgrad_flops"] += 2.0 * B * H * W * taps * K * N
        self.stats["wgrad_bytes"] += 4.0 * (B * H * W * (K + N) + taps * K * N)
        self._pending_work[0] += 2.0 * B * H * W * taps * K * N
        self._pending_work[1] += 2.0 * B * H * W * ((K + 31) // 32 * 32 + (N + 31) // 32 * 32) + 4.0 * taps * K * N      # bf16 shadows in, fp32 gradient out
        self.stats["wgrad_launches"] += 1
        self.stats["grad_bytes"] += 4.0 * taps * K * N
        if splits > 1:
            self.stats["wgrad_ws_bytes"] += 2 * 4.0 * splits * taps * K * N

    def conv2d_head(self, dref, inp, w, bias, out, out2, out2_ld, out3, out3_ld, stream):
        self._tally(dref._obj, "conv")
        self._desc_op(_ffi.OP_HEAD_FWD, dref, locals())

    def head_bwd(self, dref, src0, src1, dV, dV_shadow, w, dx, mask, dx_shadow, stream):
        self._desc_op(_ffi.OP_HEAD_BWD, dref, locals())

    def wgrad_reduce(self, segs, nseg, nblocks, stream):
        self._op(_ffi.OP_WGRAD_REDUCE, locals())

    def corr_fwd(self, L, l_ld, R, r_ld, u, out, out_ld, coff, B, H, W, Cc, md, stride, copy_left, zero_tail, stream):
        self.corr_fwd_prec(L, l_ld, R, r_ld, u, out, out_ld, coff, B, H, W, Cc, md, stride, copy_left, zero_tail, 0, stream)

    def corr_fwd_prec(self, L, l_ld, R, r_ld, u, out, out_ld, coff, B, H, W, Cc, md, stride, copy_left, zero_tail, precision, stream):
        self._op(_ffi.OP_CORR_FWD, locals())

    # (the three forms of OP_LEVEL_FRONT: without planes out_pld = 0 and no out_hi / out_lo, without the coarser level's head no X)
    def level_front_fwd(self, Vc, Hc, Wc, mul, L, l_ld, R, r_ld, out, out_ld, coff, Rw, rw_ld, u, B, H, W, Cc, md, zero_tail, stream):
        self.level_front_fwd_planes(Vc, Hc, Wc, mul, L, l_ld, R, r_ld, out, out_ld, coff, Rw, rw_ld, u, B, H, W, Cc, md, zero_tail, None, None, 0, stream)

    def level_front_fwd_planes(self, Vc, Hc, Wc, mul, L, l_ld, R, r_ld, out, out_ld, coff, Rw, rw_ld, u, B, H, W, Cc, md, zero_tail, out_hi, out_lo, out_pld, stream):
        self.level_front_head_fwd(None, 0, 0, None, None, Vc, Hc, Wc, mul, L, l_ld, R, r_ld, out, out_ld, coff, Rw, rw_ld, u, B, H, W, Cc, md, zero_tail, out_hi, out_lo, out_pld, stream)

    def level_front_head_fwd(self, X, x_ld, K, hw, hb, Vc, Hc, Wc, mul, L, l_ld, R, r_ld, out, out_ld, coff, Rw, rw_ld, u, B, H, W, Cc, md, zero_tail, out_hi, out_lo, out_pld,
                             stream):
        self._op(_ffi.OP_LEVEL_FRONT, locals())

    def conv_image_fwd(self, frames, NB, H0, W0, Cc, Hp, Wp, rpt, rpl, div, sub, w, bias, N, stride, pad_t, pad_l, alpha, out, out_ld, shadow, shadow_ld, stream):
        self._op(_ffi.OP_CONV_IMAGE, locals())

    def corr_bwd(self, g, g_ld, coff, L, l_ld, R, r_ld, dL, dl_ld, acc_l, dR, dr_ld, acc_r, du, acc_u,
                 B, H, W, Cc, md, stride, copy_left, stream):
        self.corr_bwd_prec(g, g_ld, coff, L, l_ld, R, r_ld, dL, dl_ld, acc_l, dR, dr_ld, acc_r, du, acc_u, B, H, W, Cc, md, stride, copy_left, 0, stream)

    def corr_bwd_prec(self, g, g_ld, coff, L, l_ld, R, r_ld, dL, dl_ld, acc_l, dR, dr_ld, acc_r, du, acc_u,
                      B, H, W, Cc, md, stride, copy_left, precision, stream):
        self._op(_ffi.OP_CORR_BWD, locals())

    def corr_warp_bwd(self, g, g_ld, coff, L, l_ld, Rw, rw_ld, img, img_ld, u, dL, dl_ld, acc_l, dimg, dimg_ld, du, B, H, W, Cc, md, stride, copy_left, stream):
        self._op(_ffi.OP_CORR_WARP_BWD, locals())

    def warp_fwd(self, img, img_ld, u, out, out_ld, B, H, W, Cc, stream):
        self._op(_ffi.OP_WARP_FWD, locals())

    def warp_bwd(self, g, g_ld, img, img_ld, u, dimg, dimg_ld, du, acc_u, B, H, W, Cc, stream):
        self._op(_ffi.OP_WARP_BWD, locals())

    def resize_fwd(self, inp, out, B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode, stream):
        self._op(_ffi.OP_RESIZE_FWD, locals(), accumulate=0)

    def resize_bwd(self, g, inp, din, accumulate, B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode, stream):
        self._op(_ffi.OP_RESIZE_BWD, locals())

    def resize_image_fwd(self, inp, out, B, Hi, Wi, Cc, Ho, Wo, stream):
        self._op(_ffi.OP_RESIZE_IMAGE, locals())

    def pad_reflect(self, inp, out, B, H, W, Cc, Hp, Wp, pt, pl, out_ld, div, sub, stream):
        self._op(_ffi.OP_PAD_REFLECT, locals())

    def reprojection_loss(self, left, right, disp, ws, result, ddisp, grad_scale, B, H, W, stream):
        self.reprojection_loss_phase(left, right, disp, ws, result, ddisp, grad_scale, B, H, W, 0, stream)

    def reprojection_loss_phase(self, left, right, disp, ws, result, ddisp, grad_scale, B, H, W, phase, stream):
        self._op(_ffi.OP_LOSS, locals(), smooth_weight=self.smoothness, phase=phase | (oplayout.LOSS_MASKED if self.loss_masked else 0))

    def proxy_loss(self, pred, proxy, ws, result, dpred, weight, grad_scale, B, H, W, stream):
        self._op(_ffi.OP_PROXY_LOSS, locals(), loss=self.label_loss)

    def proxy_loss_scaled(self, pred, proxy, ws, result, dpred, weight, grad_scale, scale, B, H, W, stream):
        self._op(_ffi.OP_PROXY_LOSS_SCALED, locals(), loss=self.label_loss)

    def supervised_loss(self, pred, target, ws, result, dpred, weight, grad_scale, max_disp, B, H, W, stream):
        self._op(_ffi.OP_SUPERVISED_LOSS, locals())

    def adam(self, var, m, v, grad, n, state, lr, beta1, beta2, eps, gs, stream):
        self._op(_ffi.OP_ADAM, locals(), gs_bits=struct.unpack("<i", struct.pack("<f", gs))[0])

    def adam_advance(self, state, beta1, beta2, stream):
        self._op(_ffi.OP_ADAM_ADVANCE, locals())

    def metrics(self, disp, gt, ws, result, th, B, H, W, stream):
        self._op(_ffi.OP_METRICS, locals())

    def metrics_kitti(self, disp, gt, ws, result, B, H, W, stream):
        self._op(_ffi.OP_METRICS_KITTI, locals())

    def momentum(self, var, accum, grad, n, lr, mom, gs, stream):
        self._op(_ffi.OP_MOMENTUM, locals())

    def copy_channels(self, src, src_ld, dst, dst_ld, npix, nch, scale, accumulate, stream):
        self._op(_ffi.OP_COPY_CH, locals())

    def leaky_bwd(self, dy, dy_ld, y, y_ld, npix, nch, alpha, stream):
        self._op(_ffi.OP_LEAKY_BWD, locals())

    def bias_grad(self, dz, dz_ld, npix, nch, db, stream):
        self._op(_ffi.OP_BIAS_GRAD, locals(), nblocks=0)

    def bias_grad_partial(self, dz, dz_ld, npix, nch, ws, nblocks, stream):
        self._op(_ffi.OP_BIAS_GRAD, locals(), db=ws)

    def _counted(self, kind, nmax, n, counts, tail, ptrs, **head):
        """an op with a counted tail (oplayout): the first n of the nmax slots count<k> / <tail><k> are set"""
        vals = dict(head, n=n)
        for k in range(nmax):
            vals["count%d" % k] = counts[k] if k < n else 0
            vals["%s%d" % (tail, k)] = ptrs[k] if k < n else None
        self._op(kind, vals)

    def allreduce_sum(self, bufs, counts, n, comm, stream):
        """bufs / counts: ctypes arrays as for _ffi.Lib.allreduce_sum (the recorder copies the n pointers and counts into the op)"""
        assert 1 <= n <= _ffi.ALLREDUCE_MAX_BUFS
        self._counted(_ffi.OP_ALLREDUCE, _ffi.ALLREDUCE_MAX_BUFS, n, counts, "buf", bufs, comm=comm)

    def fetch_inputs(self, table, dst, counts, n, stream):
        """table: device-visible address of an mh_input_table; dst / counts: ctypes arrays as for _ffi.Lib.fetch_inputs"""
        assert 1 <= n <= _ffi.FETCH_MAX
        self._counted(_ffi.OP_FETCH_INPUTS, _ffi.FETCH_MAX, n, counts, "dst", dst, table=table)

    def fill(self, p, n, v, stream):
        self._op(_ffi.OP_FILL, locals())

    # -- finalise ---------------------------------------------------------------------------
    def _plan(self, a, b, stats):
        """the Plan of ops a .. b - 1 (the elision is a property of the recorded step, whichever part a reader holds)"""
        p = Plan((_ffi.Op * (b - a))(*self.ops[a:b]), b - a, self.keep, stats)
        p.work = {k - a: v for k, v in self.work.items() if a <= k < b}
        p.elided = list(self.elided)
        return p

    def compile(self):
        return self._plan(0, len(self.ops), dict(self.stats))

    def compile_parts(self):
        """One Plan per section between cut() marks (the work statistics stay with the first)."""
        bounds = [0] + [c for c in self.cuts if 0 < c < len(self.ops)] + [len(self.ops)]
        return [self._plan(a, b, dict(self.stats) if a == 0 else {}) for a, b in zip(bounds[:-1], bounds[1:])]


class Plan(object):
    """An immutable op array + (optionally) its captured hipGraph."""

    def __init__(self, arr, n, keep, stats=None):
        self.arr, self.n, self.keep, self.stats = arr, n, keep, stats or {}
        self.graph = None
        self.work = {}
        self.elided = []          # [(pointer, bytes)] of fp32 buffers the recorded step no longer writes (Recorder._plan fills it)
        self.graphs, self._turn = [], 0       # capture(copies > 1): the executable graphs and the one launched last

    def run(self, lib, stream):
        lib.plan_run(self.arr, self.n, C.c_void_p(stream))

    def capture(self, lib, stream, copies=1):
        """Capture the plan into a hipGraph on `stream` (must not be the legacy default stream).  copies > 1: that many executable graphs of the same plan, launched
        in turn -- a replay enqueued while the previous one is in flight is then never the SAME executable (experiment r6v)."""
        s = C.c_void_p(stream)
        self.graphs = []
        for _ in range(max(1, copies)):
            lib.graph_begin(s)
            try:
                lib.plan_run(self.arr, self.n, s)
            finally:
                g = C.c_void_p()
                lib.graph_end(s, C.byref(g))
            self.graphs.append(g)
        self.graph, self._turn = self.graphs[0], 0

    def launch(self, lib, stream):
        if self.graph is not None:
            if len(self.graphs) > 1:
                self._turn = (self._turn + 1) % len(self.graphs)
                lib.graph_launch(self.graphs[self._turn], C.c_void_p(stream))
            else:
                lib.graph_launch(self.graph, C.c_void_p(stream))
        else:
            self.run(lib, stream)


class MultiPlan(object):
    """Several independent plans (one per private-model stream of a GPU) replayed as parallel branches of ONE hipGraph (mh_plans_run): the
    latency-bound step chains of S models share the chip instead of queueing behind one another."""

    def __init__(self, plans):
        self.plans = list(plans)
        self.refs = (_ffi.PlanRef * len(self.plans))()
        for i, p in enumerate(self.plans):
            self.refs[i].ops, self.refs[i].nops = C.addressof(p.arr), p.n
        self.graph = None
        self.n = sum(p.n for p in self.plans)

    def run(self, lib, stream):
        lib.plans_prepare(len(self.plans))
        lib.plans_run(self.refs, len(self.plans), C.c_void_p(stream))

    def capture(self, lib, stream):
        lib.plans_prepare(len(self.plans))
        s = C.c_void_p(stream)
        lib.graph_begin(s)
        try:
            lib.plans_run(self.refs, len(self.plans), s)
        finally:
            g = C.c_void_p()
            lib.graph_end(s, C.byref(g))
        self.graph = g

    def launch(self, lib, stream):
        if self.graph is not None:
            lib.graph_launch(self.graph, C.c_void_p(stream))
        else:
            self.run(lib, stream)
