"""Dead-store elimination over a recorded MADNet plan (post-passes of MadNetEngine.build_plan): fp32 tensors that only bf16-reading kernels consume are not
stored at all.  A mixin of MadNetEngine: the passes read the engine's tensor lists (E, Cx, dE, dCx), its library handle and its Schedule."""
import ctypes as C

from . import _ffi, oplayout
from .netdef import LEVELS
from .oplayout import fields


def _dgrad(op, bit):
    """fields of `op` if it is an input gradient of the tiled families in the bf16 arithmetic that was given the shadow `bit` names, else None"""
    if op.kind != _ffi.OP_CONV:
        return None
    f = fields(op)
    return f if (f.mode == 1 and f.precision == 1 and (f.flags & bit)) else None


class ElisionPasses(object):
    def _elide_fp32_gradient_maps(self, r):
        """Post-pass over the recorded plan (dead-store elimination): an input-gradient launch that writes the bf16 shadow of its result does not
        store the fp32 map when the ONLY op that touches that buffer afterwards is the next input gradient and that launch stages the shadow
        (mh_conv2d_takes_shadows answers for the recorded descriptor): inside the 1/4-resolution estimator and the context network the gradient
        maps then exist in bf16 only (15.7 MB less written per 128-channel layer)."""
        if not (self.sched.SHADOW_DGRAD and self.sched.SHADOW_ONLY):
            return 0
        ops_ = r.ops
        n = 0
        spans = []
        for idx, o in enumerate(ops_):
            f = fields(o) if o.kind == _ffi.OP_CONV else None
            if f and f.mode == 1 and f.shadow and not f.accumulate and f.precision == 1 and f.out:
                spans.append((idx, int(f.out), int(f.out) + 4 * f.B * f.Ho * f.Wo * f.out_ld))
        for idx, lo, hi in spans:
            if any(a < hi and lo < a + nb for _, a, nb in r.refs):
                continue                # a device table (cast / split segment) reads the map
            users = [j for j, q in enumerate(ops_) if j != idx and oplayout.pointers_into(q, lo, hi)]
            if len(users) != 1 or users[0] < idx:
                continue
            c = ops_[users[0]]
            cf = _dgrad(c, oplayout.CONV_IN_SHADOW)
            if not (cf and int(cf.inp) == lo and len(oplayout.pointers_into(c, lo, hi)) == 1):
                continue
            if not (self._takes_shadows(c) & 1):
                continue
            fields(ops_[idx]).flags |= oplayout.CONV_SHADOW_ONLY
            cf.flags |= oplayout.CONV_IN_F32_STALE          # a replay whose dispatch no longer stages the shadow is refused, not wrong
            self._note_elided(r, lo, hi - lo)
            n += 1
        return n

    def _note_elided(self, r, ptr, nbytes):
        """An fp32 buffer no op of this plan writes any more.  Kept on the recorder / plan (plan.elided) so that a reader OUTSIDE the plan can ask; with
        MH_POISON_ELIDED=1 (tests) the buffer is filled with NaN at once: an op that still reads it -- a device-table op whose table building forgot
        Recorder.note_refs, a debug read of engine.E / Cx -- then fails loudly instead of consuming a stale map."""
        r.elided.append((int(ptr), int(nbytes)))
        if self.sched.POISON_ELIDED:
            t = self._tensor_by_ptr().get(int(ptr))
            if t is not None:
                t.fill_(float("nan"))

    def _tensor_by_ptr(self):
        out = {}
        for k in LEVELS:
            for t in list(self.E[k]) + list(self.dE[k]):
                out[t.data_ptr()] = t
        for t in list(self.Cx) + list(self.dCx):
            out[t.data_ptr()] = t
        return out

    def _takes_shadows(self, c):
        """mh_conv2d_takes_shadows for a recorded OP_CONV: bit 1 = the launch stages in_shadow, bit 2 = it reads the mask from mask_shadow"""
        d, f = oplayout.conv_desc(c), fields(c)
        return self.lib.conv2d_takes_shadows(C.byref(d), C.c_void_p(f.inp), C.c_void_p(f.w), C.c_void_p(f.wb), C.c_void_p(f.out), C.c_void_p(f.mask))

    def _standalone_activations(self):
        """{data pointer: bytes} of the activation tensors that are allocations of their own (no view of them can start in front of them): the only
        candidates for an elided fp32 store"""
        out = {}
        for k in LEVELS:
            for t in self.E[k]:
                out[t.data_ptr()] = t.numel() * 4
        for t in self.Cx:
            out[t.data_ptr()] = t.numel() * 4
        for k in LEVELS:                    # ... and the gradient maps between the input gradients of an estimator / the context network
            for t in self.dE[k]:
                out[t.data_ptr()] = t.numel() * 4
        for t in self.dCx:
            out[t.data_ptr()] = t.numel() * 4
        return out

    def _elide_fp32_activations(self, r):
        """Post-pass (dead-store elimination, forward side): a plane-writing forward layer (OP_CONV_PLANES) does not store its fp32 result when no op
        of the recorded plan reads that tensor -- the next forward layer takes the planes, the filter gradient the hi plane, the input gradient of the
        next layer the sign of the hi plane for its leaky mask (it gets MH_CONV_MASK_F32_STALE, so a replay under another dispatch fails loudly).
        Readers are found conservatively: any pointer field of any op, and any tensor a device table of an op references (Recorder.refs), that
        OVERLAPS the buffer."""
        if not (self.use_planes and self.sched.PLANES_ONLY):
            return 0
        ops_ = r.ops
        cand = self._standalone_activations()
        n = 0
        for idx, o in enumerate(ops_):
            if o.kind not in (_ffi.OP_CONV_PLANES, _ffi.OP_CONV_PLANES_BWD):
                continue
            f = fields(o)
            if o.kind == _ffi.OP_CONV_PLANES and f.out and f.out_hi and f.out_lo:
                slot = "out"                # forward: fp32 result beside both planes
            elif o.kind == _ffi.OP_CONV_PLANES_BWD and f.dx and f.dx_hi:
                slot = "dx"                 # input gradient: fp32 map beside its shadow
            else:
                continue
            lo = int(getattr(f, slot))
            if lo not in cand:
                continue
            hi = lo + cand[lo]
            if any(a < hi and lo < a + nb for _, a, nb in r.refs):
                continue
            ok, mask_users = True, []
            for j, q in enumerate(ops_):
                if j == idx:
                    continue
                hits = oplayout.pointers_into(q, lo, hi)
                if not hits:
                    continue
                # the only tolerated readers: an input gradient (tiled families) that was given this tensor as its leaky mask TOGETHER with the mask's
                # shadow and whose kernel tests the shadow -- or as its dz together with dz's shadow and whose kernel stages the shadow
                qf = _dgrad(q, oplayout.CONV_MASK_SHADOW)
                if qf and hits == ["mask"] and int(qf.mask) == lo and (self._takes_shadows(q) & 2):
                    mask_users.append((qf, oplayout.CONV_MASK_F32_STALE))
                    continue
                qf = _dgrad(q, oplayout.CONV_IN_SHADOW)
                if qf and hits == ["inp"] and int(qf.inp) == lo and (self._takes_shadows(q) & 1):
                    mask_users.append((qf, oplayout.CONV_IN_F32_STALE))
                    continue
                ok = False
                break
            if not ok:
                continue
            setattr(f, slot, None)
            for qf, bit in mask_users:
                qf.flags |= bit
            self._note_elided(r, lo, hi - lo)
            n += 1
        return n
