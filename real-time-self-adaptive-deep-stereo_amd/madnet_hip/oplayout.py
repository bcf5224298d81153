"""Field layout of the plan record mh_op (include/madnet_hip.h: kind, i[27], f[4], p[12], n): THE host-side statement of which value sits in which
slot, per op kind.  plan.Recorder packs through it, every reader (elision passes, benchtools, scripts, tests) reads and mutates through `fields(op)`;
run_op() of csrc/lib.hip is the native reader, the argument order of the mh_* entry points is its statement of the same layout.

One line per kind in _TABLE: slot names in slot order, "_" = slot not used, "a/b" = one slot with two meanings (first name = the one packed by),
"name*N" = a counted tail name0 .. name<N-1>.  Names are the Recorder's argument names wherever an argument goes into the slot as it is."""
import ctypes as C

from . import _ffi

# ---- the scheduling word: slot i[26] of EVERY kind (mh_op in the header) -------------------------------------------------------------------------
SCHED_SLOT = 26
LANE_MASK = 0xff                # low byte: the lane (0 = the caller's stream, 1 .. MAX_LANES - 1 = side lanes)
OP_JOIN = _ffi.OP_JOIN          # lane 0 first waits for every side lane
OP_NODEFER = _ffi.OP_NODEFER    # a side-lane op that is launched at once
JOIN_LANES_SHIFT = 16           # bits 16 .. 23: first wait for exactly these side lanes (bit l = lane l)


def sched_word(lane, join=False, join_lanes=0, nodefer=False):
    return lane | (OP_JOIN if join else 0) | ((join_lanes & 0xff) << JOIN_LANES_SHIFT) | (OP_NODEFER if (nodefer and lane > 0) else 0)


def lane_of(op):
    return op.i[SCHED_SLOT] & LANE_MASK


def on_callers_stream(op):
    """the op alone on the caller's stream: lane 0, no join (a copy of a plan's op that is timed by itself)"""
    op.i[SCHED_SLOT] = 0
    return op


# ---- OP_CONV's flag word, slot i[23] (not the MH_CONV_* flags of mh_conv2d_sh3: run_op translates) ---------------------------------------------------
CONV_IN_SHADOW = 1          # p[5] is the bf16 shadow of the input
CONV_MASK_SHADOW = 2        # p[2] is the bf16 shadow of the mask (else the bias)
CONV_SHADOW_ONLY = 4        # the fp32 result is not stored
CONV_IN_F32_STALE = 8       # the fp32 input was not stored: refused unless the dispatched kernel stages the shadow
CONV_MASK_F32_STALE = 16    # likewise the fp32 mask
CONV_OUT_PLANES = 32        # p[7] / p[5] are the hi / lo planes of the result (mh_conv2d_sh4)
# OP_LOSS, `phase` slot (MH_LOSS_MASKED): phase | LOSS_MASKED = mh_reprojection_loss_masked, its validity masks at mh_loss_valid_offset of the record's own ws (Recorder.loss_masked)
LOSS_MASKED = 4

# ---- the prefix the conv kinds share: the mh_conv_desc ints in slots 0 .. 20, precision in 22, alpha / mask_alpha in f ----------------------------------
DESC_I = "B Hi Wi Ho Wo K N kh kw stride dil pad_t pad_l mode w_trans in_ld out_ld mask_ld accumulate mask_c0 mask_c1"
DESC_F = "alpha mask_alpha"
DESC_FIELDS = tuple(DESC_I.split() + DESC_F.split() + ["precision"])


def _desc(slot21="_", tail=""):
    return "%s %s precision %s" % (DESC_I, slot21, tail)


_TABLE = {
    # OP_CONV: one record for the six mh_conv2d* forms, told apart by `flags` and by which of wb / shadow is set (run_op's ladder)
    "CONV": dict(i=_desc(tail="flags"), f=DESC_F, p="inp w bias/mask_shadow out mask in_shadow/out_lo wb shadow/out_hi"),
    "WGRAD": dict(i=_desc("dout_ld"), f=DESC_F, p="inp dout dw db"),
    "WGRAD_PARTIAL": dict(i=_desc("dout_ld", "splits group_max_m"), f=DESC_F, p="inp dout ws db"),
    "HEAD_FWD": dict(i=_desc(tail="out2_ld out3_ld"), f=DESC_F, p="inp w bias out out2 out3"),
    "CONV_PLANES": dict(i=_desc(tail="in_pld out_pld"), f=DESC_F, p="in_hi in_lo wb32 bias out out_hi out_lo"),
    "CONV_PLANES_BWD": dict(i=_desc(tail="dz_pld mask_pld dx_pld"), f=DESC_F, p="dz_hi wb32t mask_hi dx dx_hi"),     # (the FORWARD layer's descriptor)
    "CONV_IMAGE": dict(i="NB H0 W0 Cc Hp Wp rpt rpl N stride pad_t pad_l out_ld shadow_ld", f="div sub alpha", p="frames w bias out shadow"),
    "HEAD_BWD": dict(i="kind B H W N Hr Wr cy cx Ho Wo src0_ld src1_ld dx_ld mask_ld accumulate_dx", f="mul mask_alpha", p="src0 src1 dV dV_shadow w dx mask dx_shadow"),
    "CORR_FWD": dict(i="l_ld r_ld out_ld coff B H W Cc md stride copy_left zero_tail precision", p="L R u out"),
    "CORR_BWD": dict(i="g_ld coff l_ld r_ld dl_ld acc_l dr_ld acc_r acc_u B H W Cc md stride copy_left precision", p="g L R dL dR du"),
    "CORR_WARP_BWD": dict(i="g_ld coff l_ld rw_ld img_ld dl_ld acc_l dimg_ld B H W Cc md stride copy_left", p="g L Rw img u dL dimg du"),
    # OP_LEVEL_FRONT: X set = the coarser level's disparity head runs in the same launch (then hw, hb, x_ld, K count)
    "LEVEL_FRONT": dict(i="Hc Wc l_ld r_ld out_ld coff rw_ld B H W Cc md zero_tail out_pld x_ld K", f="mul", p="Vc L R out Rw u out_hi out_lo X hw hb"),
    "WARP_FWD": dict(i="img_ld out_ld B H W Cc", p="img u out"),
    "WARP_BWD": dict(i="g_ld img_ld dimg_ld acc_u B H W Cc", p="g img u dimg du"),
    "RESIZE_FWD": dict(i="B Hi Wi Hr Wr cy cx Ho Wo mode accumulate", f="mul", p="inp out"),
    "RESIZE_BWD": dict(i="B Hi Wi Hr Wr cy cx Ho Wo mode accumulate", f="mul", p="g inp din"),
    "RESIZE_IMAGE": dict(i="B Hi Wi Cc Ho Wo", p="inp out"),
    "PAD_REFLECT": dict(i="B H W Cc Hp Wp pt pl out_ld", f="div sub", p="inp out"),
    # OP_LOSS: smooth_weight != 0 = mh_smoothness_loss(disp, left) follows the reprojection loss and adds its term to result[0] and ddisp (Recorder.smoothness)
    "LOSS": dict(i="B H W phase", f="grad_scale smooth_weight", p="left right disp ws result ddisp"),
    # OP_PROXY_LOSS / OP_PROXY_LOSS_SCALED: loss = _ffi.LABEL_LOSS (MH_LOSS_*); 0 = mean_l1 through mh_proxy_loss / mh_proxy_loss_scaled, else mh_label_loss* (rule 0, hi 192)
    "PROXY_LOSS": dict(i="B H W loss", f="weight grad_scale", p="pred proxy ws result dpred"),
    "PROXY_LOSS_SCALED": dict(i="B H W scale loss", f="weight grad_scale", p="pred proxy ws result dpred"),
    "SUPERVISED_LOSS": dict(i="B H W", f="weight grad_scale max_disp", p="pred target ws result dpred"),
    "METRICS": dict(i="B H W", f="th", p="disp gt ws result"),
    "METRICS_KITTI": dict(i="B H W", p="disp gt ws result"),
    "MOMENTUM": dict(f="lr mom gs", p="var accum grad", n="n"),
    "ADAM": dict(i="gs_bits", f="lr beta1 beta2 eps", p="var m v grad state", n="n"),       # gs_bits: the float grad_scale bit-cast into the int slot
    "ADAM_ADVANCE": dict(f="beta1 beta2", p="state"),
    "COPY_CH": dict(i="src_ld dst_ld nch accumulate", f="scale", p="src dst", n="npix"),
    "LEAKY_BWD": dict(i="dy_ld y_ld nch", f="alpha", p="dy y", n="npix"),
    "FILL": dict(f="v", p="p", n="n"),
    # OP_BIAS_GRAD: nblocks > 0 = the partial form (mh_bias_grad_partial), p[1] is then the workspace [nblocks][nch]
    "BIAS_GRAD": dict(i="dz_ld nch nblocks", p="dz db/ws", n="npix"),
    "WGRAD_REDUCE": dict(i="nseg nblocks", p="segs"),
    "PACK_W": dict(i="nseg nblocks", p="segs"),
    "SHADOW_CAST": dict(i="nseg nblocks", p="segs"),
    "PLANE_SPLIT": dict(i="nseg nblocks", p="segs"),
    "WGRAD_STREAM": dict(i="nlayers nblocks nwaves max_dil", p="layers"),
    "STAMP": dict(p="slot"),
    "DET_FLUSH": dict(p="dst twin", n="n"),
    # counted tails: the first n of the counts / pointers are set
    "ALLREDUCE": dict(i="n count*%d" % _ffi.ALLREDUCE_MAX_BUFS, p="comm buf*%d" % _ffi.ALLREDUCE_MAX_BUFS),
    "FETCH_INPUTS": dict(i="n count*%d" % _ffi.FETCH_MAX, p="table dst*%d" % _ffi.FETCH_MAX),
    "RESERVED_25": dict(),
}
_SIZE = {"i": SCHED_SLOT, "f": 4, "p": 12}      # (i: the slots in front of the scheduling word)


class Layout(object):
    """name; i / f / p: [(slot, name packed by)] in slot order; n: name of the value in mh_op.n or None; at: {name: (array, slot)}, aliases included"""

    def __init__(self, name, i="", f="", p="", n=None):
        self.name, self.n = name, n
        self.at = {"sched": ("i", SCHED_SLOT)}
        if n:
            self.at[n] = ("n", 0)
        for arr, spec in (("i", i), ("f", f), ("p", p)):
            slots = []
            for tok in spec.split():
                base, _, count = tok.partition("*")
                slots += [base + str(k) for k in range(int(count))] if count else [base]
            assert len(slots) <= _SIZE[arr], (name, arr)
            packed = []
            for k, tok in enumerate(slots):
                if tok == "_":
                    continue
                for alias in tok.split("/"):
                    assert alias not in self.at, (name, alias)
                    self.at[alias] = (arr, k)
                packed.append((k, tok.split("/")[0]))
            setattr(self, arr, packed)
        self.pnames = dict((k, nm) for k, nm in self.p)


LAYOUT = {}         # kind -> Layout
for _name, _spec in _TABLE.items():
    LAYOUT[getattr(_ffi, "OP_" + _name)] = Layout(_name, **_spec)


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, C.c_void_p):
        return x.value
    return int(x)


def pack(kind, values, sched=0):
    """A new mh_op of `kind` from {name: value}: every slot the layout names must be given (the second meaning of a two-meaning slot goes in under the
    first name)."""
    L = LAYOUT[kind]
    o = _ffi.Op()
    o.kind = kind
    oi, of, op = o.i, o.f, o.p          # (views of the record's own arrays)
    for k, name in L.i:
        v = int(values[name])
        if not -0x80000000 <= v <= 0x7fffffff:      # (ctypes would store the low 32 bits without a word)
            raise ValueError("%s: %s = %d does not fit the int32 slot i[%d]" % (L.name, name, v, k))
        oi[k] = v
    for k, name in L.f:
        of[k] = float(values[name])
    for k, name in L.p:
        op[k] = _ptr(values[name])
    if L.n:
        o.n = int(values[L.n])
    oi[SCHED_SLOT] = sched
    return o


class fields(object):
    """An op's fields by name: fields(op).mode, fields(op).flags |= CONV_SHADOW_ONLY, fields(op).out = None (pointers read as int or None)."""
    __slots__ = ("op", "_at")

    def __init__(self, op):
        object.__setattr__(self, "op", op)
        object.__setattr__(self, "_at", LAYOUT[op.kind].at)

    def _slot(self, name):
        """(the array or the record itself, index or attribute name)"""
        if name not in self._at:
            raise AttributeError("%s has no field %r" % (LAYOUT[self.op.kind].name, name))
        arr, k = self._at[name]
        return (self.op, "n") if arr == "n" else (getattr(self.op, arr), k)

    def __getattr__(self, name):
        obj, k = self._slot(name)
        return obj.n if k == "n" else obj[k]

    def __setattr__(self, name, value):
        obj, k = self._slot(name)
        if k == "n":
            obj.n = value
        else:
            obj[k] = value


def pointers_into(op, lo, hi):
    """names of the op's pointer slots that point into [lo, hi) -- ALL twelve slots are looked at, a slot the layout does not name counts as None, a
    two-meaning slot under its first name"""
    names = LAYOUT[op.kind].pnames
    return [names.get(k) for k, a in enumerate(op.p) if a and lo <= a < hi]


def conv_desc(op):
    """the _ffi.ConvDesc a recorded op of a conv kind carries"""
    f = fields(op)
    return _ffi.ConvDesc(**{name: getattr(f, name) for name in DESC_FIELDS})
