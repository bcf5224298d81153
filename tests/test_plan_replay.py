"""Every plan op kind, recorded and replayed, against the direct call of its entry point: pins run_op() of csrc/lib.hip, the NATIVE reader of the
mh_op record (tests/test_plan_packing.py pins the host side and launches nothing).

A case (CASES) builds its inputs once from literal seeds and states ONE call of an entry point as `call(target, outputs)`; the target is the library
(the direct call) or a plan.Recorder, which have the same call surface.  The direct call writes one set of outputs, the recorded op -- compiled and
run with mh_plan_run -- a second set; every buffer, inputs included, is a footprint.Guarded allocation prefilled with a NaN pattern.  Asserted per case:
  1. the replay noted the same kernel as the direct call (mh_last_kernel; another kernel is noted in between);
  2. the outputs of the replay equal those of the direct call ON BITS over the whole allocation, guards included -- every kind but the ones of 3.;
  3. outputs that accumulate with fp32 atomics across workgroups are judged against their float64 oracle instead, direct and replay each, with the bound
     the op has in its own sweep:  WARP_BWD dimg / du and CORR_WARP_BWD dimg / du: GRAD (5e-5) of test_shape_sweep.py, du with its atol 2e-5;
     BIAS_GRAD (atomic form) 1e-5 of test_ops_parity.py::test_bias_grad_column_sums;  WGRAD dw 1e-4 (exact fp32) and db 1e-4, the bias output of
     WGRAD_PARTIAL and of WGRAD_STREAM 1e-4 (test_conv_sweep.py / test_wgrad_sweep.py).  Everything else of those kinds (dL, partial sums) is compared on bits;
     STAMP stores a clock: the replayed stamp is written and not earlier than the direct one;
  4. the direct result is finite, written where the entry point documents it (a channel slice: nothing outside it) and not constant; cases that
     name an oracle are checked against the float64 oracle and the bound of the op's sweep (FWD / GRAD of test_shape_sweep.py, Layer / _tolerance of
     test_conv_sweep.py): the case computes what it claims;
  5. guards intact on every buffer and every input unchanged on bits.

Swapped slots.  After recording, the op is read back through oplayout.LAYOUT: within a case the int slots the layout names (and mh_op.n) hold pairwise
different values, so do the float slots; a pair that collides must be listed in SAME_OK with its reason: 'same' = the entry point cannot express
unequal values, 'flags' = both are 0/1 flags or small enums, 'tied' = a flag or enum against a small count (a batch of 2 or 3, a 'SAME' padding of 0 .. 2
cannot avoid the values of every flag in every case).  For every pair listed as 'flags' or 'tied' the cases of the kind together hold one in which the two
differ (test_exempted_pairs_differ_in_some_case), so a swap of ANY two slots of a kind changes the arguments of at least one case.  Of the descriptor
kinds only CONV is held to this for the descriptor prefix (desc_from_op reads it for all of them); the others for their tail slots.  Counted tails
(FETCH_INPUTS): the slots in use.  Every pointer slot is non-NULL in some case of its kind, two-meaning slots under both meanings.

Worst errors of the atomic outputs against float64 (direct and replay alike; the same on the MI355X and on the CPU emulator unless two figures are given,
MI355X first): BIAS_GRAD db 5.4e-6; WARP_BWD dimg 3.6e-7 / 2.4e-7, du 1.4e-6; CORR_WARP_BWD dimg 2.7e-7, du 3.8e-7; WGRAD dw 6.3e-6, db 2.3e-6; WGRAD_PARTIAL db 2.3e-6;
WGRAD_STREAM db 0 (test_zz_report prints them, one line per kind).

No test mutates a recorded op."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import footprint as FP
from madnet_hip import _ffi, ops, oplayout, plan as PL
from oracle import tf_ops as T
from test_conv_sweep import Layer, _tolerance
from test_loss_tiles import _oracle as _loss_oracle
from test_shape_sweep import FWD, GRAD, _coords, _err, _rand, _resize_ref

EXEMPT = {
    _ffi.OP_RESERVED_25: "no entry point: the kind number is reserved",
    _ffi.OP_ALLREDUCE: "needs a communicator: test_distributed_gpu.py::test_comm_abi_single_rank replays it",
}
BF16 = torch.bfloat16
DESC_KINDS = ("CONV", "WGRAD", "WGRAD_PARTIAL", "HEAD_FWD", "CONV_PLANES", "CONV_PLANES_BWD")


def _P(g, off=0):
    return C.c_void_p(g.ptr(off))


def _shadow(x, ld=None):
    """[B,H,W,C] -> its bf16 shadow in rows of shadow_ld(C) halfs, zero padding"""
    B, H, W, Cc = x.shape
    s = torch.zeros(B, H, W, ld or ops.shadow_ld(Cc), dtype=BF16)
    s[..., :Cc] = x.to(BF16)
    return s


class Run(object):
    """the buffers and the call of one case"""

    def __init__(self, dev, lib):
        self.dev, self.lib = dev, lib
        self.ins, self.spec, self.atomic, self.oracle, self.keep = {}, {}, {}, [], []
        self.call, self.stamp = None, False

    def inp(self, name, t):
        t = t.contiguous()
        self.ins[name] = FP.Guarded(t.numel(), t.dtype, self.dev).set(t)
        return self.ins[name]

    def out(self, name, shape, dtype=torch.float32, prefill=None, sl=None, written="all", const_ok=False, zero_cols=0):
        """sl = (C, coff): the output is channels [coff, coff + C) of rows of shape[-1]; written: 'all' | 'slice' | 'acc' (prefilled everywhere, added to) |
        'any' (guards only) | 'none' (must stay untouched) | an int (the first that many elements)"""
        self.spec[name] = dict(shape=tuple(shape), dtype=dtype, prefill=prefill, sl=sl, written=("slice" if sl and written == "all" else written),
                               const_ok=const_ok, zero_cols=zero_cols)

    def fresh(self):
        o = {}
        for name, s in self.spec.items():
            g = FP.Guarded(int(np.prod(s["shape"])), s["dtype"], self.dev)
            if s["prefill"] is not None:
                if s["sl"]:
                    g.t.view(*s["shape"])[..., s["sl"][1]:s["sl"][1] + s["sl"][0]] = s["prefill"].to(self.dev)
                else:
                    g.set(s["prefill"])
            o[name] = g
        return o

    def value(self, name, g):
        s = self.spec[name]
        t = g.t.view(*s["shape"])
        if s["sl"]:
            t = t[..., s["sl"][1]:s["sl"][1] + s["sl"][0]]
        return t.cpu()

    def view(self, name, g):
        """ops.View of a [B,H,W,ld] output (its slice)"""
        s = self.spec[name]
        B, H, W, ld = s["shape"]
        Cc, coff = s["sl"] if s["sl"] else (ld, 0)
        return ops.View(g.t.view(B, H, W, ld), B, H, W, Cc, ld, coff=coff)


CASES = []          # (kind name, form, builder(run))


def case(kind, form):
    def deco(fn):
        CASES.append((kind, form, fn))
        return fn
    return deco


# ---- elementwise glue ---------------------------------------------------------------------------------------------------------------------------------
@case("FILL", "n=301")
def _(r):
    r.out("p", (301,), const_ok=True)
    r.call = lambda t, o: t.fill(_P(o["p"]), 301, 1.25, None)
    r.oracle.append(("p", lambda: torch.full((301,), 1.25, dtype=torch.float64), 0.0, 0.0))


def _f(v):
    return float(np.float32(v))


@case("MOMENTUM", "n=1027")
def _(r):
    n, lr, mom, gs = 1027, 1e-2, 0.9, 0.5
    w, m, g = _rand((n,), 1), _rand((n,), 2), _rand((n,), 3)
    gi = r.inp("grad", g)
    r.out("var", (n,), prefill=w, written="acc"); r.out("accum", (n,), prefill=m, written="acc")
    r.call = lambda t, o: t.momentum(_P(o["var"]), _P(o["accum"]), _P(gi), n, lr, mom, gs, None)
    m_ref = _f(mom) * m.double() + _f(gs) * g.double()
    r.oracle += [("accum", lambda: m_ref, 1e-6, 0.0), ("var", lambda: w.double() - _f(lr) * m_ref, 1e-6, 0.0)]


@case("ADAM", "n=1029")
def _(r):
    n, lr, b1, b2, eps, gs = 1029, 1e-3, 0.9, 0.999, 1e-8, 0.5
    w, m, v, g = _rand((n,), 5), _rand((n,), 6, 0.1), _rand((n,), 7, 0.1).abs(), _rand((n,), 8, 0.3)
    state = torch.tensor([0.9 ** 3, 0.999 ** 3], dtype=torch.float32)
    gi, si = r.inp("grad", g), r.inp("state", state)
    for name, t in (("var", w), ("m", m), ("v", v)):
        r.out(name, (n,), prefill=t, written="acc")
    r.call = lambda t, o: t.adam(_P(o["var"]), _P(o["m"]), _P(o["v"]), _P(gi), n, _P(si), lr, b1, b2, eps, gs, None)
    gd = _f(gs) * g.double()
    m_ref, v_ref = _f(b1) * m.double() + (1.0 - _f(b1)) * gd, _f(b2) * v.double() + (1.0 - _f(b2)) * gd ** 2
    lr_t = _f(lr) * np.sqrt(1.0 - float(state[1])) / (1.0 - float(state[0]))
    r.oracle += [("m", lambda: m_ref, 1e-6, 0.0), ("v", lambda: v_ref, 1e-6, 0.0), ("var", lambda: w.double() - lr_t * m_ref / (v_ref.sqrt() + _f(eps)), 1e-6, 0.0)]


@case("ADAM_ADVANCE", "state")
def _(r):
    state = torch.tensor([0.9 ** 3, 0.999 ** 3], dtype=torch.float32)
    r.out("state", (2,), prefill=state, written="acc")
    r.call = lambda t, o: t.adam_advance(_P(o["state"]), 0.9, 0.999, None)
    r.oracle.append(("state", lambda: state.double() * torch.tensor([_f(0.9), _f(0.999)], dtype=torch.float64), 1e-6, 0.0))


def _copy_ch(acc):
    def build(r):
        n = 37
        src, old = _rand((n, 5), 9), _rand((1, 1, n, 3), 10)
        si = r.inp("src", src)
        r.out("dst", (1, 1, n, 7), prefill=(old if acc else None), sl=(3, 2))
        r.call = lambda t, o: t.copy_channels(_P(si, 1), 5, _P(o["dst"], 2), 7, n, 3, 2.5, acc, None)
        r.oracle.append(("dst", lambda: (2.5 * src.double()[:, 1:4] + (old.double()[0, 0] if acc else 0)).view(1, 1, n, 3), 1e-6, 0.0))
    return build


case("COPY_CH", "accumulate=0")(_copy_ch(0))
case("COPY_CH", "accumulate=1")(_copy_ch(1))


@case("LEAKY_BWD", "slices")
def _(r):
    n = 41
    dy, y = _rand((1, 1, n, 3), 11), _rand((n, 5), 12)
    y[0, 1] = 0.0
    yi = r.inp("y", y)
    r.out("dy", (1, 1, n, 7), prefill=dy, sl=(3, 2))
    r.call = lambda t, o: t.leaky_bwd(_P(o["dy"], 2), 7, _P(yi, 1), 5, n, 3, 0.2, None)
    r.oracle.append(("dy", lambda: (dy[0, 0] * torch.where(y[:, 1:4] > 0, torch.tensor(1.0), torch.tensor(0.2))).double().view(1, 1, n, 3), 0.0, 0.0))


@case("BIAS_GRAD", "atomic")
def _(r):
    npix, nch, ld = 777, 8, 12
    dz, db0 = _rand((npix, ld), 31), _rand((nch,), 32)
    zi = r.inp("dz", dz)
    r.out("db", (nch,), prefill=db0, written="acc")
    r.call = lambda t, o: t.bias_grad(_P(zi), ld, npix, nch, _P(o["db"]), None)
    r.atomic["db"] = (lambda: db0.double() + dz.double()[:, :nch].sum(0), 1e-5, 0.0)


@case("BIAS_GRAD", "partial")
def _(r):
    npix, nch, ld = 777, 8, 12
    dz = _rand((npix, ld), 31)
    zi = r.inp("dz", dz)
    nb = int(r.lib.bias_grad_blocks(npix, nch))
    r.out("ws", (nb, nch))
    r.call = lambda t, o: t.bias_grad_partial(_P(zi), ld, npix, nch, _P(o["ws"]), nb, None)
    r.oracle.append(("ws", lambda: dz.double()[:, :nch].sum(0), 1e-5, 0.0, lambda v: v.double().sum(0)))


@case("DET_FLUSH", "n=77")
def _(r):
    n = 77
    old = _rand((n,), 41)
    add = torch.round(_rand((n,), 42) * 1024) / 1024
    twin = (add.double() * 2.0 ** 48).to(torch.int64)
    r.out("dst", (n,), prefill=old, written="acc"); r.out("twin", (n,), dtype=torch.int64, prefill=twin, written="acc", const_ok=True)
    r.call = lambda t, o: t.det_flush(_P(o["dst"]), _P(o["twin"]), n, None)
    r.oracle += [("dst", lambda: old.double() + add.double(), 1e-6, 0.0), ("twin", lambda: torch.zeros(n, dtype=torch.float64), 0.0, 0.0)]


@case("STAMP", "slot")
def _(r):
    r.out("slot", (1,), dtype=torch.int64, const_ok=True)
    r.stamp = True
    r.call = lambda t, o: t.stamp(_P(o["slot"]), None)


def _fetch(n):
    def build(r):
        table = ops.InputTable(r.lib, r.dev)
        r.keep.append(table)
        sizes = [33, 1025, 257, 64][:n]
        srcs = []
        for k, sz in enumerate(sizes):
            if k % 2 == 0:
                s = torch.randint(0, 256, (sz,), generator=torch.Generator().manual_seed(50 + k), dtype=torch.uint8)
            else:
                s = _rand((sz,), 50 + k)
            gi = r.inp("src%d" % k, s)
            table.tab.src[k], table.tab.u8[k] = gi.ptr(), int(s.dtype == torch.uint8)
            srcs.append(s)
            r.out("dst%d" % k, (sz,))
            r.oracle.append(("dst%d" % k, (lambda s=s: s.double()), 0.0, 0.0))

        def call(t, o):
            dp = (C.c_void_p * n)(*[o["dst%d" % k].ptr() for k in range(n)])
            cnt = (C.c_int64 * n)(*sizes)
            t.fetch_inputs(C.c_void_p(table.ptr), dp, cnt, n, None)
        r.call = call
    return build


case("FETCH_INPUTS", "1 entry")(_fetch(1))
case("FETCH_INPUTS", "%d entries" % _ffi.FETCH_MAX)(_fetch(_ffi.FETCH_MAX))


# ---- warp, resize, pad ---------------------------------------------------------------------------------------------------------------------------------
@case("WARP_FWD", "slice")
def _(r):
    B, H, W, Cc = 2, 5, 9, 16
    img, u = _rand((B, H, W, Cc), 20), _coords(B, H, W, 120, -6.0, 6.0)
    ii, ui = r.inp("img", FP.wide_rows(img, 20, "cpu")), r.inp("u", u)
    r.out("out", (B, H, W, 24), sl=(Cc, 4))
    r.call = lambda t, o: t.warp_fwd(_P(ii), 20, _P(ui), _P(o["out"], 4), 24, B, H, W, Cc, None)
    r.oracle.append(("out", lambda: T.linear_warp(img.double(), u.double()[..., None]), FWD, 2e-6))


def _warp_bwd(acc_u):
    def build(r):
        B, H, W, Cc = 2, 5, 9, 16
        img, u, g = _rand((B, H, W, Cc), 20), _coords(B, H, W, 120, -6.0, 6.0), _rand((B, H, W, Cc), 220)
        oldi, oldu = _rand((B, H, W, Cc), 320), _rand((B, H, W), 420)
        gi_, ii, ui = r.inp("g", FP.wide_rows(g, 28, "cpu")), r.inp("img", FP.wide_rows(img, 20, "cpu")), r.inp("u", u)
        r.out("dimg", (B, H, W, 24), prefill=oldi, sl=(Cc, 4)); r.out("du", (B, H, W), prefill=(oldu if acc_u else None), written=("acc" if acc_u else "all"))
        r.call = lambda t, o: t.warp_bwd(_P(gi_), 28, _P(ii), 20, _P(ui), _P(o["dimg"], 4), 24, _P(o["du"]), acc_u, B, H, W, Cc, None)

        def refs():
            ic, uc = img.double().requires_grad_(True), u.double()[..., None].requires_grad_(True)
            return torch.autograd.grad(T.linear_warp(ic, uc), [ic, uc], g.double())
        r.atomic["dimg"] = (lambda: refs()[0] + oldi.double(), GRAD, 2e-6)
        r.atomic["du"] = (lambda: refs()[1][..., 0] + (oldu.double() if acc_u else 0), GRAD, 2e-5)
    return build


case("WARP_BWD", "acc_u=1")(_warp_bwd(1))
case("WARP_BWD", "acc_u=0")(_warp_bwd(0))

RESIZE = dict(B=2, Hi=5, Wi=7, Hr=11, Wr=13, cy=3, cx=4, Ho=6, Wo=8)


def _resize_input(mode, mul):
    g = RESIZE
    for attempt in range(20):             # (no pre-activation near the relu's kink: test_shape_sweep.py)
        x = _rand((g["B"], g["Hi"], g["Wi"]), 1000 + attempt)
        _, pre = _resize_ref(x.double(), g["Hr"], g["Wr"], g["cy"], g["cx"], g["Ho"], g["Wo"], mul, mode)
        if pre is None or bool((pre.abs() >= 1e-4).all()):
            return x
    raise AssertionError("no unambiguous input")


def _resize_fwd(mode):
    def build(r):
        g, mul = RESIZE, -1.5
        x = _resize_input(mode, mul)
        xi = r.inp("x", x)
        r.out("out", (g["B"], g["Ho"], g["Wo"]))
        r.call = lambda t, o: t.resize_fwd(_P(xi), _P(o["out"]), g["B"], g["Hi"], g["Wi"], g["Hr"], g["Wr"], g["cy"], g["cx"], g["Ho"], g["Wo"], mul, mode, None)
        r.oracle.append(("out", lambda: _resize_ref(x.double(), g["Hr"], g["Wr"], g["cy"], g["cx"], g["Ho"], g["Wo"], mul, mode)[0], FWD, 2e-6))
    return build


case("RESIZE_FWD", "mode=0")(_resize_fwd(0))
case("RESIZE_FWD", "mode=1")(_resize_fwd(1))


def _resize_bwd(mode, acc):
    def build(r):
        g, mul = RESIZE, -1.5
        x = _resize_input(mode, mul)
        gr, old = _rand((g["B"], g["Ho"], g["Wo"]), 3000), _rand((g["B"], g["Hi"], g["Wi"]), 5000)
        xi, gi = r.inp("x", x), r.inp("g", gr)
        r.out("din", (g["B"], g["Hi"], g["Wi"]), prefill=(old if acc else None), written=("acc" if acc else "all"))
        r.call = lambda t, o: t.resize_bwd(_P(gi), _P(xi), _P(o["din"]), acc, g["B"], g["Hi"], g["Wi"], g["Hr"], g["Wr"], g["cy"], g["cx"], g["Ho"], g["Wo"], mul, mode, None)

        def ref():
            xc = x.double().requires_grad_(True)
            out, _ = _resize_ref(xc, g["Hr"], g["Wr"], g["cy"], g["cx"], g["Ho"], g["Wo"], mul, mode)
            return torch.autograd.grad(out, [xc], gr.double())[0] + (old.double() if acc else 0)
        r.oracle.append(("din", ref, GRAD, 1e-5))
    return build


case("RESIZE_BWD", "mode=1 accumulate=0")(_resize_bwd(1, 0))
case("RESIZE_BWD", "mode=0 accumulate=1")(_resize_bwd(0, 1))


@case("RESIZE_IMAGE", "2x5x7x3 -> 9x11")
def _(r):
    B, Hi, Wi, Cc, Ho, Wo = 2, 5, 7, 3, 9, 11
    x = _rand((B, Hi, Wi, Cc), 100)
    xi = r.inp("x", x)
    r.out("out", (B, Ho, Wo, Cc))
    r.call = lambda t, o: t.resize_image_fwd(_P(xi), _P(o["out"]), B, Hi, Wi, Cc, Ho, Wo, None)
    r.oracle.append(("out", lambda: T.resize_bilinear(x.double(), Ho, Wo), FWD, 2e-6))


@case("PAD_REFLECT", "div, sub")
def _(r):
    B, H, W, Cc, Hp, Wp, pt, pl, ld, div, sub = 2, 5, 7, 3, 11, 15, 4, 6, 8, 255.0, 100.0 / 255.0
    x = torch.floor(torch.rand(B, H, W, Cc, generator=torch.Generator().manual_seed(40)) * 256)
    xi = r.inp("x", x)
    r.out("out", (B, Hp, Wp, ld))
    r.call = lambda t, o: t.pad_reflect(_P(xi), _P(o["out"]), B, H, W, Cc, Hp, Wp, pt, pl, ld, div, sub, None)

    def ref():
        refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
        iy, ix = refl(np.arange(Hp) - pt, H), refl(np.arange(Wp) - pl, W)
        return x.double()[:, iy][:, :, ix] / _f(div) - _f(sub)
    r.oracle.append(("out", ref, 1e-6, 0.0, lambda v: v[..., :Cc]))


# ---- losses and metrics: the workspace and the result vector are outputs like any other --------------------------------------------------------------
LB, LH, LW = 2, 9, 14


def _loss(phase):
    def build(r):
        left = torch.floor(torch.rand(LB, LH, LW, 3, generator=torch.Generator().manual_seed(61)) * 256)
        right = torch.floor(torch.rand(LB, LH, LW, 3, generator=torch.Generator().manual_seed(62)) * 256)
        disp = torch.rand(LB, LH, LW, generator=torch.Generator().manual_seed(63)) * 3.0
        li, ri, di = r.inp("left", left), r.inp("right", right), r.inp("disp", disp)
        nws = int(r.lib.loss_ws_floats(LB, LH, LW))
        ws0 = None
        if phase == 2:            # the partial sums phase 1 left: an input of phase 2 (and bit-equal in both output sets)
            ws, res, dd = torch.zeros(nws, device=r.dev), torch.zeros(4, device=r.dev), torch.zeros(LB, LH, LW, device=r.dev)
            r.lib.reprojection_loss_phase(_P(li), _P(ri), _P(di), ops._p(ws), ops._p(res), ops._p(dd), 0.75, LB, LH, LW, 1, None)
            ws0 = ws.cpu()
        r.out("ws", (nws,), prefill=ws0, written="any"); r.out("result", (4,), written="any", const_ok=True)
        r.out("ddisp", (LB, LH, LW), written=("any" if phase == 2 else "all"))
        r.call = lambda t, o: t.reprojection_loss_phase(_P(li), _P(ri), _P(di), _P(o["ws"]), _P(o["result"]), _P(o["ddisp"]), 0.75, LB, LH, LW, phase, None)
        if phase == 0:          # (loss, mean SSIM term, mean L1 term): the oracle and the bound of test_loss_tiles.py::test_loss_values
            r.oracle.append(("result", lambda: torch.tensor(_loss_oracle(disp, left, right, torch.float64)[:3], dtype=torch.float64), 2e-6, 0.0, lambda v: v[:3]))
    return build


for _ph in (0, 1, 2):
    case("LOSS", "phase=%d" % _ph)(_loss(_ph))


def _l1_inputs(r, hi):
    pred = torch.rand(LB, LH, LW, generator=torch.Generator().manual_seed(71)) * 40.0
    tgt = torch.rand(LB, LH, LW, generator=torch.Generator().manual_seed(72)) * 40.0
    tgt[0, 0, :5] = 0.0
    tgt[1, 2, :3] = hi
    return pred, tgt, r.inp("pred", pred), r.inp("target", tgt)


def _masked_l1_ref(p, t, valid, weight):
    return weight * ((p.double() - t.double()).abs() * valid).sum() / valid.sum()


@case("PROXY_LOSS", "with gradient")
def _(r):
    pred, tgt, pi, ti = _l1_inputs(r, 200.0)
    r.out("ws", (int(r.lib.proxy_ws_floats(LB, LH, LW)),), written="any"); r.out("result", (4,), written="any", const_ok=True); r.out("dpred", (LB, LH, LW))
    r.call = lambda t, o: t.proxy_loss(_P(pi), _P(ti), _P(o["ws"]), _P(o["result"]), _P(o["dpred"]), 0.01, 0.75, LB, LH, LW, None)
    r.oracle.append(("result", lambda: _masked_l1_ref(pred, tgt, ~((tgt <= 0) | (tgt >= 192)), _f(0.01)).view(1), 1e-5, 0.0, lambda v: v[:1]))


@case("PROXY_LOSS_SCALED", "scale=3")
def _(r):
    B, H, W, scale = 2, 9, 15, 3
    pred = torch.rand(B, H, W, generator=torch.Generator().manual_seed(73)) * 40.0
    tgt = torch.rand(B, H, W, generator=torch.Generator().manual_seed(74)) * 40.0 + 1.0
    pi, ti = r.inp("pred", pred), r.inp("proxy", tgt)
    r.out("ws", (int(r.lib.proxy_scaled_ws_floats(B, H, W, scale)),), written="any"); r.out("result", (4,), written="any", const_ok=True); r.out("dpred", (B, H, W))
    r.call = lambda t, o: t.proxy_loss_scaled(_P(pi), _P(ti), _P(o["ws"]), _P(o["result"]), _P(o["dpred"]), 0.1, 0.75, scale, B, H, W, None)

    def ref():
        p = T.resize_bilinear(pred.double()[..., None], H // scale, W // scale)[..., 0]
        q = T.resize_bilinear(tgt.double()[..., None], H // scale, W // scale)[..., 0] / scale
        return _masked_l1_ref(p, q, ~((q <= 0) | (q >= 192)), _f(0.1)).view(1)
    r.oracle.append(("result", ref, 1e-5, 0.0, lambda v: v[:1]))


@case("SUPERVISED_LOSS", "max_disp=35")
def _(r):
    pred, tgt, pi, ti = _l1_inputs(r, 36.0)
    r.out("ws", (int(r.lib.proxy_ws_floats(LB, LH, LW)),), written="any"); r.out("result", (4,), written="any", const_ok=True); r.out("dpred", (LB, LH, LW))
    r.call = lambda t, o: t.supervised_loss(_P(pi), _P(ti), _P(o["ws"]), _P(o["result"]), _P(o["dpred"]), 1.25, 0.75, 35.0, LB, LH, LW, None)
    r.oracle.append(("result", lambda: _masked_l1_ref(pred, tgt, ~((tgt == 0) | (tgt >= 35.0)), 1.25).view(1), 1e-5, 0.0, lambda v: v[:1]))


@case("METRICS", "th=2.5")
def _(r):
    pred, tgt, pi, ti = _l1_inputs(r, 200.0)
    r.out("ws", (int(r.lib.metrics_ws_floats(LB, LH, LW)),), written="any"); r.out("result", (4,), written="any", const_ok=True)
    r.call = lambda t, o: t.metrics(_P(pi), _P(ti), _P(o["ws"]), _P(o["result"]), 2.5, LB, LH, LW, None)

    def ref():
        valid = tgt != 0
        d = (pred.double() - tgt.double()).abs() * valid
        return torch.stack([d.sum() / valid.sum(), (d > 2.5).sum() / valid.sum().double(), valid.sum().double()])
    r.oracle.append(("result", ref, 1e-5, 0.0, lambda v: v[:3]))


@case("METRICS_KITTI", "report")
def _(r):
    pred, tgt, pi, ti = _l1_inputs(r, 200.0)
    r.out("ws", (int(r.lib.metrics_kitti_ws_floats(LB, LH, LW)),), written="any"); r.out("result", (4,), written="any", const_ok=True)
    r.call = lambda t, o: t.metrics_kitti(_P(pi), _P(ti), _P(o["ws"]), _P(o["result"]), LB, LH, LW, None)

    def ref():
        val = tgt > 0
        diff = (tgt.double() - pred.double()).abs()
        d1 = ((diff > 3) & (diff / tgt.double().clamp(min=1e-30) >= 0.05) & val).sum().double() / val.sum() * 100.0
        return torch.stack([(diff * val).sum() / val.sum(), d1, val.sum().double()])
    r.oracle.append(("result", ref, 1e-5, 0.0, lambda v: v[:3]))


# ---- correlation ---------------------------------------------------------------------------------------------------------------------------------------
def _corr_fwd(prec, copy_left, zero_tail, Cc=16, md=3, stride=1):
    def build(r):
        B, H, W = 2, 5, 21
        D = 2 * md // stride + 1
        L, R, u = _rand((B, H, W, Cc), 10), _rand((B, H, W, Cc), 110), _rand((B, H, W), 210)
        l_ld, r_ld = Cc + 4, Cc + 8
        li, ri, ui = r.inp("L", FP.wide_rows(L, l_ld, "cpu")), r.inp("R", FP.wide_rows(R, r_ld, "cpu")), r.inp("u", u)
        if copy_left:
            coff, out_ld = Cc + 40, FP.round_up(Cc + 40 + D + 1, 4) + 12
            r.out("out", (B, H, W, out_ld), written="any")
        else:
            coff, out_ld = 12, FP.round_up(12 + D, 4) + 16
            r.out("out", (B, H, W, out_ld), sl=(D, coff))
        base = 0 if copy_left else coff
        r.call = lambda t, o: t.corr_fwd_prec(_P(li), l_ld, _P(ri), r_ld, (_P(ui) if copy_left else None), _P(o["out"], base), out_ld, (coff if copy_left else 0),
                                               B, H, W, Cc, md, stride, copy_left, zero_tail, prec, None)
        r.oracle.append(("out", lambda: T.correlation(L.double(), R.double(), md, stride), FWD, 2e-6, (lambda v: v[..., Cc + 40:Cc + 40 + D]) if copy_left else None))
    return build


# each precision the entry accepts; the concat form with the tail zero-filled and left alone; stride 2
case("CORR_FWD", "precision=0 volume")(_corr_fwd(0, 0, 0))
case("CORR_FWD", "precision=1 concat zero_tail")(_corr_fwd(1, 1, 1))
case("CORR_FWD", "precision=2 concat")(_corr_fwd(2, 1, 0, Cc=24, md=4, stride=2))


def _corr_bwd(prec, copy_left, acc_l, acc_r, acc_u, Cc=16, md=3, stride=1):
    def build(r):
        B, H, W = 2, 5, 21
        D = 2 * md // stride + 1
        coff = Cc + 40 if copy_left else 4
        g_ld = FP.round_up(coff + D + 1, 4) + 28
        L, R, g = _rand((B, H, W, Cc), 10), _rand((B, H, W, Cc), 110), _rand((B, H, W, g_ld), 310)
        oldl, oldr, oldu = _rand((B, H, W, Cc), 410), _rand((B, H, W, Cc), 411), _rand((B, H, W), 412)
        l_ld, r_ld, dl_ld, dr_ld = Cc + 4, Cc + 8, Cc + 12, Cc + 16
        gi, li, ri = r.inp("g", g), r.inp("L", FP.wide_rows(L, l_ld, "cpu")), r.inp("R", FP.wide_rows(R, r_ld, "cpu"))
        r.out("dL", (B, H, W, dl_ld), prefill=(oldl if acc_l else None), sl=(Cc, 4)); r.out("dR", (B, H, W, dr_ld), prefill=(oldr if acc_r else None), sl=(Cc, 8))
        r.out("du", (B, H, W), prefill=(oldu if acc_u else None), written=("acc" if acc_u else "all") if copy_left else "none")
        r.call = lambda t, o: t.corr_bwd_prec(_P(gi), g_ld, coff, _P(li), l_ld, _P(ri), r_ld, _P(o["dL"], 4), dl_ld, acc_l, _P(o["dR"], 8), dr_ld, acc_r,
                                               (_P(o["du"]) if copy_left else None), acc_u, B, H, W, Cc, md, stride, copy_left, prec, None)

        def refs():
            Lc, Rc = L.double().requires_grad_(True), R.double().requires_grad_(True)
            return torch.autograd.grad(T.correlation(Lc, Rc, md, stride), [Lc, Rc], g.double()[..., coff:coff + D])
        r.oracle += [("dL", lambda: refs()[0] + (g.double()[..., :Cc] if copy_left else 0) + (oldl.double() if acc_l else 0), GRAD, 2e-6),
                     ("dR", lambda: refs()[1] + (oldr.double() if acc_r else 0), GRAD, 2e-6)]
    return build


case("CORR_BWD", "precision=0 acc_l")(_corr_bwd(0, 0, 1, 0, 0))
case("CORR_BWD", "precision=1 copy_left acc_r")(_corr_bwd(1, 1, 0, 1, 0))
case("CORR_BWD", "precision=2 copy_left acc_u stride 2")(_corr_bwd(2, 1, 0, 0, 1, Cc=24, md=4, stride=2))


def _corr_warp_bwd(copy_left, acc_l, acc_img, md=3, stride=1):
    def build(r):
        B, H, W, Cc = 2, 5, 21, 16
        D = 2 * md // stride + 1
        coff = Cc + 40 if copy_left else 8
        g_ld = FP.round_up(coff + D + 1, 4) + 32
        img, L, u, g = _rand((B, H, W, Cc), 7000), _rand((B, H, W, Cc), 7001), _coords(B, H, W, 7002, -6.0, 6.0), _rand((B, H, W, g_ld), 7005)
        oldl, oldi = _rand((B, H, W, Cc), 7003), _rand((B, H, W, Cc), 7004)
        ic, uc = img.double().requires_grad_(True), u.double()[..., None].requires_grad_(True)
        Rw64 = T.linear_warp(ic, uc)
        Rw = Rw64.detach().float()
        l_ld, rw_ld, img_ld, dl_ld, dimg_ld = Cc + 4, Cc + 8, Cc + 12, Cc + 16, Cc + 20
        gi, li, wi, ii, ui = (r.inp("g", g), r.inp("L", FP.wide_rows(L, l_ld, "cpu")), r.inp("Rw", FP.wide_rows(Rw, rw_ld, "cpu")),
                              r.inp("img", FP.wide_rows(img, img_ld, "cpu")), r.inp("u", u))
        r.out("dL", (B, H, W, dl_ld), prefill=(oldl if acc_l else None), sl=(Cc, 4)); r.out("dimg", (B, H, W, dimg_ld), prefill=(oldi if acc_img else None), sl=(Cc, 8))
        r.out("du", (B, H, W))
        r.call = lambda t, o: t.corr_warp_bwd(_P(gi), g_ld, coff, _P(li), l_ld, _P(wi), rw_ld, _P(ii), img_ld, _P(ui), _P(o["dL"], 4), dl_ld, acc_l | (0 if acc_img else 2),
                                               _P(o["dimg"], 8), dimg_ld, _P(o["du"]), B, H, W, Cc, md, stride, copy_left, None)

        def refs():
            Lc, Rl = L.double().requires_grad_(True), Rw.double().requires_grad_(True)
            gl, grw = torch.autograd.grad(T.correlation(Lc, Rl, md, stride), [Lc, Rl], g.double()[..., coff:coff + D])
            gim, gu = torch.autograd.grad(Rw64, [ic, uc], grw, retain_graph=True)
            return gl + (g.double()[..., :Cc] if copy_left else 0), gim, g.double()[..., coff + D] + gu[..., 0]
        r.oracle.append(("dL", lambda: refs()[0] + (oldl.double() if acc_l else 0), GRAD, 2e-6))
        r.atomic["dimg"] = (lambda: refs()[1] + (oldi.double() if acc_img else 0), GRAD, 2e-6)
        r.atomic["du"] = (lambda: refs()[2], GRAD, 2e-6)
    return build


case("CORR_WARP_BWD", "copy_left acc_img")(_corr_warp_bwd(1, 0, 1))
case("CORR_WARP_BWD", "acc_l overwrite dimg stride 2")(_corr_warp_bwd(0, 1, 0, md=4, stride=2))


def _level_front(form):
    """form: 'plain' | 'planes' | 'head'"""
    def build(r):
        B, H, W, Cc, md, K = 2, 6, 22, 16, 3, 8
        Hc, Wc = (4, 11) if form == "head" else (5, 9)
        D = 2 * md + 1
        coff = Cc + 4 if form == "plain" else Cc          # (the engines' form is coff = C: one case unties the two)
        n = coff + D + 1
        out_ld, pld = FP.round_up(n, 4) + 12, FP.round_up(n, 32) + 32
        l_ld, r_ld, rw_ld, x_ld = Cc + 8, Cc + 12, Cc + 28, K + 4
        L, R, Vc = _rand((B, H, W, Cc), 9000), _rand((B, H, W, Cc), 9001), _rand((B, Hc, Wc), 9002, 1.5)
        li, ri = r.inp("L", FP.wide_rows(L, l_ld, "cpu")), r.inp("R", FP.wide_rows(R, r_ld, "cpu"))
        zero_tail = 1 if form != "planes" else 0
        r.out("out", (B, H, W, out_ld), written="any"); r.out("Rw", (B, H, W, rw_ld), sl=(Cc, 0)); r.out("u", (B, H, W))
        if form != "plain":
            r.out("hi", (B, H, W, pld), dtype=BF16, written="any"); r.out("lo", (B, H, W, pld), dtype=BF16, written="any")
        common = lambda o: (2.5, _P(li), l_ld, _P(ri), r_ld, _P(o["out"]), out_ld, coff, _P(o["Rw"]), rw_ld, _P(o["u"]), B, H, W, Cc, md, zero_tail)
        if form == "plain":
            vi = r.inp("Vc", Vc)
            r.call = lambda t, o: t.level_front_fwd(_P(vi), Hc, Wc, *(common(o) + (None,)))
        elif form == "planes":
            vi = r.inp("Vc", Vc)
            r.call = lambda t, o: t.level_front_fwd_planes(_P(vi), Hc, Wc, *(common(o) + (_P(o["hi"]), _P(o["lo"]), pld, None)))
        else:
            assert r.lib.level_front_head_ok(Hc, Wc, H, W, Cc, K, md) == 1
            X, hw, hb = _rand((B, Hc, Wc, K), 9003), _rand((3, 3, K, 1), 9004, 0.2), _rand((1,), 9005)
            xi, wi, bi = r.inp("X", FP.wide_rows(X, x_ld, "cpu")), r.inp("hw", hw), r.inp("hb", hb)
            r.out("Vc", (B, Hc, Wc))
            r.call = lambda t, o: t.level_front_head_fwd(_P(xi), x_ld, K, _P(wi), _P(bi), _P(o["Vc"]), Hc, Wc, *(common(o) + (_P(o["hi"]), _P(o["lo"]), pld, None)))
            r.oracle.append(("Vc", lambda: T.conv2d(X.double(), hw.double(), hb.double(), 1, 1, 1.0)[..., 0], FWD, 2e-6))
        if form != "head":
            r.oracle.append(("u", lambda: 2.5 * T.resize_bilinear(Vc.double()[..., None], H, W)[..., 0], FWD, 2e-6))
    return build


for _form in ("plain", "planes", "head"):
    case("LEVEL_FRONT", _form)(_level_front(_form))


# ---- the conv family ---------------------------------------------------------------------------------------------------------------------------------
def _bank(r, w, planes, trans):
    """the fragment bank of w, packed once by the library (an input of the case)"""
    bank = torch.zeros(ops.pack_bytes(w, planes, trans) // 4, device=r.dev)
    ops.pack_weights(r.lib, [(w.to(r.dev), bank, planes, trans)], r.dev, r.keep)
    if r.dev != "cpu":
        torch.cuda.synchronize()
    return r.inp("bank", bank.cpu())


CONV_LAYERS = {          # form -> (seed, B, H, W, Ci, Co, k, stride, dil): H even, W odd, stride 2 without dilation (Hi != Ho, Wi != Wo, pad_t != pad_l); one dilated
    "fwd": (31000, 3, 8, 11, 12, 16, 5, 2, 1),
    "dgrad": (31010, 3, 13, 15, 20, 16, 5, 2, 1),          # (H odd: pad_t = 2 != dil)
    "dil": (31020, 2, 9, 14, 12, 16, 3, 1, 2),
}
_layers = {}


def _layer(key):
    if key not in _layers:
        _layers[key] = Layer(*CONV_LAYERS[key])
    return _layers[key]


def _conv(form, lkey, mode, prec, bias=False, alpha=1.0, mask=None, acc=False, sh_in=False, sh_mask=False, only=False):
    """form: conv2d | wb | sh | sh2 | sh3 | sh4"""
    def build(r):
        L = _layer(lkey)
        K, N = (L.Ci, L.Co) if mode == 0 else (L.Co, L.Ci)
        Hi, Wi, Ho, Wo = (L.H, L.W, L.Ho, L.Wo) if mode == 0 else (L.Ho, L.Wo, L.H, L.W)
        src = L.x if mode == 0 else L.dz
        in_ld, coff, out_ld, mask_ld = K + 8, 4, N + 20, N + 24
        xi, wi = r.inp("x", FP.wide_rows(src, in_ld, "cpu")), r.inp("w", L.w)
        bi = r.inp("bias", L.bias[mode]) if bias else None
        mi = r.inp("mask", FP.wide_rows(L.mask[mode], mask_ld, "cpu", fill=0.0)) if mask is not None else None
        c0, c1 = mask if mask is not None else (0, 0)
        d = ops.conv_desc(L.B, Hi, Wi, Ho, Wo, K, N, L.k, L.k, L.stride, L.dil, L.pt, L.pl, mode, mode, in_ld, out_ld, mask_ld=(mask_ld if mask is not None else 0),
                          accumulate=int(acc), alpha=alpha, mask_alpha=0.3, mask_c0=c0, mask_c1=c1, precision=prec)
        r.keep.append(d)
        r.out("out", (L.B, Ho, Wo, out_ld), prefill=(L.old[mode] if acc else None), sl=(N, coff), written=("any" if only else "all"))
        bank = None
        if form != "conv2d":
            bank = _bank(r, L.w, 2 if (prec == 2 and mode == 0) else 1, mode)
        sld = ops.shadow_ld(N)
        if form in ("sh", "sh2", "sh3", "sh4"):
            r.out("shadow", (L.B, Ho, Wo, sld), dtype=BF16, written="any")
        if form == "sh4":
            r.out("lo", (L.B, Ho, Wo, sld), dtype=BF16, written="any")
        ish = r.inp("in_shadow", _shadow(src)) if (form == "sh2" or sh_in) else None
        msh = r.inp("mask_shadow", _shadow(L.mask[mode])) if sh_mask else None
        P_ = lambda g: (_P(g) if g is not None else None)

        def call(t, o):
            out = _P(o["out"], coff)
            if form == "conv2d":
                t.conv2d(C.byref(d), _P(xi), _P(wi), P_(bi), out, P_(mi), None)
            elif form == "wb":
                t.conv2d_wb(C.byref(d), _P(xi), _P(wi), _P(bank), P_(bi), out, P_(mi), None)
            elif form == "sh":
                t.conv2d_sh(C.byref(d), _P(xi), _P(wi), _P(bank), P_(bi), out, P_(mi), _P(o["shadow"]), None)
            elif form == "sh2":
                t.conv2d_sh2(C.byref(d), _P(xi), _P(ish), _P(wi), _P(bank), P_(bi), out, P_(mi), _P(o["shadow"]), None)
            elif form == "sh3":
                t.conv2d_sh3(C.byref(d), _P(xi), P_(ish), _P(wi), _P(bank), None, out, P_(mi), P_(msh), _P(o["shadow"]), int(only), None)
            else:
                t.conv2d_sh4(C.byref(d), _P(xi), _P(wi), _P(bank), P_(bi), out, P_(mi), _P(o["shadow"]), _P(o["lo"]), None)
        r.call = call
        if not only:
            r.oracle.append(("out", ("conv", L, mode, bias, alpha, mask, acc), None, None))
    return build


case("CONV", "conv2d fwd bias mask acc")(_conv("conv2d", "fwd", 0, 0, bias=True, alpha=0.2, mask=(7, 13), acc=True))
case("CONV", "conv2d_wb bf16x3")(_conv("wb", "dil", 0, 2, bias=True, alpha=0.2))
case("CONV", "conv2d_sh fwd bf16")(_conv("sh", "fwd", 0, 1, bias=True, mask=(7, 13), acc=True))
case("CONV", "conv2d_sh2 dgrad")(_conv("sh2", "dgrad", 1, 1, mask=(9, 14), acc=True))
case("CONV", "conv2d_sh3 mask shadow")(_conv("sh3", "dgrad", 1, 1, mask=(9, 14), sh_mask=True))
case("CONV", "conv2d_sh3 in + mask shadow acc")(_conv("sh3", "dgrad", 1, 1, mask=(9, 14), acc=True, sh_in=True, sh_mask=True))
case("CONV", "conv2d_sh3 shadow only")(_conv("sh3", "dil", 1, 1, mask=(7, 11), only=True))
case("CONV", "conv2d_sh3 in shadow, shadow only")(_conv("sh3", "dgrad", 1, 1, sh_in=True, only=True))
case("CONV", "conv2d_sh4 planes")(_conv("sh4", "fwd", 0, 2, bias=True, alpha=0.2))


@case("WGRAD", "exact fp32, atomics")
def _(r):
    L = _layer("fwd")
    xld, zld = L.Ci + 8, L.Co + 12
    xi, zi = r.inp("x", FP.wide_rows(L.x, xld, "cpu")), r.inp("dz", FP.wide_rows(L.dz, zld, "cpu"))
    d = ops.conv_desc(L.B, L.H, L.W, L.Ho, L.Wo, L.Ci, L.Co, L.k, L.k, L.stride, L.dil, L.pt, L.pl, 0, 0, xld, zld, precision=0)
    r.keep.append(d)
    r.out("dw", (L.w.numel(),), prefill=torch.zeros(L.w.numel()), written="acc"); r.out("db", (L.Co,), prefill=torch.zeros(L.Co), written="acc")
    r.call = lambda t, o: t.conv2d_wgrad(C.byref(d), _P(xi), _P(zi), zld, _P(o["dw"]), _P(o["db"]), None)
    r.atomic["dw"] = (lambda: L.wgrad_ref(False).reshape(-1), 1e-4, 0.0)
    r.atomic["db"] = (lambda: L.dz.double().sum((0, 1, 2)), 1e-4, 0.0)


def _wgrad_partial(with_ws):
    def build(r):
        L = _layer("fwd")
        xld, zld = L.Ci + 8, L.Co + 12
        xi, zi = r.inp("x", FP.wide_rows(L.x, xld, "cpu")), r.inp("dz", FP.wide_rows(L.dz, zld, "cpu"))
        d = ops.conv_desc(L.B, L.H, L.W, L.Ho, L.Wo, L.Ci, L.Co, L.k, L.k, L.stride, L.dil, L.pt, L.pl, 0, 0, xld, zld, precision=0)
        r.keep.append(d)
        sp = C.c_int32(0)
        r.lib.conv2d_wgrad_partial(C.byref(d), _P(xi), _P(zi), zld, None, C.byref(sp), None, None)
        ns, size = sp.value, L.w.numel()
        assert ns >= 1
        r.out("ws", (ns * size + (ns * L.Co if ns > 1 else 0),), written=("all" if with_ws else "none"))
        r.out("db", (L.Co,), prefill=torch.zeros(L.Co), written=("acc" if with_ws else "none"), const_ok=True)

        def call(t, o):
            n = C.c_int32(ns)
            t.conv2d_wgrad_partial(C.byref(d), _P(xi), _P(zi), zld, (_P(o["ws"]) if with_ws else None), C.byref(n), (_P(o["db"]) if with_ws else None), None)
            if not with_ws:
                assert n.value == ns            # (the query form: nothing is launched; a replay of it is a no-op as well)
        r.call = call
        if with_ws:
            r.oracle.append(("ws", lambda: L.wgrad_ref(False).reshape(-1), 1e-4, 0.0, lambda v: v[:ns * size].view(ns, size).double().sum(0)))
            if ns == 1:
                r.atomic["db"] = (lambda: L.dz.double().sum((0, 1, 2)), 1e-4, 0.0)
    return build


case("WGRAD_PARTIAL", "with workspace")(_wgrad_partial(True))
case("WGRAD_PARTIAL", "query (no workspace)")(_wgrad_partial(False))


@case("HEAD_FWD", "two extra slots")
def _(r):
    L = Layer(32000, 2, 7, 13, 20, 1, 3, 1, 1)
    in_ld = 24
    xi, wi, bi = r.inp("x", FP.wide_rows(L.x, in_ld, "cpu")), r.inp("w", L.w), r.inp("bias", L.bias[0])
    d = ops.conv_desc(L.B, L.H, L.W, L.Ho, L.Wo, L.Ci, 1, 3, 3, 1, 1, L.pt, L.pl, 0, 0, in_ld, 5)
    r.keep.append(d)
    r.out("out", (L.B, L.H, L.W, 5), sl=(1, 2)); r.out("out2", (L.B, L.H, L.W, 6), sl=(1, 3)); r.out("out3", (L.B, L.H, L.W, 9), sl=(1, 4))
    r.call = lambda t, o: t.conv2d_head(C.byref(d), _P(xi), _P(wi), _P(bi), _P(o["out"], 2), _P(o["out2"], 3), 6, _P(o["out3"], 4), 9, None)
    for name in ("out", "out2", "out3"):
        r.oracle.append((name, lambda: L.expected(0, False, True, 1.0, None, False), 2e-5, 0.0))


def _head_bwd(kind):
    def build(r):
        B, H, W, N = 2, 5, 21, 16
        w, mref, old = _rand((3, 3, N, 1), 8000, 0.3), _rand((B, H, W, N), 8001), _rand((B, H, W, N), 8002)
        mask_ld, dx_ld = N + 12, N + 8
        wi, mi = r.inp("w", w), r.inp("mask", FP.wide_rows(mref, mask_ld, "cpu", fill=0.0))
        d = _ffi.HeadBwdDesc()
        d.B, d.H, d.W, d.N, d.dx_ld, d.mask_ld, d.accumulate_dx, d.mask_alpha = B, H, W, N, dx_ld, mask_ld, int(kind == 0), 0.2
        if kind == 0:
            Hr, Wr, cy, cx, Ho, Wo, mul = 12, 45, 3, 4, 7, 37, 2.5
            du = _rand((B, Ho, Wo), 8003)
            d.kind, d.Hr, d.Wr, d.cy, d.cx, d.Ho, d.Wo, d.mul = 0, Hr, Wr, cy, cx, Ho, Wo, mul
            s0, s1 = r.inp("du", du), None
        else:
            a1, a2 = _rand((B, H, W, 6), 8005), _rand((B, H, W, 9), 8006)
            d.kind, d.src0_ld, d.src1_ld = 1, 6, 9
            s0, s1 = r.inp("a1", a1), r.inp("a2", a2)
        r.keep.append(d)
        r.out("dV", (B, H, W)); r.out("dx", (B, H, W, dx_ld), prefill=(old if kind == 0 else None), sl=(N, 4))
        r.out("dV_shadow", (B, H, W, 32), dtype=BF16, written="any"); r.out("dx_shadow", (B, H, W, ops.shadow_ld(N)), dtype=BF16, written="any")
        r.call = lambda t, o: t.head_bwd(C.byref(d), (_P(s0) if kind == 0 else _P(s0, 2)), (_P(s1, 5) if s1 is not None else None), _P(o["dV"]), _P(o["dV_shadow"]), _P(wi),
                                          _P(o["dx"], 4), _P(mi), _P(o["dx_shadow"]), None)

        def dV_ref():
            if kind == 1:
                return a1.double()[..., 2] + a2.double()[..., 5]
            Vc = torch.zeros(B, H, W, dtype=torch.float64, requires_grad=True)
            up = (T.resize_bilinear(Vc[..., None], Hr, Wr) * mul)[:, cy:cy + Ho, cx:cx + Wo, 0]
            return torch.autograd.grad(up, [Vc], du.double())[0]
        r.oracle.append(("dV", dV_ref, GRAD, 2e-6))
    return build


case("HEAD_BWD", "kind 0: resize gradient, accumulate")(_head_bwd(0))
case("HEAD_BWD", "kind 1: two addends")(_head_bwd(1))


def _conv_planes(bf16):
    def build(r):
        B, H, W, K, N, dil = 2, 6, 13, 24, 40, 2
        x, w, b = _rand((B, H, W, K), 17000), _rand((3, 3, K, N), 17001, 0.2), _rand((N,), 17002)
        in_pld, out_pld, out_ld = ops.shadow_ld(K) + 32, ops.shadow_ld(N) + 64, N + 12
        d = ops.conv_desc(B, H, W, H, W, K, N, 3, 3, 1, dil, dil, dil, 0, 0, 0, out_ld, alpha=0.2, precision=1 if bf16 else 2)
        assert r.lib.conv2d_planes_ok(C.byref(d)) == 1
        r.keep.append(d)
        hi = x.to(BF16)
        hi_i, lo_i = r.inp("in_hi", _shadow(x, in_pld)), r.inp("in_lo", _shadow(x - hi.float(), in_pld))
        bank = _bank(r, w, 1 if bf16 else 2, 2)
        bi = r.inp("bias", b)
        r.out("out", (B, H, W, out_ld), sl=(N, 4)); r.out("out_hi", (B, H, W, out_pld), dtype=BF16, written="any")
        r.out("out_lo", (B, H, W, out_pld), dtype=BF16, written=("none" if bf16 else "any"))
        r.call = lambda t, o: t.conv2d_planes(C.byref(d), _P(hi_i), (None if bf16 else _P(lo_i)), in_pld, _P(bank), _P(bi), _P(o["out"], 4), _P(o["out_hi"]),
                                               (None if bf16 else _P(o["out_lo"])), out_pld, None)
        rd = FP.bf16_round if bf16 else (lambda t: t)
        r.oracle.append(("out", lambda: T.conv2d(rd(x).double(), rd(w).double(), b.double(), stride=1, dilation=dil, alpha=0.2), 3e-5 if bf16 else 4e-5, 0.0))
    return build


case("CONV_PLANES", "precision=1")(_conv_planes(True))
case("CONV_PLANES", "precision=2")(_conv_planes(False))


@case("CONV_PLANES_BWD", "mask sub-range")
def _(r):
    B, H, W, Ci, Co, dil = 2, 6, 13, 40, 24, 2
    dz, w, x = _rand((B, H, W, Co), 19000), _rand((3, 3, Ci, Co), 19001, 0.2), _rand((B, H, W, Ci), 19002)
    dz_pld, mask_pld, dx_pld, dx_ld = ops.shadow_ld(Co) + 32, ops.shadow_ld(Ci) + 64, ops.shadow_ld(Ci) + 96, Ci + 12
    d = ops.conv_desc(B, H, W, H, W, Ci, Co, 3, 3, 1, dil, dil, dil, 0, 0, dx_ld, 0, mask_alpha=0.2, precision=1, mask_c0=7, mask_c1=33)
    assert r.lib.conv2d_planes_bwd_ok(C.byref(d)) == 1
    r.keep.append(d)
    zi, mi = r.inp("dz_hi", _shadow(dz, dz_pld)), r.inp("mask_hi", _shadow(x, mask_pld))
    bank = _bank(r, w, 1, 3)
    r.out("dx", (B, H, W, dx_ld), sl=(Ci, 4)); r.out("dx_hi", (B, H, W, dx_pld), dtype=BF16, written="any")
    r.call = lambda t, o: t.conv2d_planes_bwd(C.byref(d), _P(zi), dz_pld, _P(bank), _P(mi), mask_pld, _P(o["dx"], 4), _P(o["dx_hi"]), dx_pld, None)

    def ref():
        xin = torch.zeros(B, H, W, Ci, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(T.conv2d(xin, FP.bf16_round(w).double(), None, stride=1, dilation=dil, alpha=1.0), xin, FP.bf16_round(dz).double())
        mk = torch.where(x.double() > 0, 1.0, 0.2)
        mk[..., :7] = 1.0
        mk[..., 33:] = 1.0
        return g * mk
    r.oracle.append(("dx", ref, 2e-5, 0.0))


@case("CONV_IMAGE", "stride 2, reflect pad, shadow")
def _(r):
    NB, H0, W0, Cc, N, stride = 4, 9, 14, 3, 16, 2
    rpt, rpl, Hp, Wp = 5, 7, 20, 29
    frames = torch.floor(torch.rand(NB, H0, W0, Cc, generator=torch.Generator().manual_seed(81)) * 256)
    w, b = _rand((3, 3, Cc, N), 82, 0.2), _rand((N,), 83)
    Ho, Wo, pt, pl = ops.conv_geometry(Hp, Wp, 3, 3, stride, 1)
    out_ld, shadow_ld, div, sub, alpha = N + 8, 64, 255.0, 0.25, 0.2
    fi, wi, bi = r.inp("frames", frames), r.inp("w", w), r.inp("bias", b)
    r.out("out", (NB, Ho, Wo, out_ld), sl=(N, 4)); r.out("shadow", (NB, Ho, Wo, shadow_ld), dtype=BF16, written="any")
    r.call = lambda t, o: t.conv_image_fwd(_P(fi), NB, H0, W0, Cc, Hp, Wp, rpt, rpl, div, sub, _P(wi), _P(bi), N, stride, pt, pl, alpha, _P(o["out"], 4), out_ld,
                                            _P(o["shadow"]), shadow_ld, None)

    def ref():
        refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
        iy, ix = refl(np.arange(Hp) - rpt, H0), refl(np.arange(Wp) - rpl, W0)
        xp = frames.double()[:, iy][:, :, ix] / _f(div) - _f(sub)
        return T.conv2d(xp, w.double(), b.double(), stride=stride, dilation=1, alpha=alpha)
    r.oracle.append(("out", ref, 2e-5, 0.0))


# ---- the table-driven launches: the device table points at the output set, so it is built per call ------------------------------------------------------
@case("WGRAD_REDUCE", "two segments")
def _(r):
    sizes, splits = (432, 1027), (5, 3)
    ws = [_rand((sp, sz), 90 + k) for k, (sz, sp) in enumerate(zip(sizes, splits))]
    wi = [r.inp("ws%d" % k, t) for k, t in enumerate(ws)]
    old = _rand((sizes[1],), 95)
    r.out("dst0", (sizes[0],)); r.out("dst1", (sizes[1],), prefill=old, written="acc")

    def call(t, o):
        segs = [(wi[0].ptr(), o["dst0"].ptr(), sizes[0], splits[0]), (wi[1].ptr(), o["dst1"].ptr(), sizes[1], splits[1], 1)]
        ops.wgrad_reduce(t, segs, r.dev, r.keep)
    r.call = call
    r.oracle += [("dst0", lambda: ws[0].double().sum(0), 1e-6, 0.0), ("dst1", lambda: ws[1].double().sum(0) + old.double(), 1e-6, 0.0)]


@case("PACK_W", "two banks")
def _(r):
    w0, w1 = _rand((3, 3, 12, 16), 96, 0.2), _rand((3, 3, 24, 40), 97, 0.2)
    i0, i1 = r.inp("w0", w0), r.inp("w1", w1)
    r.out("bank0", (ops.pack_bytes(w0, 2, 0) // 4,), written="any"); r.out("bank1", (ops.pack_bytes(w1, 1, 2) // 4,), written="any")
    r.call = lambda t, o: ops.pack_weights(t, [(i0.t.view(3, 3, 12, 16), o["bank0"].t, 2, 0), (i1.t.view(3, 3, 24, 40), o["bank1"].t, 1, 2)], r.dev, r.keep)


@case("SHADOW_CAST", "two tensors")
def _(r):
    a, b = _rand((2, 5, 7, 12), 98), _rand((1, 3, 9, 40), 99)
    ai, bi = r.inp("a", FP.wide_rows(a, 16, "cpu")), r.inp("b", b)
    r.out("sa", (2, 5, 7, 32), dtype=BF16); r.out("sb", (1, 3, 9, 64), dtype=BF16)

    def call(t, o):
        sa, sb = ops.Shadow.__new__(ops.Shadow), ops.Shadow.__new__(ops.Shadow)
        sa.B, sa.H, sa.W, sa.C, sa.ld, sa.t = 2, 5, 7, 12, 32, o["sa"].t
        sb.B, sb.H, sb.W, sb.C, sb.ld, sb.t = 1, 3, 9, 40, 64, o["sb"].t
        ops.shadow_cast(t, [(ops.View(ai.t.view(2, 5, 7, 16), 2, 5, 7, 12, 16), sa), (ops.view(bi.t.view(1, 3, 9, 40)), sb)], r.dev, r.keep)
    r.call = call
    r.oracle += [("sa", lambda: _shadow(a).double(), 0.0, 0.0), ("sb", lambda: _shadow(b).double(), 0.0, 0.0)]


@case("PLANE_SPLIT", "hi + lo, hi only")
def _(r):
    a, b = _rand((2, 5, 7, 12), 98), _rand((1, 3, 9, 40), 99)
    ai, bi = r.inp("a", FP.wide_rows(a, 16, "cpu")), r.inp("b", b)
    r.out("hi", (2, 5, 7, 32), dtype=BF16); r.out("lo", (2, 5, 7, 32), dtype=BF16); r.out("hb", (1, 3, 9, 64), dtype=BF16)

    def call(t, o):
        def sh(g, B, H, W, Cc, ld):
            s = ops.Shadow.__new__(ops.Shadow)
            s.B, s.H, s.W, s.C, s.ld, s.t = B, H, W, Cc, ld, g.t
            return s
        ops.plane_split(t, [(ops.View(ai.t.view(2, 5, 7, 16), 2, 5, 7, 12, 16), ops.Planes(sh(o["hi"], 2, 5, 7, 12, 32), sh(o["lo"], 2, 5, 7, 12, 32))),
                            (ops.view(bi.t.view(1, 3, 9, 40)), sh(o["hb"], 1, 3, 9, 40, 64))], r.dev, r.keep)
    r.call = call
    r.oracle += [("hi", lambda: _shadow(a).double(), 0.0, 0.0), ("lo", lambda: _shadow(a - a.to(BF16).float()).double(), 0.0, 0.0), ("hb", lambda: _shadow(b).double(), 0.0, 0.0)]


@case("WGRAD_STREAM", "two layers, one split each or more")
def _(r):
    layers = [(1, 6, 13, 24, 40, 5), (1, 6, 13, 40, 16, 1)]          # (B, H, W, K, N, dil)
    data = []
    for li, (B, H, W, K, N, dil) in enumerate(layers):
        x, gz = _rand((B, H, W, K), 20000 + 2 * li), _rand((B, H, W, N), 20001 + 2 * li)
        data.append((x, gz, r.inp("xs%d" % li, _shadow(x)), r.inp("zs%d" % li, _shadow(gz))))
        r.out("dw%d" % li, (9 * K * N,)); r.out("db%d" % li, (N,), prefill=torch.zeros(N), written="acc")
        r.atomic["db%d" % li] = ((lambda gz=gz: FP.bf16_round(gz).double().sum((0, 1, 2))), 1e-4, 0.0)

        def ref(x=x, gz=gz, K=K, N=N, dil=dil):
            w0 = torch.zeros(3, 3, K, N, dtype=torch.float64, requires_grad=True)
            return torch.autograd.grad(T.conv2d(FP.bf16_round(x).double(), w0, None, stride=1, dilation=dil, alpha=1.0), [w0], FP.bf16_round(gz).double())[0].reshape(-1)
        r.oracle.append(("dw%d" % li, ref, 2e-5, 0.0))

    def call(t, o):
        def sh(g, B, H, W, Cc):
            s = ops.Shadow.__new__(ops.Shadow)
            s.B, s.H, s.W, s.C, s.ld, s.t = B, H, W, Cc, ops.shadow_ld(Cc), g.t
            return s
        items = [(sh(xs, B, H, W, K), sh(zs, B, H, W, N), o["dw%d" % li].t.view(3, 3, K, N), o["db%d" % li].t, dil)
                 for li, ((B, H, W, K, N, dil), (_, _, xs, zs)) in enumerate(zip(layers, data))]
        wsa = ops.WgradWorkspace(r.dev); wsa.CHUNK = 1 << 20
        segs = []
        ops.wgrad_stream(t, r.lib, wsa, segs, items, r.dev, r.keep, target_wgs=5, nwaves=3)
        assert not segs, "the case is built for one split per layer (the gradient is stored straight into dw)"
        r.keep.append(wsa)
    r.call = call


# ---- the exemptions of the distinctness rule -------------------------------------------------------------------------------------------------------------
def _all_pairs(names, reason):
    names = names.split()
    return {(a, b): reason for i, a in enumerate(names) for b in names[i + 1:]}


def _cross(flags, counts, reason="tied"):
    return {(a, b): reason for a in flags.split() for b in counts.split()}


def _table(*dicts):
    out = {}
    for d in dicts:
        out.update(d)
    return out


# kind -> {(slot_a, slot_b): 'same' | 'flags' | 'tied'} (module docstring); written for either order of the pair
SAME_OK = {
    "CONV": _table({("kh", "kw"): "same", ("mode", "w_trans"): "same", ("Hi", "Ho"): "tied", ("Wi", "Wo"): "tied"},
                   _all_pairs("stride dil mode accumulate precision flags pad_t pad_l", "flags"), _all_pairs("stride dil w_trans accumulate precision flags pad_t pad_l", "flags"),
                   _cross("stride dil mode w_trans accumulate precision flags pad_t pad_l", "B kh kw mask_c0 mask_c1 Ho Wo")),
    "RESIZE_FWD": _table(_all_pairs("mode accumulate", "flags")),
    "RESIZE_BWD": _table(_all_pairs("mode accumulate", "flags")),
    "LOSS": _cross("phase", "B"),
    "COPY_CH": _cross("accumulate", "nch"),
    "WARP_BWD": _cross("acc_u", "B"),
    "CORR_FWD": _table(_all_pairs("stride copy_left zero_tail precision", "flags"), _cross("stride copy_left zero_tail precision", "B md coff")),
    "CORR_BWD": _table(_all_pairs("acc_l acc_r acc_u stride copy_left precision", "flags"), _cross("acc_l acc_r acc_u stride copy_left precision", "B md coff")),
    "CORR_WARP_BWD": _table(_all_pairs("acc_l stride copy_left", "flags"), _cross("acc_l stride copy_left", "B md coff")),
    "LEVEL_FRONT": _table(_cross("zero_tail", "B md"), {("coff", "Cc"): "tied"}),
    "HEAD_BWD": _table(_all_pairs("kind accumulate_dx", "flags"), _cross("kind accumulate_dx", "B Hr Wr cy cx Ho Wo src0_ld src1_ld")),
    "BIAS_GRAD": _cross("nblocks", "nch"),
}


def _named_slots(op):
    """([(name, value)] of the int slots the rule covers -- mh_op.n among them --, the same of the float slots)"""
    L = oplayout.LAYOUT[op.kind]
    ints, floats = [(nm, int(op.i[k])) for k, nm in L.i], [(nm, float(op.f[k])) for k, nm in L.f]
    if L.name == "FETCH_INPUTS":
        ints = [(nm, v) for nm, v in ints if nm == "n" or int(nm[5:]) < op.i[0]]
    if L.name in DESC_KINDS and L.name != "CONV":
        ints = [(nm, v) for nm, v in ints if nm not in oplayout.DESC_FIELDS]
        floats = []
    if L.name == "HEAD_BWD":
        kind = op.i[0]          # kind 0 reads the resize geometry, kind 1 the addends' strides: the others are not arguments of the case
        dead = ("src0_ld", "src1_ld") if kind == 0 else ("Hr", "Wr", "cy", "cx", "Ho", "Wo")
        ints = [(nm, v) for nm, v in ints if nm not in dead]
    if L.name == "LEVEL_FRONT":          # the forms without planes / without the head do not read their slots
        dead = (() if op.p[6] else ("out_pld",)) + (() if op.p[8] else ("x_ld", "K"))
        ints = [(nm, v) for nm, v in ints if nm not in dead]
    if L.name == "CONV" and not op.p[4]:      # no mask_ref: its stride, range and slope are not read
        ints = [(nm, v) for nm, v in ints if nm not in ("mask_ld", "mask_c0", "mask_c1")]
        floats = [(nm, v) for nm, v in floats if nm != "mask_alpha"]
    if L.n:
        ints.append((L.n, int(op.n)))
    return ints, floats


def _collisions(op):
    out = []
    for slots in _named_slots(op):
        out += [(a, b) for i, (a, va) in enumerate(slots) for b, vb in slots[i + 1:] if va == vb]
    return out


def _allowed(kind, a, b):
    t = SAME_OK.get(kind, {})
    return t.get((a, b)) or t.get((b, a))


def _record(run):
    rec = PL.Recorder()
    o = run.fresh()
    run.call(rec, o)
    assert len(rec.ops) == 1
    return rec, o


# ---- the tests --------------------------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_kind():
    """host only: every kind of the layout outside EXEMPT has a case (a new kind cannot arrive untested); EXEMPT holds exactly the two documented kinds"""
    assert set(EXEMPT) == {_ffi.OP_RESERVED_25, _ffi.OP_ALLREDUCE}
    names = {L.name: k for k, L in oplayout.LAYOUT.items()}
    assert {names[kind] for kind, _, _ in CASES} == set(oplayout.LAYOUT) - set(EXEMPT)
    assert len({(k, f) for k, f, _ in CASES}) == len(CASES)


def test_exempted_pairs_differ_in_some_case(backend):
    """over the case table (recorded, nothing launched but the packing of the banks): every SAME_OK pair of flags or small values differs in one case of
    its kind; every pointer slot the layout names is non-NULL in one case; the two-meaning slots appear under both meanings"""
    seen, ptrs, meanings = {}, {}, set()
    for kind, form, build in CASES:
        run = Run(backend.device, backend.lib)
        build(run)
        rec, _ = _record(run)
        op = rec.ops[0]
        L = oplayout.LAYOUT[op.kind]
        assert L.name == kind, (kind, form)
        vals = dict(_named_slots(op)[0])
        for (a, b), why in SAME_OK.get(kind, {}).items():
            if why != "same" and a in vals and b in vals and vals[a] != vals[b]:
                seen[(kind, a, b)] = form
        ptrs.setdefault(kind, set()).update(nm for k, nm in L.p if op.p[k])
        f = oplayout.fields(op)
        if kind == "CONV":
            if op.p[2]:
                meanings.add("mask_shadow" if f.flags & oplayout.CONV_MASK_SHADOW else "bias")
            if op.p[5]:
                meanings.add("out_lo" if f.flags & oplayout.CONV_OUT_PLANES else "in_shadow")
            if op.p[7]:
                meanings.add("out_hi" if f.flags & oplayout.CONV_OUT_PLANES else "shadow")
        if kind == "BIAS_GRAD":
            meanings.add("ws" if f.nblocks > 0 else "db")
    backend.sync()
    missing = [(kind, a, b) for kind, t in SAME_OK.items() for (a, b), why in t.items() if why != "same" and (kind, a, b) not in seen]
    assert not missing, "exempted pairs that are equal in every case of their kind: %s" % missing
    for kind, got in ptrs.items():
        L = oplayout.LAYOUT[getattr(_ffi, "OP_" + kind)]
        want = {nm for k, nm in L.p}
        if kind == "FETCH_INPUTS":
            want = {"table"} | {"dst%d" % k for k in range(_ffi.FETCH_MAX)}
        assert got == want, "%s: pointer slots that are NULL in every case: %s" % (kind, sorted(want - got))
    assert meanings == {"bias", "mask_shadow", "in_shadow", "out_lo", "shadow", "out_hi", "db", "ws"}, meanings


_worst = {}          # kind -> {"forms": [...], "bits": bool, "err": {output: worst error}}


def _judge_atomic(run, name, g, what, rec):
    ref, rtol, atol = run.atomic[name]
    ok, e = _err(run.value(name, g), ref().reshape(run.value(name, g).shape), rtol, atol)
    rec[name] = max(rec.get(name, 0.0), e)
    assert ok, "%s: %s error %.3g against float64 (rtol %g, atol %g)" % (what, name, e, rtol, atol)


def _conv_oracle(run, spec, got, name, what):
    _, L, mode, bias, alpha, mask, acc = spec
    rounded, tol, _ = _tolerance(name)
    ref = L.expected(mode, rounded, bias, alpha, mask, acc, mask_alpha=0.3)
    e = (got.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    assert e <= tol, "%s: relative error %.3g > %.3g against the float64 oracle [%s]" % (what, e, tol, name)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["%s: %s" % (k, f) for k, f, _ in CASES])
def test_replay_equals_the_direct_call(backend, idx):
    kind, form, build = CASES[idx]
    lib, dev = backend.lib, backend.device
    what = "%s [%s] (%s)" % (kind, form, backend.name)
    run = Run(dev, lib)
    build(run)
    backend.sync()
    ins_before = {k: g.snapshot() for k, g in run.ins.items()}
    marker = torch.zeros(64, device=dev)
    md = ops.conv_desc(1, 1, 1, 1, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, 4, 4)

    def note_another_kernel():
        lib.conv2d(C.byref(md), ops._p(marker), ops._p(marker[16:]), None, ops._p(marker[32:]), None, None)
        return lib.last_kernel().decode()

    # the direct call
    note_another_kernel()
    od = run.fresh()
    before = {k: g.snapshot() for k, g in od.items()}
    run.call(lib, od)
    kd = lib.last_kernel().decode()
    backend.sync()
    # the recorded op, replayed
    rec, op_ = _record(run)
    op = rec.ops[0]
    assert oplayout.LAYOUT[op.kind].name == kind
    bad = [(a, b) for a, b in _collisions(op) if not _allowed(kind, a, b)]
    assert not bad, "%s: slots with equal values (a swap of the two would go unseen): %s of %s" % (what, bad, _named_slots(op))
    km = note_another_kernel()
    rec.compile().run(lib, None)
    kp = lib.last_kernel().decode()
    backend.sync()
    assert kp == kd, "%s: the replay noted %r, the direct call %r" % (what, kp, kd)
    w = _worst.setdefault(kind, {"forms": [], "err": {}, "bits": True})
    w["forms"].append(form)
    # 4. / 5. the direct result
    for name, g in od.items():
        s = run.spec[name]
        g.assert_guards(what + ": " + name)
        wr = s["written"]
        if wr == "slice":
            FP.assert_only_slice_written(g, run.view(name, g), s["sl"][1], before[name], what + ": " + name, zero_cols=s["zero_cols"])
        elif wr == "all":
            FP.assert_fully_written(g, g.n, what + ": " + name)
        elif wr == "none":
            FP.assert_untouched(g, before[name], what + ": " + name)
        if wr in ("slice", "all", "acc") and s["dtype"] in (torch.float32, BF16):
            v = run.value(name, g).float()
            assert torch.isfinite(v).all(), "%s: %s is not finite" % (what, name)
            assert s["const_ok"] or v.numel() < 4 or v.unique().numel() > 1, "%s: %s is constant" % (what, name)
    for ent in run.oracle:
        name, ref, rtol, atol = ent[:4]
        got = run.value(name, od[name])
        if isinstance(ref, tuple):
            _conv_oracle(run, ref, got, kd, what + ": " + name)
            continue
        if len(ent) > 4 and ent[4] is not None:
            got = ent[4](got)
        r64 = ref()
        ok, e = _err(got.double() if got.dtype == torch.int64 else got.float(), r64.reshape(got.shape), rtol, atol)
        assert ok, "%s: %s error %.3g against the float64 oracle (rtol %g, atol %g)" % (what, name, e, rtol, atol)
    # 2. / 3. the replay against the direct call
    for name in od:
        op_[name].assert_guards(what + ": replayed " + name)
        if name in run.atomic:
            w["bits"] = False
            _judge_atomic(run, name, od[name], what + " direct", w["err"])
            _judge_atomic(run, name, op_[name], what + " replay", w["err"])
        elif run.stamp:
            a, b = int(od[name].t.cpu()[0]), int(op_[name].t.cpu()[0])
            assert a != od[name].fill and b != op_[name].fill and b >= a, "%s: stamps %d (direct), %d (replay)" % (what, a, b)
        else:
            same = torch.equal(FP.bits(op_[name].all), FP.bits(od[name].all))
            assert same, "%s: output %s of the replay differs from the direct call in %d elements" % (
                what, name, int((FP.bits(op_[name].all) != FP.bits(od[name].all)).sum()))
    for k, g in run.ins.items():
        FP.assert_untouched(g, ins_before[k], what + ": input " + k)
    assert km != "" or kd == ""


def test_zz_report(backend):
    """one line per kind (run behind the cases of its backend): the forms run, whether compared on bits, the worst float64 error of the atomic outputs"""
    for kind in sorted(_worst):
        w = _worst[kind]
        print("%s (%s): forms %s; %s%s" % (kind, backend.name, ", ".join(sorted(set(w["forms"]))), "bits" if w["bits"] else "float64 oracle for the atomic outputs, bits for the rest",
                                            "".join("; worst %s %.3g" % kv for kv in sorted(w["err"].items()))))
