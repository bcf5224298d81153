"""Seeded shape sweeps of the FUSED level ops -- mh_corr_warp_bwd (all three kernels and the ,det twin), mh_head_bwd, mh_level_front_fwd / _planes / _head --
in the style of tests/test_shape_sweep.py (whose helpers they use): fixed lists drawn from the literal seed plus hand-placed edge shapes, every output in a
guarded NaN-prefilled buffer or a channel slice of one, references in float64 from oracle/tf_ops.py and its autograd, the tolerances of the simple ops' sweeps
(FWD 2e-5, GRAD 5e-5 relative to max(1, |ref|max)).  Failure messages carry the shape and the kernel that was dispatched."""
import ctypes as C

import torch

import footprint as FP
from madnet_hip import _ffi, ops
from oracle import tf_ops as T
from test_shape_sweep import FWD, GRAD, _Worst as _WorstAbs, _coords, _err, _out, _rand, _rng


class _Worst(_WorstAbs):
    """_Worst of tests/test_shape_sweep.py that also keeps, per key, the largest FRACTION of its tolerance an error used (the gradients here reach |ref| ~ 100:
    an absolute figure alone says little)"""

    def __init__(self, op):
        _WorstAbs.__init__(self, op)
        self.frac = {}

    def check(self, what, key, got, ref, rtol, atol=2e-6):
        _, e = _err(got, ref, rtol, atol)
        r = ref.detach().cpu().double()
        tol = atol + rtol * max(1.0, r.abs().max().item() if r.numel() else 0.0)
        self.frac[key] = max(self.frac.get(key, 0.0), e / tol)
        _WorstAbs.check(self, what, key, got, ref, rtol, atol)

    def report(self, backend, n):
        _WorstAbs.report(self, backend, n)
        print("%s (%s): worst error / tolerance %s" % (self.op, backend.name, ", ".join("%s %.3g" % kv for kv in sorted(self.frac.items()))))


def _kernel(lib):
    return lib.last_kernel().decode()


def _i16(dev, n):
    """a guarded buffer of n halfs (bf16 shadows / planes), sentinel-prefilled"""
    return FP.Guarded(n, torch.int16, dev)


def _bf16_bits(t):
    return FP.bits(t.detach().cpu().float().to(torch.bfloat16))


# ---- mh_corr_warp_bwd ---------------------------------------------------------------------------------------------------------------------------
CWB_FORMS = {"rowlds": 1, "row": 3, "atomic": 0}                   # mh_tune_corr_row
CWB_FLAGS = [(1, 1, 1, 0), (1, 0, 0, 1), (0, 0, 1, 1), (0, 1, 0, 0)]          # (copy_left, acc_l, acc_img, outputs are channel slices)
CWB_HAND = [(1, 2, 9, 8, 2, 1), (2, 3, 17, 32, 2, 1),
            (1, 2, 21, 16, 3, 1), (1, 2, 21, 32, 4, 1), (1, 2, 3, 4, 4, 1),        # D = 7 and 9: the generic kernel; W < D in the last
            (1, 3, 13, 16, 4, 2), (1, 2, 11, 8, 2, 2),                             # stride 2
            (1, 1, 1, 4, 2, 1), (1, 2, 5, 64, 0, 1),                               # W = 1; D = 1
            (1, 1, 40, 132, 2, 1)]                                                 # C > 128: no LDS-staged instance


def _cwb_dispatch(form, W, Cc, D, det):
    """The kernel mh_corr_warp_bwd launches (the prefix of mh_last_kernel's note) -- the conditions of its dispatch in csrc/corr.hip restated; every launch
    of the sweep asserts the name, so a threshold that moves there fails here instead of silently moving a shape to another kernel."""
    C4 = Cc // 4
    lpp_px = 4 if C4 <= 4 else (8 if C4 <= 8 else 16)
    fast = D <= 5
    row_lds = (W * Cc * (8 if det else 4) + W * 4 + 15) & ~15
    if form != "atomic" and fast and row_lds <= 150 * 1024:
        lpp = 8 if C4 <= 8 else (16 if C4 <= 16 else 32)
        lds_st = (3 * W * Cc + W * 23 + 8) * 4
        if form == "rowlds" and C4 <= 32 and W <= 3 * (1024 // lpp) and W * C4 <= 3 * 1024 and W * 8 <= 3 * 1024 and lds_st <= 155 * 1024:
            return "corr_warp_bwd_rowlds_kernel<LPP=%d,DT=5>" % lpp
        return "corr_warp_bwd_row_kernel<LPP=%d,DT=5%s>" % (lpp_px, ",det" if det else "")
    return "corr_warp_bwd_kernel<LPP=%d%s>" % (lpp_px, ",DT=5" if fast else "")


def _cwb_limit(form, Cc, det=False):
    """(W, W + 1): the last width the row-owned kernel of `form` serves at C channels (D = 5) and the first it does not"""
    own = "corr_warp_bwd_%s_kernel" % form
    W = 1
    assert own in _cwb_dispatch(form, W, Cc, 5, det)
    while own in _cwb_dispatch(form, W + 1, Cc, 5, det):
        W += 1
    return W, W + 1


def _cwb_seeded():
    r = _rng("corr_warp_bwd")
    out = []
    while len(out) < 25:
        md = r.randint(0, 4)
        st = 2 if (md in (2, 4) and r.random() < 0.4) else 1
        out.append((r.randint(1, 2), r.randint(1, 4), r.randint(1, 45), r.choice([4, 8, 16, 20, 32, 48, 64, 96, 128]), md, st))
    return out


def _cwb_limit_shapes():
    """[(shape, form)]: both sides of every dispatch limit, at H = 1 / 2.  Derived, not written down -- at the time of writing the LDS-staged kernel ends at
    W = 96 (C = 128: W * C / 4 <= 3072), 184 (C = 64: the 155 KiB of LDS), 333 (C = 32: LDS), 384 (C = 8: three items per thread); the row kernel at C = 128 at
    W = 297 (516 bytes of LDS per column in 150 KiB), 149 in deterministic mode (1028 bytes per column: test_corr_warp_bwd_sweep adds that pair itself)."""
    out = []
    for Cc in (128, 64, 32, 8):
        for i, W in enumerate(_cwb_limit("rowlds", Cc)):
            out.append(((1, 1 + i, W, Cc, 2, 1), "rowlds"))
    for i, W in enumerate(_cwb_limit("row", 128)):
        out.append(((1, 1 + i, W, 128, 2, 1), "row"))
    return out


CWB_SHAPES = CWB_HAND + _cwb_seeded()


class _CwbCase(object):
    """inputs and the float64 reference gradients of one shape (computed once, shared by every form and flag combination)"""

    def __init__(self, k, shp, dev):
        B, H, W, Cc, md, st = shp
        self.shp, self.dev = shp, dev
        self.D = D = 2 * md // st + 1
        self.img, self.L = _rand((B, H, W, Cc), 7000 + 10 * k), _rand((B, H, W, Cc), 7001 + 10 * k)
        self.u = _coords(B, H, W, 7002 + 10 * k, -6.0, 6.0)
        if k % 3 == 2 and W >= 12:
            # a compressed stretch: the whole first row lands on two source columns (more taps than a column's list holds in the LDS-staged kernel)
            self.u[0, 0] = float(W // 2) + 0.25 - torch.arange(W, dtype=torch.float32)
        self.oldl, self.oldi = _rand((B, H, W, Cc), 7003 + 10 * k), _rand((B, H, W, Cc), 7004 + 10 * k)
        ic, uc = self.img.double().requires_grad_(True), self.u.double()[..., None].requires_grad_(True)
        Rw64 = T.linear_warp(ic, uc)
        self.Rw = Rw64.detach().float()
        self.g, self.ref = {}, {}
        for copy_left in (0, 1):
            coff = Cc if copy_left else 3
            g_ld = FP.round_up(coff + D + 1, 4)
            g = _rand((B, H, W, g_ld), 7005 + 10 * k + copy_left)
            Lc, Rl = self.L.double().requires_grad_(True), self.Rw.double().requires_grad_(True)
            corr = T.correlation(Lc, Rl, md, st)
            assert corr.shape[-1] == D
            gl, grw = torch.autograd.grad(corr, [Lc, Rl], g.double()[..., coff:coff + D])
            gi, gu = torch.autograd.grad(Rw64, [ic, uc], grw, retain_graph=True)
            self.g[copy_left] = (g, coff, g_ld)
            self.ref[copy_left] = (gl + (g.double()[..., :Cc] if copy_left else 0), gi, g.double()[..., coff + D] + gu[..., 0])
        self.dev_in = None

    def on_device(self):
        if self.dev_in is None:
            d = self.dev
            self.dev_in = dict(img=self.img.to(d), L=self.L.to(d), u=self.u.to(d), Rw=self.Rw.to(d), g={c: v[0].to(d) for c, v in self.g.items()})
        return self.dev_in

    def run(self, backend, W_, form, flags, expect, seen, what, want_dimg=True, want_du=True):
        """one launch, every output guarded, compared with the oracle -> the (dL, dimg, du) bits"""
        lib, dev = backend.lib, self.dev
        B, H, W, Cc, md, st = self.shp
        copy_left, acc_l, acc_img, sliced = flags
        t = self.on_device()
        g, coff, g_ld = self.g[copy_left]
        rl, ri, ru = self.ref[copy_left]
        if sliced:
            gl_, dLv = FP.slice_view(dev, B, H, W, Cc, 4, 4, self.oldl if acc_l else None)
            gi_, div = FP.slice_view(dev, B, H, W, Cc, 8, 4, self.oldi if acc_img else None)
        else:
            gl_, dLt = _out(dev, (B, H, W, Cc), self.oldl if acc_l else None)
            gi_, dit = _out(dev, (B, H, W, Cc), self.oldi if acc_img else None)
            dLv, div = ops.view(dLt), ops.view(dit)
        gu_, du = _out(dev, (B, H, W))
        bl, bi, bu = gl_.snapshot(), gi_.snapshot(), gu_.snapshot()
        gv = ops.View(t["g"][copy_left], B, H, W, g_ld, g_ld)
        ops.corr_warp_bwd(lib, gv, ops.view(t["L"]), ops.view(t["Rw"]), ops.view(t["img"]), t["u"], dLv, div if want_dimg else None, du if want_du else None,
                          md, st, coff=coff, acc_l=bool(acc_l), copy_left=bool(copy_left), acc_img=bool(acc_img))
        name = _kernel(lib)
        backend.sync()
        what = "%s flags %s -> %s" % (what, flags, name)
        assert name.startswith(expect), "%s: expected %s" % (what, expect)
        seen.add(name.split(">")[0] + ">")
        if sliced:
            FP.assert_only_slice_written(gl_, dLv, 4, bl, what + ": dL")
            dL = FP.slice_of(gl_, dLv, 4)
        else:
            FP.assert_fully_written(gl_, gl_.n, what + ": dL")
            dL = gl_.t.view(B, H, W, Cc).cpu()
        W_.check(what, "dL", dL, rl + (self.oldl.double() if acc_l else 0), GRAD)
        dimg = None
        if not want_dimg:
            FP.assert_untouched(gi_, bi, what + ": dimg (not passed)")
        else:
            if sliced:
                FP.assert_only_slice_written(gi_, div, 8, bi, what + ": dimg")          # (overwrite mode: the slice started as the sentinel)
                dimg = FP.slice_of(gi_, div, 8)
            else:
                FP.assert_fully_written(gi_, gi_.n, what + ": dimg")
                dimg = gi_.t.view(B, H, W, Cc).cpu()
            W_.check(what, "dimg", dimg, ri + (self.oldi.double() if acc_img else 0), GRAD)
        if not want_du:
            FP.assert_untouched(gu_, bu, what + ": du (not passed)")
        else:
            FP.assert_fully_written(gu_, gu_.n, what + ": du")
            W_.check(what, "du", du, ru, GRAD)
        return FP.bits(dL), (FP.bits(dimg) if dimg is not None else None), FP.bits(du)


def test_corr_warp_bwd_sweep(backend):
    """mh_corr_warp_bwd against float64: Rw = linear_warp(img, u), the autograd gradients of correlation(L, Rw) w.r.t. L and Rw, the latter pushed through
    the warp to img and u.  Every shape x {LDS-staged row kernel, row kernel, global atomics} x four (copy_left, acc_l, overwrite dimg, sliced outputs)
    combinations; D = 1 .. 9 (the DT=5 and the generic atomic kernel), stride 2, W = 1, W < D, C > 128, a row folded onto two columns; both sides of every
    width limit of the dispatch; the ,det row kernel (oracle + bit-identical twice); the du-only and the scatter-only call.  At the end: every kernel
    instance the dispatch can choose has been seen."""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_corr_warp_bwd")
    seen = set()
    cases = {}

    def case(k, shp):
        if k not in cases:
            cases.clear()                       # (one shape's tensors at a time)
            cases[k] = _CwbCase(k, shp, dev)
        return cases[k]

    limits = _cwb_limit_shapes()
    det_limits = [((1, 1 + i, W, 128, 2, 1), "row") for i, W in enumerate(_cwb_limit("row", 128, det=True))]
    nlaunch = 0
    try:
        for k, shp in enumerate(CWB_SHAPES):
            B, H, W, Cc, md, st = shp
            c = case(k, shp)
            for form in ("rowlds", "row", "atomic"):
                lib.tune_corr_row(CWB_FORMS[form])
                expect = _cwb_dispatch(form, W, Cc, c.D, False)
                for flags in CWB_FLAGS:
                    c.run(backend, W_, form, flags, expect, seen, "shape %d %s D=%d form %s" % (k, shp, c.D, form))
                    nlaunch += 1
                if k % 5 == 0:
                    # du only / scatter only: the output that is not passed stays untouched, the other two are what the full call gives
                    c.run(backend, W_, form, CWB_FLAGS[k // 5 % 4], expect, seen, "shape %d %s du only, form %s" % (k, shp, form), want_dimg=False)
                    c.run(backend, W_, form, CWB_FLAGS[(k // 5 + 1) % 4], expect, seen, "shape %d %s scatter only, form %s" % (k, shp, form), want_du=False)
                    nlaunch += 2
        # both sides of every dispatch limit
        for n, (shp, form) in enumerate(limits):
            k = 100 + n
            c = case(k, shp)
            own = "corr_warp_bwd_%s_kernel" % form
            assert (own in _cwb_dispatch(form, shp[2], shp[3], c.D, False)) == (n % 2 == 0), (shp, form)            # W: the last one served; W + 1: the next kernel down
            for f in ("rowlds", "row", "atomic"):
                lib.tune_corr_row(CWB_FORMS[f])
                expect = _cwb_dispatch(f, shp[2], shp[3], c.D, False)
                for flags in CWB_FLAGS:
                    c.run(backend, W_, f, flags, expect, seen, "limit shape %s (of %s) form %s" % (shp, form, f))
                    nlaunch += 1
        # deterministic mode (an unrelated registered range switches it on): the row kernel accumulates in 64-bit fixed point
        other = torch.zeros(64, device=dev); twin = torch.zeros(64, dtype=torch.int64, device=dev)
        assert lib.deterministic_add(C.c_void_p(other.data_ptr()), 64, C.c_void_p(twin.data_ptr())) == 0
        try:
            lib.tune_corr_row(3)
            dets = [(k, CWB_SHAPES[k], "row") for k in (0, 1, 5, 6, 8, 9, 12, 15)] + [(120 + n, s, f) for n, (s, f) in enumerate(det_limits)]
            for n, (k, shp, form) in enumerate(dets):
                c = case(k, shp)
                expect = _cwb_dispatch(form, shp[2], shp[3], c.D, True)
                if k >= 120:
                    assert (",det" in expect) == (k == 120), (shp, expect)
                flags = CWB_FLAGS[n % 4]
                a = c.run(backend, W_, form, flags, expect, seen, "det shape %d %s" % (k, shp))
                b = c.run(backend, W_, form, flags, expect, seen, "det shape %d %s (again)" % (k, shp))
                nlaunch += 2
                if ",det" in expect:
                    assert all(torch.equal(x, y) for x, y in zip(a, b)), "det shape %d %s: two launches of %s differ" % (k, shp, expect)
        finally:
            lib.deterministic_remove(C.c_void_p(other.data_ptr()))
    finally:
        lib.tune_corr_row(1)
    W_.report(backend, len(CWB_SHAPES) + len(limits) + len(det_limits))
    print("mh_corr_warp_bwd (%s): %d launches, kernels %s" % (backend.name, nlaunch, sorted(seen)))
    need = ["corr_warp_bwd_rowlds_kernel<LPP=%d,DT=5>" % l for l in (8, 16, 32)] + ["corr_warp_bwd_row_kernel<LPP=%d,DT=5>" % l for l in (4, 8, 16)] + \
           ["corr_warp_bwd_kernel<LPP=%d,DT=5>" % l for l in (4, 8, 16)] + ["corr_warp_bwd_kernel<LPP=%d>" % l for l in (4, 8, 16)]
    missing = [n for n in need if n not in seen]
    assert not missing and any(",det>" in n for n in seen), "kernel instances the sweep never launched: %s (seen %s)" % (missing, sorted(seen))


# ---- mh_head_bwd --------------------------------------------------------------------------------------------------------------------------------
def _head_bwd_shapes():
    r = _rng("head_bwd")
    out = []
    Ns = [4, 8, 12, 16, 20, 32, 48, 64]
    for i in range(40):
        B, H, W = r.randint(1, 2), r.randint(1, 9), r.randint(1, 70)
        if i == 3:
            H, W = 9, 70                                     # three tiles down, three across, partial in both directions
        N = Ns[i % 8] if i < 16 else r.choice(Ns)
        kind = 1 if i % 3 == 2 else 0
        acc, mask = i % 2, (i // 2) % 2
        if kind == 0:
            Hr, Wr = r.randint(H, 3 * H + 2), r.randint(W, 3 * W + 2)
            Ho, Wo = r.randint(1, Hr), r.randint(1, Wr)
            cy, cx = r.randint(0, Hr - Ho), r.randint(0, Wr - Wo)
            if i % 8 == 0:
                Hr, Wr, cy, cx, Ho, Wo = 2 * H, 2 * W, 0, 0, 2 * H, 2 * W           # the exact x2 form
            geo = (Hr, Wr, cy, cx, Ho, Wo, r.choice([2.5, -20.0, 1.0]))
        else:
            geo = r.choice(["both", "both", "src0", "src1"])
        out.append((B, H, W, N, kind, acc, mask, geo))
    return out


HEAD_BWD_SHAPES = _head_bwd_shapes()


def test_head_bwd_sweep(backend):
    """mh_head_bwd against float64.  kind 0: dV = the autograd gradient of (resize_bilinear(V, Hr, Wr) * mul)[crop] against du for ANY resized size in
    [H, 3H+2] x [W, 3W+2] and crop (every eighth shape the exact x2 form), kind 1: the sum of one or two strided addends; dx = (input gradient of the head's
    3x3 N -> 1 conv against dV + old dx) * leaky'(mask_ref) -- the mask applies to the SUM (mh_conv2d mode 1, accumulate) and an exact 0.0 in mask_ref takes
    the slope.  N = 4 .. 64, the four (accumulate, mask) combinations, partial and several 4 x 32 tiles in both directions, dx a channel slice; the bf16
    shadows bit-equal to the rounded fp32 stores, their padding halfs untouched."""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_head_bwd")
    assert len(set((s[4], s[5], s[6]) for s in HEAD_BWD_SHAPES)) == 8 and set(s[3] for s in HEAD_BWD_SHAPES) == {4, 8, 12, 16, 20, 32, 48, 64}
    for k, shp in enumerate(HEAD_BWD_SHAPES):
        B, H, W, N, kind, acc, mask, geo = shp
        w = _rand((3, 3, N, 1), 8000 + 10 * k, 0.3)
        mref = _rand((B, H, W, N + 4), 8001 + 10 * k)
        mref[0, 0, 0, 0] = 0.0                               # exactly zero: takes the slope
        old = _rand((B, H, W, N), 8002 + 10 * k)
        alpha = 0.2
        d = _ffi.HeadBwdDesc()
        d.B, d.H, d.W, d.N = B, H, W, N
        keep = []
        if kind == 0:
            Hr, Wr, cy, cx, Ho, Wo, mul = geo
            du = _rand((B, Ho, Wo), 8003 + 10 * k)
            Vc = _rand((B, H, W), 8004 + 10 * k).double().requires_grad_(True)
            up = (T.resize_bilinear(Vc[..., None], Hr, Wr) * mul)[:, cy:cy + Ho, cx:cx + Wo, 0]
            (dV_ref,) = torch.autograd.grad(up, [Vc], du.double())
            d.kind, d.Hr, d.Wr, d.cy, d.cx, d.Ho, d.Wo, d.mul = 0, Hr, Wr, cy, cx, Ho, Wo, mul
            dud = du.to(dev); keep.append(dud)
            src0, src1 = ops._p(dud), None
        else:
            a1, a2b = _rand((B, H, W), 8005 + 10 * k), _rand((B, H, W, 8), 8006 + 10 * k)
            a1d, a2d = a1.to(dev), a2b.to(dev); keep += [a1d, a2d]
            p1, p2 = ops._p(a1d), C.c_void_p(a2d.data_ptr() + 4 * 5)            # a plain map; channel 5 of rows of 8
            d.kind = 1
            if geo == "both":
                dV_ref, src0, src1, d.src0_ld, d.src1_ld = a1.double() + a2b.double()[..., 5], p1, p2, 1, 8
            elif geo == "src0":
                dV_ref, src0, src1, d.src0_ld, d.src1_ld = a2b.double()[..., 5], p2, None, 8, 0
            else:
                dV_ref, src0, src1, d.src0_ld, d.src1_ld = a1.double(), None, p1, 0, 1
        xin = torch.zeros(B, H, W, N, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad(T.conv2d(xin, w.double(), None, 1, 1, 1.0), [xin], dV_ref.detach()[..., None])
        dx_ref = gx + (old.double() if acc else 0)
        if mask:
            dx_ref = dx_ref * torch.where(mref[..., :N] > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(float(torch.tensor(alpha, dtype=torch.float32)), dtype=torch.float64))
        coff = 4 if k % 2 else 0                             # rows of N + 4: the slice at either end
        gx_, dxv = FP.slice_view(dev, B, H, W, N, coff, 4 - coff, old if acc else None)
        gv_, dV = _out(dev, (B, H, W))
        shV, shx = _i16(dev, B * H * W * 32), _i16(dev, B * H * W * FP.round_up(N, 32))
        before = gx_.snapshot()
        md_ = mref.to(dev); wd = w.to(dev)
        d.dx_ld, d.mask_ld, d.accumulate_dx, d.mask_alpha = dxv.ld, (N + 4 if mask else 0), acc, alpha
        lib.head_bwd(C.byref(d), src0, src1, ops._p(dV), C.c_void_p(shV.ptr()), ops._p(wd), ops._p(dxv), (ops._p(md_) if mask else None), C.c_void_p(shx.ptr()), None)
        name = _kernel(lib)
        backend.sync()
        what = "shape %d %s -> %s" % (k, shp, name)
        assert "head_bwd_kernel kind %d N=%d" % (kind, N) in name, what
        FP.assert_fully_written(gv_, gv_.n, what + ": dV")
        FP.assert_only_slice_written(gx_, dxv, coff, before, what + ": dx")
        dx = FP.slice_of(gx_, dxv, coff)
        W_.check(what, "dV", dV, dV_ref, GRAD)
        W_.check(what, "dx", dx, dx_ref, GRAD)
        shV.assert_guards(what + ": dV shadow"); shx.assert_guards(what + ": dx shadow")
        sv = shV.payload_bits().view(B, H, W, 32)
        sx = shx.payload_bits().view(B, H, W, FP.round_up(N, 32))
        assert torch.equal(sv[..., 0], _bf16_bits(dV)), what + ": dV shadow != bf16(dV)"
        assert bool((sv[..., 1:] == FP.NAN16).all()), what + ": halfs behind channel 0 of the dV shadow were written"
        assert torch.equal(sx[..., :N], _bf16_bits(dx)), what + ": dx shadow != bf16(dx)"
        assert bool((sx[..., N:] == FP.NAN16).all()), what + ": padding halfs of the dx shadow were written"
    W_.report(backend, len(HEAD_BWD_SHAPES))


# ---- mh_level_front_fwd / _planes / _head_fwd ---------------------------------------------------------------------------------------------------
def _level_front_shapes():
    r = _rng("level_front")
    out = [(1, 1, 1, 4, 0, 1, 4, 1, 1, 1, 1), (2, 13, 70, 32, 2, 0, 32, 7, 35, 7, 35)]          # one pixel; several workgroups per row, H = 2 Hc - 1
    i = len(out)
    while len(out) < 40:
        B, H, W = r.randint(1, 2), r.randint(1, 13), r.randint(1, 70)
        Cc, md, K = r.choice([4, 16, 20, 32, 64, 96, 128]), r.randint(0, 4), r.choice([4, 8, 16, 32])
        Hc, Wc = r.randint(1, H), r.randint(1, W)            # the head form: up-scaling only
        if i % 5 == 0:
            Hc, Wc = (H + 1) // 2, (W + 1) // 2
        if i % 7 == 0:
            Hc, Wc = H, W
        if i % 9 == 0 and H % 2 == 0:
            Hc = H // 2                                     # two fine rows per workgroup
        Hp, Wp = r.randint(1, 2 * H), r.randint(1, 2 * W)    # the plain / planes forms: down-scaling too
        out.append((B, H, W, Cc, md, i % 2, K, Hc, Wc, Hp, Wp))
        i += 1
    return out


LEVEL_FRONT_SHAPES = _level_front_shapes()


def _front_check(W_, what, tag, mul, md, L, R, Vc_k, u_k, Rw_k, out, Cc, D, zero_tail, Vc_ref):
    """the stages of one launch, each against the float64 oracle of that stage applied to the kernel's own previous stage (its own rounding only: FWD);
    then end to end against the oracle chain from Vc_ref (bound of tests/test_ops_parity.py: 1e-5 + 32 |du|).  All tensors on the CPU."""
    B, H, W = u_k.shape
    u_st = mul * T.resize_bilinear(Vc_k.double()[..., None], H, W)[..., 0]
    W_.check(what, tag + " u", u_k, u_st, FWD)
    W_.check(what, tag + " Rw", Rw_k, T.linear_warp(R.double(), u_k.double()[..., None]), FWD)
    W_.check(what, tag + " vol", out[..., Cc:Cc + D], T.correlation(L.double(), Rw_k.double(), md, 1), FWD)
    assert torch.equal(FP.bits(out[..., :Cc]), FP.bits(L)), what + ": out[..., :C] != L"
    assert torch.equal(FP.bits(out[..., Cc + D]), FP.bits(u_k)), what + ": the disparity channel != u"
    tb = FP.bits(out[..., Cc + D + 1:])
    assert bool((tb == (0 if zero_tail else FP.NAN32)).all()), what + ": tail channels"
    # end to end
    u_o = mul * T.resize_bilinear(Vc_ref.double()[..., None], H, W)[..., 0]
    Rw_o = T.linear_warp(R.double(), u_o[..., None])
    vol_o = T.correlation(L.double(), Rw_o, md, 1)
    dv = (Vc_k.double() - Vc_ref.double()).abs().max().item()
    du = (u_k.double() - u_o).abs().max().item()
    eR, eV = (Rw_k.double() - Rw_o).abs().max().item(), (out[..., Cc:Cc + D].double() - vol_o).abs().max().item()
    # The bound |du| x the steepest |R[x + 1] - R[x]| (<= 32) is a Lipschitz bound in the warp COORDINATE, and the kernel evaluates that as cx = fl32(x + u),
    # the float32 coordinates of the reference graph, while the oracle chain adds in float64: half an ulp of cx (3.8e-6 at x = 64 .. 127) comes on top of the
    # error of u itself wherever x + u is no float32 number.  |du| below is therefore the error of cx as evaluated, not of u alone.
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    dc = ((xs + u_k).double() - (xs.double() + u_o)).abs().max().item()
    for key, e in (("u", du), ("cx", dc), ("Rw", eR), ("vol", eV)):
        key = "%s end-to-end %s" % (tag, key)
        W_.w[key] = max(W_.w.get(key, 0.0), e)
    assert du <= 1e-5 + 4.0 * abs(mul) * dv, "%s: end-to-end u error %.3g (Vc error %.3g)" % (what, du, dv)
    assert eR <= 1e-5 + 32.0 * dc and eV <= 1e-5 + 32.0 * dc, "%s: end-to-end Rw error %.3g, volume error %.3g at u error %.3g, coordinate error %.3g" % (what, eR, eV, du, dc)


def _front_planes_check(what, out, ghi, glo, B, H, W, n, pld):
    hi = ghi.payload_bits().view(B, H, W, pld)
    ghi.assert_guards(what + ": hi plane")
    assert torch.equal(hi[..., :n], _bf16_bits(out[..., :n])), what + ": hi plane != bf16(out)"
    assert bool((hi[..., n:] == FP.NAN16).all()), what + ": padding halfs of the hi plane were written"
    if glo is not None:
        lo = glo.payload_bits().view(B, H, W, pld)
        glo.assert_guards(what + ": lo plane")
        hif = hi[..., :n].contiguous().view(torch.bfloat16).float()
        assert torch.equal(lo[..., :n], _bf16_bits(out[..., :n] - hif)), what + ": lo plane != bf16(out - hi)"
        assert bool((lo[..., n:] == FP.NAN16).all()), what + ": padding halfs of the lo plane were written"


def test_level_front_sweep(backend):
    """mh_level_front_fwd, _planes and _head_fwd against float64, stage by stage (Vc = conv2d(X, hw) + hb; u = mul * resize_bilinear(Vc); Rw =
    linear_warp(R, u); volume = correlation(L, Rw)) and end to end: C = 4 .. 128, D = 1 .. 9, H x W from one pixel to several workgroups per row, the tail
    zero-filled or left alone.  Head form: ANY up-scaling geometry Hc <= H, Wc <= W the entry point says it serves (every coarse pixel stored), one and two
    fine rows per workgroup storing the same bits; plain / planes forms: down-scaling too.  Planes: hi = bf16(out), lo = bf16(out - hi) bit for bit."""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_level_front_fwd/_planes/_head_fwd")
    skipped, rows2 = 0, 0
    for k, shp in enumerate(LEVEL_FRONT_SHAPES):
        B, H, W, Cc, md, zero_tail, K, Hc, Wc, Hp, Wp = shp
        D = 2 * md + 1
        ld = FP.round_up(Cc + D + 1, 4) + 4
        pld = FP.round_up(Cc + D + 1, 32)
        mul = [2.5, 5.0, 1.25, 0.625][k % 4]
        L, R = _rand((B, H, W, Cc), 9000 + 10 * k), _rand((B, H, W, Cc), 9001 + 10 * k)
        Ld, Rd = L.to(dev), R.to(dev)

        def launch(form, Vc_in=None, X=None, hw=None, hb=None, hc=0, wc=0, planes=0):
            """-> (Vc, u, Rw, out) on the CPU and the plane buffers, after the footprint checks"""
            what = "shape %d %s %s" % (k, shp, form)
            gu, u = _out(dev, (B, H, W)); gr, Rw = _out(dev, (B, H, W, Cc)); go, out = _out(dev, (B, H, W, ld))
            ghi = _i16(dev, B * H * W * pld) if planes else None
            glo = _i16(dev, B * H * W * pld) if planes == 2 else None
            php, plp = (C.c_void_p(ghi.ptr()) if ghi else None), (C.c_void_p(glo.ptr()) if glo else None)
            common = (mul, ops._p(Ld), Cc, ops._p(Rd), Cc, ops._p(out), ld, Cc, ops._p(Rw), Cc, ops._p(u), B, H, W, Cc, md, zero_tail)
            gv = None
            if form == "head":
                gv, Vc = _out(dev, (B, hc, wc))
                lib.level_front_head_fwd(ops._p(X), K, K, ops._p(hw), ops._p(hb), ops._p(Vc), hc, wc, *(common + (php, plp, pld if planes else 0, None)))
            elif form == "planes":
                Vc = Vc_in
                lib.level_front_fwd_planes(ops._p(Vc), hc, wc, *(common + (php, plp, pld, None)))
            else:
                Vc = Vc_in
                lib.level_front_fwd(ops._p(Vc), hc, wc, *(common + (None,)))
            name = _kernel(lib)
            backend.sync()
            what = "%s -> %s" % (what, name)
            assert "level_front_kernel" in name and ("HEAD=%d" % K in name) == (form == "head"), what
            if gv is not None:
                FP.assert_fully_written(gv, gv.n, what + ": Vc")
            FP.assert_fully_written(gu, gu.n, what + ": u"); FP.assert_fully_written(gr, gr.n, what + ": Rw"); go.assert_guards(what + ": out")
            o = out.cpu()
            if planes:
                _front_planes_check(what, o, ghi, glo, B, H, W, Cc + D + 1, pld)
            return what, Vc.cpu(), u.cpu(), Rw.cpu(), o

        # plain and planes: Vc is an input, any geometry
        Vp = _rand((B, Hp, Wp), 9002 + 10 * k, 1.5)
        Vpd = Vp.to(dev)
        what, _, u1, Rw1, o1 = launch("plain", Vc_in=Vpd, hc=Hp, wc=Wp)
        _front_check(W_, what, "plain", mul, md, L, R, Vp, u1, Rw1, o1, Cc, D, zero_tail, Vp)
        what, _, u2, Rw2, o2 = launch("planes", Vc_in=Vpd, hc=Hp, wc=Wp, planes=2 - k % 2)
        assert torch.equal(FP.bits(u2), FP.bits(u1)) and torch.equal(FP.bits(Rw2), FP.bits(Rw1)) and torch.equal(FP.bits(o2), FP.bits(o1)), what + ": fp32 outputs differ from the plain form's"
        # the coarser level's head inside the launch
        if lib.level_front_head_ok(Hc, Wc, H, W, Cc, K, md) != 1:
            skipped += 1
            continue
        X, hw = _rand((B, Hc, Wc, K), 9003 + 10 * k), _rand((3, 3, K, 1), 9004 + 10 * k, 0.2)
        hb = _rand((1,), 9005 + 10 * k) if k % 3 else None
        Xd, hwd, hbd = X.to(dev), hw.to(dev), (hb.to(dev) if hb is not None else None)
        what, V3, u3, Rw3, o3 = launch("head", X=Xd, hw=hwd, hb=hbd, hc=Hc, wc=Wc, planes=k % 3)
        Vo = T.conv2d(X.double(), hw.double(), (hb.double() if hb is not None else None), 1, 1, 1.0)[..., 0]
        W_.check(what, "head Vc", V3, Vo, FWD)
        _front_check(W_, what, "head", mul, md, L, R, V3, u3, Rw3, o3, Cc, D, zero_tail, Vo)
        if H == 2 * Hc:
            rows2 += 1
            lib.tune_corr(1 | 8)                             # one fine row per workgroup instead of two: the same bits
            try:
                what, V4, u4, Rw4, o4 = launch("head", X=Xd, hw=hwd, hb=hbd, hc=Hc, wc=Wc)
            finally:
                lib.tune_corr(1)
            assert all(torch.equal(FP.bits(a), FP.bits(b)) for a, b in ((V4, V3), (u4, u3), (Rw4, Rw3), (o4, o3))), what + ": one row per workgroup stores other bits"
    W_.report(backend, len(LEVEL_FRONT_SHAPES))
    print("mh_level_front_head_fwd (%s): %d of %d shapes not served, %d with two rows per workgroup" % (backend.name, skipped, len(LEVEL_FRONT_SHAPES), rows2))
    assert 4 * skipped <= len(LEVEL_FRONT_SHAPES), "%d of %d shapes skipped by mh_level_front_head_ok" % (skipped, len(LEVEL_FRONT_SHAPES))
    assert rows2 >= 1
