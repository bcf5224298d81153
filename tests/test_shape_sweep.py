"""Seeded shape sweeps: one test per op walks a FIXED list of about 40 shapes drawn once from a literal seed (a failure message carries the shape),
every output in a guarded buffer prefilled with NaN (tests/footprint.py), references in float64 (autograd of the float64 oracle for gradients),
tolerances of tests/test_ops_parity.py's _close: rtol 2e-5 forward, 5e-5 gradients.  The hand-picked shapes of the parity tests leave most of the
(size, ratio, channel count, alignment) space unvisited; these lists visit it at sizes of a few hundred elements."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import footprint as FP
from madnet_hip import ops
from oracle import tf_ops as T

SEED = 20240611
FWD, GRAD = 2e-5, 5e-5


def _rng(tag):
    return random.Random("%d/%s" % (SEED, tag))


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _err(got, ref, rtol, atol=2e-6):
    """(within atol + rtol * max(1, |ref|max) ?, relative error) -- _close of tests/test_ops_parity.py against a float64 reference"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    e = (got - ref).abs().max().item() if ref.numel() else 0.0
    return e <= atol + rtol * max(1.0, ref.abs().max().item() if ref.numel() else 0.0), e


class _Worst(object):
    def __init__(self, op):
        self.op, self.w = op, {}

    def check(self, what, key, got, ref, rtol, atol=2e-6):
        ok, e = _err(got, ref, rtol, atol)
        self.w[key] = max(self.w.get(key, 0.0), e)
        assert ok, "%s %s: %s error %.3g" % (self.op, what, key, e)

    def report(self, backend, n):
        print("%s (%s, %d shapes): worst abs error %s" % (self.op, backend.name, n, ", ".join("%s %.3g" % kv for kv in sorted(self.w.items()))))


def _out(dev, shape, prefill=None):
    """a guarded fp32 output of `shape`: (Guarded, tensor view)"""
    n = int(np.prod(shape))
    g = FP.Guarded(n, torch.float32, dev)
    if prefill is not None:
        g.set(prefill)
    return g, g.t.view(*shape)


# ---- mh_resize_fwd / mh_resize_bwd --------------------------------------------------------------------------------------------------------------
def _resize_shapes():
    r = _rng("resize")
    out = []
    for i in range(40):
        Hi, Wi, Hr, Wr = r.randint(1, 12), r.randint(1, 18), r.randint(1, 40), r.randint(1, 60)
        if i % 8 == 0:
            Hr, Wr = Hi, Wi                                    # identity size
        Ho, Wo = r.randint(1, Hr), r.randint(1, Wr)
        cy, cx = r.randint(0, Hr - Ho), r.randint(0, Wr - Wo)
        out.append((r.randint(1, 2), Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, r.choice([1.0, -20.0, 0.625, -1.5]), i % 3, i % 2))
    return out


RESIZE_SHAPES = _resize_shapes()


def _resize_ref(x, Hr, Wr, cy, cx, Ho, Wo, mul, mode):
    xin = x[..., None]
    if mode == 0:
        pre = None
        r = T.resize_bilinear(xin, Hr, Wr) * mul
    elif mode == 1:
        pre = xin * mul
        r = T.resize_bilinear(torch.relu(pre), Hr, Wr)
    else:
        pre = T.resize_bilinear(xin, Hr, Wr) * mul
        r = torch.relu(pre)
    return r[:, cy:cy + Ho, cx:cx + Wo, 0], pre


def test_resize_sweep(backend):
    """mh_resize_fwd / mh_resize_bwd: source 1..12 x 1..18, virtual size 1..40 x 1..60 (up, down, identity, ratios that are no integers, 1-pixel
    sources), random crops, the three modes, four multipliers, accumulate 0 / 1"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_resize_fwd/bwd")
    for k, shp in enumerate(RESIZE_SHAPES):
        B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode, acc = shp
        for attempt in range(20):            # no pre-activation within 1e-4 of the relu's kink: the float32 and float64 masks then agree (decided on the inputs alone)
            x = _rand((B, Hi, Wi), 1000 + 50 * k + attempt)
            xc = x.double().requires_grad_(True)
            ref, pre = _resize_ref(xc, Hr, Wr, cy, cx, Ho, Wo, mul, mode)
            if pre is None or bool((pre.detach().abs() >= 1e-4).all()):
                break
        else:
            raise AssertionError("no unambiguous input for %s" % (shp,))
        g = _rand((B, Ho, Wo), 3000 + k)
        (gx,) = torch.autograd.grad(ref, [xc], g.double())
        old = _rand((B, Hi, Wi), 5000 + k)
        go, out = _out(dev, (B, Ho, Wo))
        gd, dx = _out(dev, (B, Hi, Wi), old if acc else None)
        xd = x.to(dev)
        ops.resize_fwd(lib, xd, out, Hr, Wr, cy, cx, mul, mode)
        ops.resize_bwd(lib, g.to(dev), xd, dx, Hr, Wr, cy, cx, mul, mode, accumulate=bool(acc))
        backend.sync()
        what = "shape %d %s" % (k, shp)
        FP.assert_fully_written(go, go.n, what); FP.assert_fully_written(gd, gd.n, what)
        W_.check(what, "fwd", out, ref, FWD)
        W_.check(what, "bwd", dx, gx + (old.double() if acc else 0), GRAD, atol=1e-5)
    W_.report(backend, len(RESIZE_SHAPES))


# ---- mh_resize_image_fwd / mh_resize_image_bwd --------------------------------------------------------------------------------------------------
def _resize_image_shapes():
    r = _rng("resize_image")
    out = [(1, 1, 1, 3, 5, 7), (2, 1, 6, 1, 4, 3), (1, 7, 1, 4, 2, 9)]            # 1-pixel sources (a column, a row)
    while len(out) < 40:
        out.append((r.randint(1, 2), r.randint(1, 14), r.randint(1, 20), r.randint(1, 4), r.randint(1, 24), r.randint(1, 33)))
    return out


RESIZE_IMAGE_SHAPES = _resize_image_shapes()


def test_resize_image_sweep(backend):
    """mh_resize_image_fwd / _bwd: C = 1..4 interleaved channels, up and down, ratios that are no integers, 1-pixel sources; din is overwritten"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_resize_image_fwd/bwd")
    for k, shp in enumerate(RESIZE_IMAGE_SHAPES):
        B, Hi, Wi, Cc, Ho, Wo = shp
        x = _rand((B, Hi, Wi, Cc), 100 + k)
        xc = x.double().requires_grad_(True)
        ref = T.resize_bilinear(xc, Ho, Wo)
        g = _rand((B, Ho, Wo, Cc), 300 + k)
        (gx,) = torch.autograd.grad(ref, [xc], g.double()) if (Hi, Wi) != (Ho, Wo) else (g.double(),)
        go, out = _out(dev, (B, Ho, Wo, Cc))
        gd, dx = _out(dev, (B, Hi, Wi, Cc))
        lib.resize_image_fwd(ops._p(x.to(dev)), ops._p(out), B, Hi, Wi, Cc, Ho, Wo, None)
        lib.resize_image_bwd(ops._p(g.to(dev)), ops._p(dx), B, Hi, Wi, Cc, Ho, Wo, None)
        backend.sync()
        what = "shape %d %s" % (k, shp)
        FP.assert_fully_written(go, go.n, what); FP.assert_fully_written(gd, gd.n, what)
        W_.check(what, "fwd", out, ref, FWD)
        W_.check(what, "bwd", dx, gx, GRAD, atol=1e-5)
    W_.report(backend, len(RESIZE_IMAGE_SHAPES))


# ---- mh_corr_fwd / mh_corr_bwd ------------------------------------------------------------------------------------------------------------------
def _corr_shapes():
    r = _rng("corr")
    out = [(1, 1, 1, 4, 1, 1, 0), (1, 2, 1, 64, 20, 1, 1), (2, 1, 3, 8, 10, 1, 2), (1, 4, 45, 48, 20, 1, 0)]      # W = 1, W < D
    while len(out) < 40:
        md = r.choice([1, 2, 3, 4, 5, 10, 20])
        st = 2 if (md <= 5 and md % 2 == 0 and r.random() < 0.4) else 1
        out.append((r.randint(1, 2), r.randint(1, 4), r.randint(1, 45), r.choice([4, 8, 16, 32, 48, 64]), md, st, len(out) % 3))
    return out


CORR_SHAPES = _corr_shapes()       # (B, H, W, C, max_disp, stride, form): form 0 = stand-alone volume in a slice, 1 = concat with zero_tail, 2 = concat without


def test_corr_sweep(backend):
    """mh_corr_fwd / mh_corr_bwd: H 1..4, W 1..45 (W < D and W = 1 included), C in {4 .. 64}, max_disp in {1..5, 10, 20}, stride 2 where D <= 9; the
    stand-alone volume stored into a channel slice, the concat form [L | corr | u | tail] with the tail zero-filled or left alone"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_corr_fwd/bwd")
    for k, shp in enumerate(CORR_SHAPES):
        B, H, W, Cc, md, st, form = shp
        L, R, u = _rand((B, H, W, Cc), 10 + k), _rand((B, H, W, Cc), 110 + k), _rand((B, H, W), 210 + k)
        Lc, Rc = L.double().requires_grad_(True), R.double().requires_grad_(True)
        ref = T.correlation(Lc, Rc, md, st)
        D = ref.shape[-1]
        Ld, Rd = L.to(dev), R.to(dev)
        what = "shape %d %s D=%d" % (k, shp, D)
        if form == 0:
            coff, extra = 3, 2
            go, ov = FP.slice_view(dev, B, H, W, D, coff, extra)
            before = go.snapshot()
            lib.corr_fwd(ops._p(Ld), Cc, ops._p(Rd), Cc, None, C.c_void_p(ov.ptr), ov.ld, 0, B, H, W, Cc, md, st, 0, 0, None)
            backend.sync()
            FP.assert_only_slice_written(go, ov, coff, before, what)
            W_.check(what, "fwd", FP.slice_of(go, ov, coff), ref, FWD)
            gcoff, gld = 0, D
        else:
            ld = FP.round_up(Cc + D + 1, 4) + 4            # (the concat form needs 16-byte aligned rows)
            go, out = _out(dev, (B, H, W, ld))
            before = go.snapshot()
            lib.corr_fwd(ops._p(Ld), Cc, ops._p(Rd), Cc, ops._p(u.to(dev)), ops._p(out), ld, Cc, B, H, W, Cc, md, st, 1, int(form == 1), None)
            backend.sync()
            go.assert_guards(what)
            o = out.cpu()
            assert torch.equal(FP.bits(o[..., :Cc]), FP.bits(L)) and torch.equal(FP.bits(o[..., Cc + D]), FP.bits(u)), what
            W_.check(what, "fwd", o[..., Cc:Cc + D], ref, FWD)
            tb = FP.bits(o[..., Cc + D + 1:])
            assert bool((tb == (0 if form == 1 else FP.NAN32)).all()), what + ": tail channels"
            gcoff, gld = Cc, ld
        # gradient: g laid out like the forward buffer
        g = _rand((B, H, W, gld), 310 + k)
        gl, gr = torch.autograd.grad(ref, [Lc, Rc], g.double()[..., gcoff:gcoff + D])
        copy_left = form != 0
        oldl = _rand((B, H, W, Cc), 410 + k)
        acc_l = k % 2
        gdl, dL = _out(dev, (B, H, W, Cc), oldl if acc_l else None)
        gdr, dR = _out(dev, (B, H, W, Cc))
        gdu, du = _out(dev, (B, H, W))
        gv = ops.View(g.to(dev), B, H, W, gld, gld)
        ops.corr_bwd(lib, gv, ops.view(Ld), ops.view(Rd), ops.view(dL), ops.view(dR), md, st, coff=gcoff, du=(du if copy_left else None),
                     acc_l=bool(acc_l), acc_r=False, acc_u=False, copy_left=copy_left, precision=0)
        backend.sync()
        FP.assert_fully_written(gdl, gdl.n, what); FP.assert_fully_written(gdr, gdr.n, what)
        W_.check(what, "dL", dL, gl + (g.double()[..., :Cc] if copy_left else 0) + (oldl.double() if acc_l else 0), GRAD)
        W_.check(what, "dR", dR, gr, GRAD)
        if copy_left:
            FP.assert_fully_written(gdu, gdu.n, what)
            assert torch.equal(FP.bits(du), FP.bits(g[..., Cc + D].contiguous())), what + ": du"
        else:
            FP.assert_untouched(gdu, gdu.snapshot() * 0 + FP.NAN32, what)
    W_.report(backend, len(CORR_SHAPES))


# ---- mh_warp_fwd / mh_warp_bwd ------------------------------------------------------------------------------------------------------------------
def _warp_shapes():
    r = _rng("warp")
    return [(r.randint(1, 2), r.randint(1, 5), r.randint(1, 40), r.choice([4, 16, 20, 128])) for _ in range(36)] + [(1, 1, 1, 4), (1, 2, 2, 20), (2, 1, 3, 16), (1, 3, 1, 128)]


WARP_SHAPES = _warp_shapes()


def _coords(B, H, W, seed, lo, hi):
    """coordinates offsets on a 2^-8 grid (x + u is exact in float32 and float64 alike) with the special cases of the first and last column: integral,
    +-0.5, far outside"""
    g = torch.Generator().manual_seed(seed)
    u = torch.round((torch.rand(B, H, W, generator=g) * (hi - lo) + lo) * 256) / 256
    special = [0.0, 1.0, -1.0, 0.5, -0.5, 100.0, -100.0, float(W), -float(W)]
    for y in range(H):
        u[0, y, 0] = special[y % len(special)]
        u[0, y, W - 1] = special[(y + 3) % len(special)]
    return u


def test_warp_sweep(backend):
    """mh_warp_fwd / mh_warp_bwd: C in {4, 16, 20, 128}, W down to 1, integral / +-0.5 / far-out coordinates on the first and last column; the output
    into a channel slice, dimg accumulated onto an earlier contribution (atomics), du accumulated or overwritten"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_warp_fwd/bwd")
    for k, shp in enumerate(WARP_SHAPES):
        B, H, W, Cc = shp
        img, u = _rand((B, H, W, Cc), 20 + k), _coords(B, H, W, 120 + k, -6.0, 6.0)
        ic, uc = img.double().requires_grad_(True), u.double()[..., None].requires_grad_(True)
        ref = T.linear_warp(ic, uc)
        g = _rand((B, H, W, Cc), 220 + k)
        gi, gu = torch.autograd.grad(ref, [ic, uc], g.double())
        imd, ud = img.to(dev), u.to(dev)
        go, ov = FP.slice_view(dev, B, H, W, Cc, 4, 4)
        before = go.snapshot()
        ops.warp_fwd(lib, ops.view(imd), ud, ov)
        oldi, oldu = _rand((B, H, W, Cc), 320 + k), _rand((B, H, W), 420 + k)
        acc_u = k % 2
        gdi, dimg = _out(dev, (B, H, W, Cc), oldi)
        gdu, du = _out(dev, (B, H, W), oldu if acc_u else None)
        ops.warp_bwd(lib, ops.view(g.to(dev)), ops.view(imd), ud, ops.view(dimg), du=du, acc_u=bool(acc_u))
        backend.sync()
        what = "shape %d %s" % (k, shp)
        FP.assert_only_slice_written(go, ov, 4, before, what)
        gdi.assert_guards(what); FP.assert_fully_written(gdu, gdu.n, what)
        W_.check(what, "fwd", FP.slice_of(go, ov, 4), ref, FWD)
        W_.check(what, "dimg", dimg, gi + oldi.double(), GRAD)
        W_.check(what, "du", du, gu[..., 0] + (oldu.double() if acc_u else 0), GRAD, atol=2e-5)
    W_.report(backend, len(WARP_SHAPES))


# ---- mh_bilinear_sampler_fwd / _bwd -------------------------------------------------------------------------------------------------------------
def _sampler_shapes():
    r = _rng("sampler")
    return [(r.randint(1, 2), r.randint(1, 9), r.randint(1, 14), r.randint(1, 4), r.randint(1, 9), r.randint(1, 17)) for _ in range(38)] + [(1, 1, 1, 3, 2, 2), (2, 1, 5, 1, 1, 1)]


SAMPLER_SHAPES = _sampler_shapes()


def test_bilinear_sampler_sweep(backend):
    """mh_bilinear_sampler_fwd / _bwd: source and target sizes independent (1 x 1 included), C = 1..4, coordinates on a 2^-8 grid reaching outside the
    source on every side (border clamp, un-masked weights); dimgs accumulated with atomics onto zeros, dcoords overwritten"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_bilinear_sampler_fwd/bwd")
    for k, shp in enumerate(SAMPLER_SHAPES):
        B, Hs, Ws, Cc, Ht, Wt = shp
        gen = torch.Generator().manual_seed(30 + k)
        img = _rand((B, Hs, Ws, Cc), 130 + k)
        cx = torch.round((torch.rand(B, Ht, Wt, generator=gen) * (Ws + 3) - 2) * 256) / 256
        cy = torch.round((torch.rand(B, Ht, Wt, generator=gen) * (Hs + 3) - 2) * 256) / 256
        co = torch.stack([cx, cy], -1).contiguous()
        ic, cc = img.double().requires_grad_(True), co.double().requires_grad_(True)
        ref = T.bilinear_sampler(ic, cc)
        g = _rand((B, Ht, Wt, Cc), 230 + k)
        gi, gc = torch.autograd.grad(ref, [ic, cc], g.double())
        go, out = _out(dev, (B, Ht, Wt, Cc))
        gdc, dco = _out(dev, (B, Ht, Wt, 2))
        gdi, dimg = _out(dev, (B, Hs, Ws, Cc), torch.zeros(B, Hs, Ws, Cc))
        imd, cd = img.to(dev), co.to(dev)
        lib.bilinear_sampler_fwd(ops._p(imd), ops._p(cd), ops._p(out), B, Hs, Ws, Cc, Ht, Wt, None)
        lib.bilinear_sampler_bwd(ops._p(g.to(dev)), ops._p(imd), ops._p(cd), ops._p(dco), ops._p(dimg), B, Hs, Ws, Cc, Ht, Wt, None)
        backend.sync()
        what = "shape %d %s" % (k, shp)
        FP.assert_fully_written(go, go.n, what); FP.assert_fully_written(gdc, gdc.n, what); gdi.assert_guards(what)
        W_.check(what, "fwd", out, ref, FWD)
        W_.check(what, "dimgs", dimg, gi, GRAD)
        W_.check(what, "dcoords", dco, gc, GRAD, atol=2e-5)
    W_.report(backend, len(SAMPLER_SHAPES))


# ---- mh_pad_reflect -----------------------------------------------------------------------------------------------------------------------------
def _pad_shapes():
    r = _rng("pad")
    out = []
    while len(out) < 40:
        B, H, W, Cc = r.randint(1, 2), r.randint(2, 11), r.randint(2, 14), r.randint(1, 4)
        pt, pl = r.randint(0, H - 1), r.randint(0, W - 1)           # reflection depth up to size - 1
        pb, pr = r.randint(0, H - 1), r.randint(0, W - 1)
        if len(out) % 5 == 0:
            pt, pb = H - 1, H - 1
        ld = r.choice([4, 8])
        div, sub = r.choice([(1.0, 0.0), (255.0, 100.0 / 255.0)])
        out.append((B, H, W, Cc, H + pt + pb, W + pl + pr, pt, pl, ld, div, sub))
    return out


PAD_SHAPES = _pad_shapes()


def test_pad_reflect_sweep(backend):
    """mh_pad_reflect: C = 1..4 into rows of 4 / 8 floats (extra channels zero), reflection depth up to size - 1 on every side, odd and even padded
    sizes, x / div - sub.  div = 1, sub = 0 is an index operation: bit-exact; otherwise one division and one subtraction in fp32 (1e-6)."""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_pad_reflect")
    assert any(s[4] % 2 for s in PAD_SHAPES) and any(s[4] % 2 == 0 for s in PAD_SHAPES)
    for k, shp in enumerate(PAD_SHAPES):
        B, H, W, Cc, Hp, Wp, pt, pl, ld, div, sub = shp
        x = torch.floor(torch.rand(B, H, W, Cc, generator=torch.Generator().manual_seed(40 + k)) * 256)
        refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
        iy, ix = refl(np.arange(Hp) - pt, H), refl(np.arange(Wp) - pl, W)
        ref = x.double()[:, iy][:, :, ix]
        if (div, sub) != (1.0, 0.0):
            ref = ref / float(np.float32(div)) - float(np.float32(sub))
        go, out = _out(dev, (B, Hp, Wp, ld))
        lib.pad_reflect(ops._p(x.to(dev)), ops._p(out), B, H, W, Cc, Hp, Wp, pt, pl, ld, div, sub, None)
        backend.sync()
        what = "shape %d %s" % (k, shp)
        FP.assert_fully_written(go, go.n, what)
        o = out.cpu()
        assert bool((FP.bits(o[..., Cc:]) == 0).all()), what + ": the extra channels must hold zeros"
        if (div, sub) == (1.0, 0.0):
            assert torch.equal(o[..., :Cc].double(), ref), what
        W_.check(what, "out", o[..., :Cc], ref, 1e-6, atol=0.0)
    W_.report(backend, len(PAD_SHAPES))


# ---- elementwise ops: both the 16-byte and the scalar kernels ---------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 255, 256, 1023, 1025]
OFFSETS = [0, 1, 2]                       # floats: pointers 0 / 4 / 8 bytes off a 16-byte boundary


def _at(g, off):
    return C.c_void_p(g.ptr(off))


def _flat(dev, n, off, values=None, dtype=torch.float32):
    """a guarded buffer whose n live elements start `off` elements into the payload; the elements in front of them are live neighbours (sentinel)"""
    g = FP.Guarded(n + off, dtype, dev)
    if values is not None:
        g.t[off:] = values.to(dev)
    return g


def _only(g, off, n, what):
    """guards intact, the `off` elements in front of the live range untouched"""
    g.assert_guards(what)
    assert bool((g.payload_bits()[:off] == g.fill).all()), what + ": elements in front of the range were written"
    return g.t[off:off + n].cpu()


def test_elementwise_sweep(backend):
    """mh_u8_to_f32, mh_fetch_inputs, mh_momentum, mh_adam, mh_copy_channels, mh_leaky_bwd, mh_fill at n in {1, 3, 4, 5, 255, 256, 1023, 1025} with every
    pointer 0 / 4 / 8 bytes off a 16-byte boundary (the float4 and the scalar twins).  Conversions, fills and the single multiplication of leaky_bwd are
    bit-equal to the host's fp32; the multiply-add chains are within 1e-6 of float64."""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("elementwise")
    table = ops.InputTable(lib, dev)
    for n in SIZES:
        for off in OFFSETS:
            what = "n=%d offset=%d bytes" % (n, 4 * off)
            seed = 7 * n + off
            # mh_u8_to_f32 (the source one / two BYTES off as well)
            src8 = torch.randint(0, 256, (n + off,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
            s8 = src8.to(dev)
            g = _flat(dev, n, off)
            lib.u8_to_f32(C.c_void_p(s8.data_ptr() + off), _at(g, off), n, None)
            backend.sync()
            assert torch.equal(_only(g, off, n, "u8_to_f32 " + what), src8[off:].float()), "u8_to_f32 " + what
            # mh_fetch_inputs: an 8-bit and a float32 source, one entry left alone
            f32 = _rand((n,), seed + 1)
            fsrc = _flat(dev, n, off, f32)
            g0, g1, g2 = _flat(dev, n, off), _flat(dev, n, (off + 1) % 3), _flat(dev, n, off)
            table.tab.src[0], table.tab.u8[0] = s8.data_ptr() + off, 1
            table.tab.src[1], table.tab.u8[1] = fsrc.ptr(off), 0
            table.tab.src[2], table.tab.u8[2] = None, 0
            dp = (C.c_void_p * 3)(g0.ptr(off), g1.ptr((off + 1) % 3), g2.ptr(off))
            cnt = (C.c_int64 * 3)(n, n, n)
            lib.fetch_inputs(C.c_void_p(table.ptr), dp, cnt, 3, None)
            backend.sync()
            assert torch.equal(_only(g0, off, n, "fetch u8 " + what), src8[off:].float()), "fetch_inputs u8 " + what
            assert torch.equal(FP.bits(_only(g1, (off + 1) % 3, n, "fetch f32 " + what)), FP.bits(f32)), "fetch_inputs f32 " + what
            FP.assert_untouched(g2, g2.snapshot() * 0 + FP.NAN32, "fetch_inputs NULL entry " + what)
            # mh_fill
            g = _flat(dev, n, off)
            lib.fill(_at(g, off), n, 1.25, None)
            backend.sync()
            assert bool((_only(g, off, n, "fill " + what) == 1.25).all()), "fill " + what
            # mh_momentum: accum = momentum * accum + grad_scale * g ; var -= lr * accum
            w, m, gr = _rand((n,), seed + 2), _rand((n,), seed + 3), _rand((n,), seed + 4)
            gw, gm, gg = _flat(dev, n, off, w), _flat(dev, n, off, m), _flat(dev, n, off, gr)
            lr, mom, gs = 1e-2, 0.9, 0.5
            lib.momentum(_at(gw, off), _at(gm, off), _at(gg, off), n, lr, mom, gs, None)
            backend.sync()
            f = lambda v: float(np.float32(v))
            m_ref = f(mom) * m.double() + f(gs) * gr.double()
            W_.check(what, "momentum accum", _only(gm, off, n, "momentum " + what), m_ref, 1e-6, atol=0.0)
            W_.check(what, "momentum var", _only(gw, off, n, "momentum " + what), w.double() - f(lr) * m_ref, 1e-6, atol=0.0)
            # mh_adam
            w, m, v, gr = _rand((n,), seed + 5), _rand((n,), seed + 6, 0.1), _rand((n,), seed + 7, 0.1).abs(), _rand((n,), seed + 8, 0.3)
            gw, gm, gv, gg = _flat(dev, n, off, w), _flat(dev, n, off, m), _flat(dev, n, off, v), _flat(dev, n, off, gr)
            state = torch.tensor([0.9 ** 3, 0.999 ** 3], dtype=torch.float32)
            b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-3
            lib.adam(_at(gw, off), _at(gm, off), _at(gv, off), _at(gg, off), n, ops._p(state.to(dev)), lr, b1, b2, eps, 1.0, None)
            backend.sync()
            s0, s1 = float(state[0]), float(state[1])
            lr_t = f(lr) * np.sqrt(1.0 - s1) / (1.0 - s0)
            m_ref = f(b1) * m.double() + (1.0 - f(b1)) * gr.double()
            v_ref = f(b2) * v.double() + (1.0 - f(b2)) * gr.double() ** 2
            W_.check(what, "adam m", _only(gm, off, n, "adam " + what), m_ref, 1e-6, atol=0.0)
            W_.check(what, "adam v", _only(gv, off, n, "adam " + what), v_ref, 1e-6, atol=0.0)
            W_.check(what, "adam var", _only(gw, off, n, "adam " + what), w.double() - lr_t * m_ref / (v_ref.sqrt() + f(eps)), 1e-6, atol=0.0)
            # mh_copy_channels: n pixels of 3 channels from rows of 5 into a slice of rows of 7, scaled, accumulating or not
            for acc in (0, 1):
                src, old = _rand((n, 5), seed + 9), _rand((n, 7), seed + 10)
                gs_, gd_ = _flat(dev, n * 5, off, src.reshape(-1)), _flat(dev, n * 7, off, old.reshape(-1))
                before = gd_.snapshot()
                lib.copy_channels(_at(gs_, off + 1), 5, _at(gd_, off + 2), 7, n, 3, 2.0, acc, None)
                backend.sync()
                got = _only(gd_, off, n * 7, "copy_channels " + what).view(n, 7)
                exp = old.double().clone()
                exp[:, 2:5] = 2.0 * src.double()[:, 1:4] + (old.double()[:, 2:5] if acc else 0)
                W_.check(what, "copy_channels", got[:, 2:5], exp[:, 2:5], 1e-6, atol=0.0)
                keepcols = [0, 1, 5, 6]
                assert torch.equal(FP.bits(got[:, keepcols].contiguous()), FP.bits(old[:, keepcols].contiguous())), "copy_channels wrote a neighbour: " + what
            # mh_leaky_bwd: dy *= (y > 0 ? 1 : alpha) on a 3-channel slice of rows of 7 / 5
            dy, y = _rand((n, 7), seed + 11), _rand((n, 5), seed + 12)
            y[0, 1] = 0.0                              # y == 0 takes the slope
            gdy, gy = _flat(dev, n * 7, off, dy.reshape(-1)), _flat(dev, n * 5, off, y.reshape(-1))
            lib.leaky_bwd(_at(gdy, off + 2), 7, _at(gy, off + 1), 5, n, 3, 0.2, None)
            backend.sync()
            got = _only(gdy, off, n * 7, "leaky_bwd " + what).view(n, 7)
            exp = dy.clone()
            exp[:, 2:5] = dy[:, 2:5] * torch.where(y[:, 1:4] > 0, torch.tensor(1.0), torch.tensor(0.2))
            assert torch.equal(FP.bits(got), FP.bits(exp)), "leaky_bwd " + what
    W_.report(backend, len(SIZES) * len(OFFSETS))
