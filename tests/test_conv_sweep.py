"""Seeded float64 sweeps of the convolution entry points (csrc/conv.hip, conv_patch.hip, conv_rows.hip, conv_planes.hip), in the manner of
tests/test_shape_sweep.py: every list is FIXED, drawn once at import from the literal seed of that file (its _rng); every result goes into a channel slice of a guarded buffer
prefilled with NaN (tests/footprint.py) and is checked on bits outside the slice; the channel padding of every input row holds NaN; references are
the float64 oracle (autograd for the gradients) on operands rounded the way the kernel that ran (mh_last_kernel) rounds them.  The dispatch is
host code, identical on both backends: the generators are fitted to each family's eligibility rule and every launch asserts the family it was built
to reach.  No shape is skipped or dropped at run time.

Bounds, relative to max(1, |ref|max): exact fp32 2e-5; bf16 kernels against bf16-rounded operands 1e-4; split-bf16 against the unrounded oracle 4e-5
(tests/test_conv_parity.py); plane kernels 3e-5 forward / 2e-5 input gradient in bf16 (tests/test_conv_planes.py); filter gradient 1e-4 / 2e-4."""
import ctypes as C

import torch

import footprint as FP
from madnet_hip import ops
from oracle import tf_ops as T
from test_shape_sweep import _Worst as _WorstAbs, _rand, _rng

NAN = float("nan")
_bf, _wide = FP.bf16_round, FP.wide_rows


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ld(c):
    return FP.round_up(c, 4) if c > 1 else 1


class _Worst(_WorstAbs):
    """_Worst of tests/test_shape_sweep.py with RELATIVE errors: check() asserts finite values and err <= rtol * max(1, |ref|max)"""

    def check(self, what, key, got, ref, rtol):
        got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
        assert torch.isfinite(got).all(), "%s %s: %s holds %d non-finite values" % (self.op, what, key, int((~torch.isfinite(got)).sum()))
        e = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        self.w[key] = max(self.w.get(key, 0.0), e)
        assert e <= rtol, "%s %s: %s relative error %.3g > %.3g" % (self.op, what, key, e, rtol)

    def report(self, backend, n):
        print("%s (%s, %d shapes): worst relative error %s" % (self.op, backend.name, n, ", ".join("%s %.3g" % kv for kv in sorted(self.w.items()))))


def _tolerance(name):
    """(operands rounded to bf16 in the oracle?, relative bound, key) by the arithmetic of the kernel that ran (test_conv_footprint._tolerance)"""
    fam = name.split("<")[0].split(" ")[0]
    if "bf16x3" in name:
        return False, 4e-5, fam + " bf16x3"
    if "bf16" in name or "conv_thin_kernel" in name:
        return True, 1e-4, fam + " bf16"
    return False, 2e-5, fam + " fp32"


class Layer(object):
    """One 'SAME' conv layer x [B,H,W,Ci] -> y [B,Ho,Wo,Co] (HWIO weights [k,k,Ci,Co]) and the float64 oracles of its forward pass (mode 0) and its
    input gradient (mode 1, operand dz [B,Ho,Wo,Co]), cached per operand rounding.  In mode 1 the descriptor's K is Co and its N is Ci."""

    def __init__(self, seed, B, H, W, Ci, Co, k, stride, dil, wscale=0.2):
        self.B, self.H, self.W, self.Ci, self.Co, self.k, self.stride, self.dil = B, H, W, Ci, Co, k, stride, dil
        self.Ho, self.Wo, self.pt, self.pl = ops.conv_geometry(H, W, k, k, stride, dil)
        self.w = _rand((k, k, Ci, Co), seed, wscale)
        self.x = _rand((B, H, W, Ci), seed + 1)
        self.dz = _rand((B, self.Ho, self.Wo, Co), seed + 2)
        self.bias = {0: _rand((Co,), seed + 3), 1: _rand((Ci,), seed + 3)}
        self.mask = {0: _rand((B, self.Ho, self.Wo, Co), seed + 4), 1: _rand((B, H, W, Ci), seed + 4)}
        self.old = {0: _rand((B, self.Ho, self.Wo, Co), seed + 5), 1: _rand((B, H, W, Ci), seed + 5)}
        self._ref, self._dev = {}, {}

    def shape(self):
        return (self.B, self.H, self.W, self.Ci, self.Co, self.k, self.stride, self.dil)

    def core(self, mode, rounded):
        """float64 conv2d(x, w) (mode 0) / conv2d_backprop_input(dz, w) (mode 1), no bias, no activation"""
        key = (mode, rounded)
        if key not in self._ref:
            rd = _bf if rounded else (lambda t: t)
            w = rd(self.w).double()
            if mode == 0:
                r = T.conv2d(rd(self.x).double(), w, None, stride=self.stride, dilation=self.dil, alpha=1.0)
            else:
                xin = torch.zeros(self.B, self.H, self.W, self.Ci, dtype=torch.float64, requires_grad=True)
                (r,) = torch.autograd.grad(T.conv2d(xin, w, None, stride=self.stride, dilation=self.dil, alpha=1.0), xin, rd(self.dz).double())
            self._ref[key] = r.detach()
        return self._ref[key]

    def expected(self, mode, rounded, bias, alpha, mask, acc, mask_alpha=0.2):
        """(leaky(core + bias, alpha) + old) * leaky'(mask): mask = None | (c0, c1) with (0, 0) = every channel"""
        r = self.core(mode, rounded)
        if bias:
            r = r + self.bias[mode].double()
        r = T.leaky(r, alpha)
        if acc:
            r = r + self.old[mode].double()
        if mask is not None:
            m = torch.where(self.mask[mode].double() > 0, 1.0, mask_alpha)
            if mask != (0, 0):
                m[..., :mask[0]] = 1.0
                m[..., mask[1]:] = 1.0
            r = r * m
        return r

    def wgrad_ref(self, rounded):
        key = ("w", rounded)
        if key not in self._ref:
            rd = _bf if rounded else (lambda t: t)
            w0 = torch.zeros(self.k, self.k, self.Ci, self.Co, dtype=torch.float64, requires_grad=True)
            (gw,) = torch.autograd.grad(T.conv2d(rd(self.x).double(), w0, None, stride=self.stride, dilation=self.dil, alpha=1.0), [w0], rd(self.dz).double())
            self._ref[key] = gw
        return self._ref[key]

    def dev(self, what, dev, make):
        if (what, dev) not in self._dev:
            self._dev[(what, dev)] = make()
        return self._dev[(what, dev)]


def launch(backend, L, mode, prec, coff=4, extra=4, xextra=0, bias=False, alpha=1.0, mask=None, acc=False, pad=0, bank=None):
    """One mh_conv2d_wb launch of layer L into channels [coff, coff + N) of rows of coff + N + extra floats inside a guarded NaN buffer -> (kernel name,
    what, result [B,Ho,Wo,N] on the CPU).  Asserts the return code and the store footprint: guards and neighbours bit-untouched, every element of the
    slice written.  pad: the padded-row form of an input gradient (ConvArgs::vecCpad, the patch-staged kernel): that many columns behind the slice
    must hold +0.0 after the launch -- stored by a plain launch, kept by an accumulating one (they hold zeros in front of it)."""
    lib, dev = backend.lib, backend.device
    K, N = (L.Ci, L.Co) if mode == 0 else (L.Co, L.Ci)
    Hi, Wi, Ho, Wo = (L.H, L.W, L.Ho, L.Wo) if mode == 0 else (L.Ho, L.Wo, L.H, L.W)
    src = L.x if mode == 0 else L.dz
    ild = _ld(K) + xextra
    x = L.dev(("in", mode, ild), dev, lambda: _wide(src, ild, dev))
    w = L.dev("w", dev, lambda: L.w.to(dev))
    b = L.dev(("bias", mode), dev, lambda: L.bias[mode].to(dev)) if bias else None
    mk = L.dev(("mask", mode), dev, lambda: _wide(L.mask[mode], _ld(N), dev, fill=0.0)) if mask is not None else None
    g, ov = FP.slice_view(dev, L.B, Ho, Wo, N, coff, extra, prefill=(L.old[mode] if acc else None))
    if pad and acc:
        g.t.view(L.B, Ho, Wo, ov.ld)[..., coff + N:coff + N + pad] = 0.0          # (what the first contribution left there: the sum must keep the zeros)
    c0, c1 = mask if mask is not None else (0, 0)
    d = ops.conv_desc(L.B, Hi, Wi, Ho, Wo, K, N, L.k, L.k, L.stride, L.dil, L.pt, L.pl, mode, mode, ild, ov.ld, mask_ld=(_ld(N) if mask is not None else 0),
                      accumulate=int(acc), alpha=alpha, mask_alpha=0.2, mask_c0=c0, mask_c1=c1, precision=prec)
    before = g.snapshot()
    rc = lib._raw_mh_conv2d_wb(C.byref(d), P(x), P(w), P(bank), P(b), C.c_void_p(ov.ptr), P(mk), None)
    name = lib.last_kernel().decode() if rc == 0 else "-"
    backend.sync()
    what = "%s mode=%d prec=%d coff=%d extra=%d xextra=%d bias=%d alpha=%g mask=%s acc=%d [%s]" % (L.shape(), mode, prec, coff, extra, xextra, bias, alpha, mask, acc, name)
    assert rc == 0, (what, lib.last_error())
    if pad:
        assert "conv_patch_kernel" in name, what + ": the padded-row form belongs to the patch-staged kernel"
    FP.assert_only_slice_written(g, ov, coff, before, what, zero_cols=pad)
    return name, what, FP.slice_of(g, ov, coff)


def check(W_, L, mode, name, what, got, bias, alpha, mask, acc, family):
    """the family assertion and the value check of one launch"""
    for sub in ((family,) if isinstance(family, str) else family):
        assert sub in name, "%s: expected %s" % (what, family)
    rounded, tol, key = _tolerance(name)
    W_.check(what, key + (" dgrad" if mode else " fwd"), got, L.expected(mode, rounded, bias, alpha, mask, acc), tol)


def _variant(r, N, mode):
    """randomised epilogue: (bias, alpha, mask, accumulate) -- bias or none, alpha 1 or 0.2 (forward), mask over every channel / a sub-range / none"""
    mk = r.choice([None, None, (0, 0), "sub"])
    if mk == "sub":
        c0 = r.randint(0, max(0, N - 1))
        mk = (c0, r.randint(c0 + 1, N)) if N > 1 else (0, 0)
        if mk == (0, N):
            mk = (0, 0)
    return (bool(r.getrandbits(1)) if mode == 0 else False), (r.choice([1.0, 0.2]) if mode == 0 else 1.0), mk, bool(r.getrandbits(1))


# ---- 1. the default dispatch ----------------------------------------------------------------------------------------------------------------------
CHANNELS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 20, 31, 32, 33, 36, 38, 63, 64, 65, 70, 100]
MAC_BUDGET = 16e6                      # taps * Cin * Cout * output pixels of one shape (emulator time)


def _default_shapes():
    """(B, H, W, Cin, Cout, k, stride, dil, forward precision, extra floats per input row, coff, extra)"""
    r = _rng("default")
    must = [1, 3, 17, 33, 38, 65, 70, 100]
    out = []
    for i in range(60):
        k = [1, 3, 3, 5, 7, 3][i % 6]
        s = r.choice([1, 2])
        dil = r.choice([1, 2, 3]) if (k == 3 and s == 1) else 1
        for attempt in range(400):
            Ci = must[i % 8] if i < 16 and i % 2 == 0 else r.choice(CHANNELS)
            Co = must[(i // 2) % 8] if i < 16 and i % 2 == 1 else r.choice(CHANNELS)
            B, H, W = r.randint(1, 2), r.randint(1, 14), r.randint(1, 23)
            if i in (3, 21):
                H = 1                                         # one-row images
            if i in (4, 22):
                W = 1                                         # one-column images
            Ho, Wo, _, _ = ops.conv_geometry(H, W, k, k, s, dil)
            if k * k * Ci * Co * B * Ho * Wo <= MAC_BUDGET:
                break
        else:
            raise AssertionError("no geometry")
        out.append((B, H, W, Ci, Co, k, s, dil, i % 3, r.randint(0, 4), r.choice([0, 1, 4, 6]), r.choice([0, 2, 4])))
    return out


DEFAULT_SHAPES = _default_shapes()


def _aligned_rows(coff, N, extra):
    return coff % 4 == 0 and (coff + N + extra) % 4 == 0


def _default_family(L, mode, prec, xextra, coff, extra, bias, alpha, mask):
    """conv_route restated for launches without hooks or banks at these sizes (the row / thin / patch kernels start at 16384+ pixels): the
    one-output-channel forward kernel, the one-input-channel gradient kernel, else the tiled kernel -- in bf16 only with vector loads on both operands"""
    K, N = (L.Ci, L.Co) if mode == 0 else (L.Co, L.Ci)
    vecA = (_ld(K) + xextra) % 4 == 0
    vecB = N % 4 == 0 if mode == 0 else K % 4 == 0
    vecC = N % 4 == 0 and _aligned_rows(coff, N, extra)
    if mode == 0 and N == 1 and vecA and K % 4 == 0 and mask is None:
        return "conv_n1_fwd_kernel"
    if mode == 1 and K == 1 and L.stride == 1 and vecC and not bias and alpha == 1.0:
        return "conv_k1_dgrad_kernel"
    return ("conv_igemm_kernel", ",bf16," if (prec == 1 and vecA and vecB) else ",f32,", ",dgrad," if mode else ",fwd,", ",vec," if (vecA and vecB) else ",scalar,")


def test_conv_default_dispatch_sweep(backend):
    """60 shapes under the default dispatch: k 1 / 3 / 5 / 7, stride 1 / 2, dilation 1 .. 3, one-row and one-column images, channel counts on both sides
    of 4 / 16 / 32 / 64, input rows with 0 .. 4 extra floats, the result in a slice at offset 0 / 1 / 4 / 6 with 0 / 2 / 4 floats behind it; per shape
    the forward pass (precision 0 / 1 / 2 by turns), the input gradient in precisions 0 and 1, and mh_conv2d_wgrad"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_conv2d (default dispatch)")
    r = _rng("default/variants")
    for i, shp in enumerate(DEFAULT_SHAPES):
        B, H, W, Ci, Co, k, s, dil, prec, xextra, coff, extra = shp
        L = Layer(1000 + 10 * i, B, H, W, Ci, Co, k, s, dil)
        for mode, pr in ((0, prec), (1, 0), (1, 1)):
            N = Co if mode == 0 else Ci
            bias, alpha, mask, acc = _variant(r, N, mode)
            name, what, got = launch(backend, L, mode, pr, coff, extra, xextra, bias, alpha, mask, acc)
            check(W_, L, mode, name, "shape %d %s" % (i, what), got, bias, alpha, mask, acc, _default_family(L, mode, pr, xextra, coff, extra, bias, alpha, mask))
        # the filter gradient, atomics onto zeros
        pw = i % 2
        xld = _ld(Ci) + xextra
        x = L.dev(("in", 0, xld), dev, lambda: _wide(L.x, xld, dev))
        dz = _wide(L.dz, _ld(Co), dev)
        dw = FP.Guarded(L.w.numel(), torch.float32, dev).set(torch.zeros(L.w.numel()))
        db = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
        d = ops.conv_desc(B, H, W, L.Ho, L.Wo, Ci, Co, k, k, s, dil, L.pt, L.pl, 0, 0, xld, _ld(Co), precision=pw)
        rc = lib._raw_mh_conv2d_wgrad(C.byref(d), P(x), P(dz), _ld(Co), C.c_void_p(dw.ptr()), C.c_void_p(db.ptr()), None)
        name = lib.last_kernel().decode()
        backend.sync()
        what = "shape %d %s wgrad prec=%d [%s]" % (i, shp, pw, name)
        assert rc == 0, (what, lib.last_error())
        bf16 = pw == 1 and xld % 4 == 0 and Co % 4 == 0
        n1 = Co == 1 and k == 3 and xld % 4 == 0 and Ci % 4 == 0
        assert ("wgrad_n1_kernel" if n1 else "wgrad_bf16_kernel" if bf16 else "wgrad_kernel<") in name, what
        dw.assert_guards(what); db.assert_guards(what)
        W_.check(what, "wgrad bf16" if (bf16 and not n1) else "wgrad fp32", dw.t.view(L.w.shape), L.wgrad_ref(bf16 and not n1), 2e-4 if (bf16 and not n1) else 1e-4)
        W_.check(what, "wgrad bias", db.t, L.dz.double().sum((0, 1, 2)), 1e-4)
    W_.report(backend, len(DEFAULT_SHAPES))


# ---- 2. the tiled kernel, every tile forced ---------------------------------------------------------------------------------------------------------
K_TILES = [(128, 128, 32), (128, 96, 32), (128, 64, 32), (64, 128, 32), (64, 96, 32), (64, 64, 32), (128, 32, 32), (32, 128, 64), (32, 96, 64), (32, 64, 64),
           (64, 32, 64), (32, 32, 64), (128, 16, 32), (64, 16, 64), (32, 64, 128), (64, 32, 128), (32, 32, 128)]           # kTiles of csrc/conv.hip


def _tiled_shapes():
    """(tile, flag bits 16 .. 19 of bm, B, H, W, Cin, Cout, k, stride, dil, precision): every tile in exact fp32 and in bf16, every third one in split-bf16 too,
    Cout around the tile's column count, any k / stride / dilation"""
    r = _rng("tiled")
    out = []
    for ti, (bm, bn, kt) in enumerate(K_TILES):
        for prec in ((0, 1, 2) if ti % 3 == 2 else (0, 1)):
            k = r.choice([1, 3, 3, 3, 4, 5, 7])
            s = r.choice([1, 1, 2])
            dil = r.choice([1, 2, 3]) if s == 1 and k == 3 else 1
            flags = r.choice([0, 0, 1, 2, 4, 8, 3, 12, 15])
            for attempt in range(400):
                # channel counts: multiples of the K tile (the uniform-tap loader), ragged ones, more than 4 K tiles per tap (the ragged-K loader)
                Ci = r.choice([4, 8, 16, 20, 32, 36, 38, 64, 70, 128, 132, 192, 260, 264])
                Co = r.choice([c for c in (4, 8, 12, 16, 20, 24, 32, 36, 40, 64, 68, 96, 100, 128, 132, 17, 33) if c <= bn + 36])
                B, H, W = r.randint(1, 2), r.randint(2, 14), r.randint(2, 23)
                Ho, Wo, _, _ = ops.conv_geometry(H, W, k, k, s, dil)
                if k * k * Ci * Co * B * Ho * Wo <= MAC_BUDGET and (attempt > 300 or B * Ho * Wo > min(bm, 64)):
                    break
            else:
                raise AssertionError("no geometry")
            out.append(((bm, bn, kt), flags, B, H, W, Ci, Co, k, s, dil, prec))
    return out


TILED_SHAPES = _tiled_shapes()


def test_conv_tiled_kernel_sweep(backend):
    """conv_igemm_kernel with each of its 17 tiles forced (mh_tune_conv_tile), exact fp32 and bf16 / split-bf16 (mh_tune_conv_x3_igemm(1)), bits 16 .. 19
    of bm flipped at random (uniform-tap loader off, split-K off, stride-2 parity classes off, ragged-K loader off); forward pass and input gradient
    into 16-byte aligned slices with live neighbours, randomised bias / alpha / mask / accumulation"""
    lib = backend.lib
    W_ = _Worst("conv_igemm_kernel (forced tiles)")
    r = _rng("tiled/variants")
    for i, shp in enumerate(TILED_SHAPES):
        (bm, bn, kt), flags, B, H, W, Ci, Co, k, s, dil, prec = shp
        L = Layer(3000 + 10 * i, B, H, W, Ci, Co, k, s, dil, wscale=0.2 if Ci <= 136 else 0.1)
        for mode in (0, 1):
            K, N = (Ci, Co) if mode == 0 else (Co, Ci)
            bias, alpha, mask, acc = _variant(r, N, mode)
            coff, extra = r.choice([(4, 4), (0, 4), (8, 0), (4, 8)])
            vecB = (N if mode == 0 else K) % 4 == 0
            x3 = prec == 2 and mode == 0 and vecB
            lib.tune_conv_patch(0)
            lib.tune_conv_x3_igemm(1)
            lib.tune_conv_tile(bm | (flags << 16), bn | (kt << 16))
            try:
                name, what, got = launch(backend, L, mode, prec, coff, extra, 0, bias, alpha, mask, acc)
            finally:
                lib.tune_conv_tile(0, 0)
                lib.tune_conv_x3_igemm(-1)
                lib.tune_conv_patch(-1)
            arith = ",bf16x3," if x3 else ",bf16," if (prec == 1 and vecB) else ",f32,"
            fam = ("conv_igemm_kernel", arith, "tile %dx%d " % (bm, 64 if (x3 and (bm, bn) == (128, 128)) else bn), ",vec," if vecB else ",scalar,")
            check(W_, L, mode, name, "shape %d tile %s flags %d %s" % (i, (bm, bn, kt), flags, what), got, bias, alpha, mask, acc, fam)
    W_.report(backend, len(TILED_SHAPES))


# ---- 2. the head kernels -----------------------------------------------------------------------------------------------------------------------------
def _head_shapes():
    """(kind, B, H, W, C, k, stride, dil): 'n1' = the one-output-channel forward kernel (C input channels, C % 4 == 0), 'k1' = the input gradient of a
    one-output-channel layer (C % 4 == 0 gradient columns), 'head' = mh_conv2d_head with its two extra slots"""
    r = _rng("heads")
    out = []
    for i in range(30):
        kind = ("n1", "k1", "head")[i % 3]
        k = 3 if kind == "head" else r.choice([1, 3, 3, 5])
        s = r.choice([1, 1, 2]) if kind == "n1" else 1
        dil = r.choice([1, 2, 4]) if (k == 3 and s == 1 and kind != "head") else 1
        out.append((kind, r.randint(1, 2), r.randint(1, 14), r.randint(1, 23), r.choice([4, 8, 12, 16, 20, 32, 36, 64, 68, 100, 128]), k, s, dil))
    return out


HEAD_SHAPES = _head_shapes()


def test_conv_head_kernels_sweep(backend):
    """conv_n1_fwd_kernel (any k / stride / dilation, bias, alpha, accumulation, every precision code: exact fp32), conv_k1_dgrad_kernel (mask, sub-range
    mask, accumulation) and mh_conv2d_head: the same bits in the result and in one-channel slots of two wider buffers, nothing else written"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("head kernels")
    r = _rng("heads/variants")
    for i, (kind, B, H, W, Cc, k, s, dil) in enumerate(HEAD_SHAPES):
        L = Layer(5000 + 10 * i, B, H, W, Cc, 1, k, s, dil)
        prec = i % 3 if kind != "k1" else i % 2
        if kind == "n1":
            bias, alpha, _, acc = _variant(r, 1, 0)
            coff, extra = r.choice([(0, 0), (5, 3), (0, 2), (4, 4)])
            name, what, got = launch(backend, L, 0, prec, coff, extra, r.choice([0, 4]), bias, alpha, None, acc)
            check(W_, L, 0, name, "shape %d %s" % (i, what), got, bias, alpha, None, acc, "conv_n1_fwd_kernel")
        elif kind == "k1":
            _, _, mask, acc = _variant(r, Cc, 1)
            coff, extra = r.choice([(4, 4), (0, 0), (8, 4)])
            name, what, got = launch(backend, L, 1, prec, coff, extra, r.randint(0, 3), False, 1.0, mask, acc)
            check(W_, L, 1, name, "shape %d %s" % (i, what), got, False, 1.0, mask, acc, "conv_k1_dgrad_kernel")
        else:
            bias = bool(r.getrandbits(1))
            slots = [FP.slice_view(dev, B, H, W, 1, c, e) for c, e in ((0, 0), (r.randint(1, 7), r.randint(0, 5)), (0, r.randint(1, 4)))]
            snaps = [g.snapshot() for g, v in slots]
            x = _wide(L.x, Cc, dev)
            ops.conv2d_head(lib, ops.View(x, B, H, W, Cc, Cc), L.w.to(dev), (L.bias[0].to(dev) if bias else None), slots[0][1], copies=(slots[1][1], slots[2][1]))
            name = lib.last_kernel().decode()
            backend.sync()
            what = "shape %d head %s bias=%d [%s]" % (i, L.shape(), bias, name)
            assert "conv_n1_fwd_kernel" in name, what
            outs = []
            for (g, v), snap in zip(slots, snaps):
                coff = (v.ptr - g.t.data_ptr()) // 4
                FP.assert_only_slice_written(g, v, coff, snap, what)
                outs.append(FP.slice_of(g, v, coff))
            assert torch.equal(FP.bits(outs[0]), FP.bits(outs[1])) and torch.equal(FP.bits(outs[0]), FP.bits(outs[2])), what + ": the three copies differ"
            W_.check(what, "conv_n1_fwd_kernel fp32 head", outs[0], L.expected(0, False, bias, 1.0, None, False), 2e-5)
    W_.report(backend, len(HEAD_SHAPES))


# ---- 3. transposed convolution -------------------------------------------------------------------------------------------------------------------------
def _transpose_shapes():
    """(B, H, W, Cin, Cout, k, precision, bias, alpha, coff, extra): H x W the INPUT size, the result is twice as large"""
    r = _rng("transpose")
    out = []
    for i in range(16):
        Ci, Co = r.choice([1, 3, 4, 8, 17, 32, 33, 38, 64, 70]), r.choice([1, 2, 4, 5, 8, 16, 20, 33, 64])
        out.append((r.randint(1, 2), r.randint(1, 7), r.randint(1, 11), Ci, Co, 4 if i % 2 == 0 else 3, (i // 2) % 2, bool(r.getrandbits(1)), r.choice([1.0, 0.2, 0.1]),
                    r.choice([0, 4, 1]), r.choice([0, 4, 2])))
    return out


TRANSPOSE_SHAPES = _transpose_shapes()


def test_conv_transpose_sweep(backend):
    """ops.conv2d_transpose_fwd (sharedLayers.conv2d_transpose: the input gradient of a stride-2 'SAME' conv, with bias and leaky): 4x4 and 3x3, ragged
    channel counts, precisions 0 and 1, into slices; against the float64 conv2d_transpose of the oracle"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("conv2d_transpose_fwd")
    for i, shp in enumerate(TRANSPOSE_SHAPES):
        B, H, W, Ci, Co, k, prec, bias, alpha, coff, extra = shp
        x, w, b = _rand((B, H, W, Ci), 7000 + 3 * i), _rand((k, k, Co, Ci), 7001 + 3 * i, 0.3), _rand((Co,), 7002 + 3 * i)
        xd = _wide(x, _ld(Ci), dev)
        g, ov = FP.slice_view(dev, B, 2 * H, 2 * W, Co, coff, extra)
        before = g.snapshot()
        ops.conv2d_transpose_fwd(lib, ops.View(xd, B, H, W, Ci, _ld(Ci)), w.to(dev), (b.to(dev) if bias else None), ov, stride=2, alpha=alpha, precision=prec)
        name = lib.last_kernel().decode()
        backend.sync()
        what = "shape %d %s [%s]" % (i, shp, name)
        FP.assert_only_slice_written(g, ov, coff, before, what)
        vec = Ci % 4 == 0                                       # (mode 1: the descriptor's K is the transposed layer's input channel count)
        fam = ("conv_igemm_kernel", ",dgrad,", ",bf16," if (prec == 1 and vec) else ",f32,")
        for sub in fam:
            assert sub in name, what
        rounded, tol, key = _tolerance(name)
        rd = _bf if rounded else (lambda t: t)
        ref = T.conv2d_transpose(rd(x).double(), rd(w).double(), (b.double() if bias else torch.zeros(Co, dtype=torch.float64)), stride=2, alpha=alpha)
        W_.check(what, key, FP.slice_of(g, ov, coff), ref, tol)
    W_.report(backend, len(TRANSPOSE_SHAPES))


# ---- 2. the row-streaming, thin-layer, small-layer bank and patch-staged kernels, each forced with its hook or bank ----------------------------------
def _epilogue(r, N, mode, plain=False):
    """(bias, alpha, mask, accumulate, (coff, extra)): randomised; plain = no mask and no accumulation (the split-bf16 row kernel)"""
    bias, alpha, mask, acc = _variant(r, N, mode)
    if plain:
        mask, acc = None, False
    return bias, alpha, mask, acc, r.choice([(4, 4), (0, 4), (8, 0), (4, 8)])


def _rows_shapes():
    """(B, H, W, Cin, Cout, stride, mode, precision): mh_conv_rows_ok -- 3x3, dilation 1; stride 1: K % 4 == 0, 2 <= K <= 16, N <= 32, N % 8 == 0 (K, N of the
    descriptor: swapped in mode 1); stride-2 forward also K = 2 / 3; bf16 in both modes, split-bf16 forward only"""
    r = _rng("rows")
    out = []
    for i in range(30):
        what = ("fwd-bf16", "dgrad-bf16", "fwd-x3", "fwd-s2-bf16", "fwd-s2-x3", "fwd-bf16")[i % 6]
        mode = 1 if what.startswith("dgrad") else 0
        s = 2 if "s2" in what else 1
        small, big = r.choice([2, 3, 4, 8, 12, 16] if s == 2 else [4, 8, 12, 16]), r.choice([8, 16, 24, 32])
        Ci, Co = (small, big) if mode == 0 else (big, small)
        H, W = r.randint(1, 14), r.choice([1, 7, 23, 31, 32, 33, 40, 45])                  # (32-column strips: ragged, exact, two)
        out.append((r.randint(1, 2), H, W, Ci, Co, s, mode, 2 if "x3" in what else 1))
    return out


ROWS_SHAPES = _rows_shapes()


def test_conv_rows_kernel_sweep(backend):
    """conv_rows_kernel forced with mh_tune_conv_rows(1)"""
    lib = backend.lib
    W_ = _Worst("conv_rows_kernel")
    r = _rng("rows/variants")
    for i, (B, H, W, Ci, Co, s, mode, prec) in enumerate(ROWS_SHAPES):
        L = Layer(9000 + 10 * i, B, H, W, Ci, Co, 3, s, 1)
        bias, alpha, mask, acc, (coff, extra) = _epilogue(r, Co if mode == 0 else Ci, mode, plain=(prec == 2))
        lib.tune_conv_rows(1)
        try:
            name, what, got = launch(backend, L, mode, prec, coff, extra, r.choice([0, 4]), bias, alpha, mask, acc)
        finally:
            lib.tune_conv_rows(-1)
        fam = ("conv_rows_kernel<%s,%s,s%d" % ("dgrad" if mode else "fwd", "bf16x3" if prec == 2 else "bf16", s),)
        check(W_, L, mode, name, "shape %d %s" % (i, what), got, bias, alpha, mask, acc, fam)
    W_.report(backend, len(ROWS_SHAPES))


def _thin_shapes():
    """(B, H, W, Cin, Cout, stride, mode): conv_thin_ok -- bf16, 3x3, dilation 1, K in {1, 2, 3, 4, 8, 16, 32} (one 4-channel group, or 2 / 4 / 8 whole
    ones), N in {16, 32}; forward stride <= 2, gradient stride 1.  30 shapes the kernel takes (16 forward: every K at both N, stride 2 with 2, 4 and 8
    groups; 14 gradients), then three ragged counts in several groups (5, 13, 30) that must be refused"""
    r = _rng("thin")
    out = []
    fwd = [(kk, nn) for nn in (16, 32) for kk in (1, 2, 3, 4, 8, 16, 32)] + [(16, 32), (8, 16)]
    for j, (kk, nn) in enumerate(fwd):
        s = 2 if (kk >= 8 and j % 2 == 0) or j >= 14 else r.choice([1, 2])
        out.append((r.randint(1, 2), r.randint(1, 14), r.randint(1, 23), kk, nn, s, 0))
    for j in range(14):
        kk, nn = (4, 8, 16, 32)[j % 4], (16, 32)[(j // 4) % 2]           # (a gradient reads the weights transposed: K = Cout, K % 4 == 0)
        out.append((r.randint(1, 2), r.randint(1, 14), r.randint(1, 23), nn, kk, 1, 1))
    for kk, nn, s in ((5, 16, 1), (13, 32, 2), (30, 16, 1)):
        out.append((r.randint(1, 2), r.randint(1, 14), r.randint(1, 23), kk, nn, s, 0))
    return out


THIN_SHAPES = _thin_shapes()


def test_conv_thin_kernel_sweep(backend):
    """conv_thin_kernel forced with mh_tune_conv_thin(1) (bf16 only)"""
    lib = backend.lib
    W_ = _Worst("conv_thin_kernel")
    r = _rng("thin/variants")
    for i, (B, H, W, Ci, Co, s, mode) in enumerate(THIN_SHAPES):
        L = Layer(11000 + 10 * i, B, H, W, Ci, Co, 3, s, 1)
        bias, alpha, mask, acc, (coff, extra) = _epilogue(r, Co if mode == 0 else Ci, mode)
        K = Ci if mode == 0 else Co
        xextra = r.choice([0, 4]) if K > 1 else 3            # (one input channel: rows of 4 floats, so that the kernel's 16-byte loads are legal)
        lib.tune_conv_thin(1)
        try:
            name, what, got = launch(backend, L, mode, 1, coff, extra, xextra, bias, alpha, mask, acc)
        finally:
            lib.tune_conv_thin(0)
        if K > 4 and K % 4:
            # a ragged channel count in more than one 4-channel group has no thin instance (the kernel pads one group only; it used to be taken
            # under the hook, dropped every fourth channel and multiplied the row padding into the result): the tiled kernel, in bf16
            fam = ("conv_igemm_kernel", ",bf16,")
        else:
            fam = ("conv_thin_kernel<NT=%d,%s>" % (1 if (Co if mode == 0 else Ci) <= 16 else 2, "dgrad" if mode else "fwd"),)
        check(W_, L, mode, name, "shape %d %s" % (i, what), got, bias, alpha, mask, acc, fam)
    W_.report(backend, len(THIN_SHAPES))


def _cover_ok(Ho, Wo, d, th, limit):
    """the lattice cover rule of the bank / patch kernels: tiles of th rows x 16 columns per dilation class may cover at most limit x the image"""
    cover = d * d * (-(-(-(-Ho // d)) // th)) * th * (-(-(-(-Wo // d)) // 16)) * 16
    return cover <= limit * Ho * Wo


def _bank_shapes():
    """(B, H, W, Cin, Cout, stride, dil, mode, precision): mh_conv_bank_small_ok -- 3x3 with a fragment bank, K, N >= 16, K <= 224 (192 at stride 2: the patch staging), dilation up to 8 where the
    lattice cover stays under 2.5x, stride-2 forward; bf16 in both modes, split-bf16 forward"""
    r = _rng("bank_small")
    out = []
    for i in range(30):
        what = ("fwd-bf16", "dgrad-bf16", "fwd-x3", "fwd-s2-bf16", "fwd-s2-x3", "dgrad-bf16")[i % 6]
        mode = 1 if what.startswith("dgrad") else 0
        s = 2 if "s2" in what else 1
        for attempt in range(1000):
            Ci, Co = r.choice([16, 17, 20, 32, 33, 38, 64, 70, 96, 128, 134, 200, 224]), r.choice([16, 17, 20, 32, 33, 36, 48, 64, 65, 96, 128, 160])
            dil = r.choice([1, 1, 2, 3, 4, 8]) if s == 1 else 1
            B, H, W = r.randint(1, 2), r.randint(1, 20), r.randint(1, 40)
            Ho, Wo, _, _ = ops.conv_geometry(H, W, 3, 3, s, dil)
            K = Ci if mode == 0 else Co
            if K <= (224 if s == 1 else 192) and Ci * Co <= 128 * 160 and 9 * Ci * Co * B * Ho * Wo <= MAC_BUDGET and _cover_ok(Ho, Wo, dil, 2, 2.5):
                break
        else:
            raise AssertionError("no geometry")
        out.append((B, H, W, Ci, Co, s, dil, mode, 2 if "x3" in what else 1))
    return out


BANK_SHAPES = _bank_shapes()


def test_conv_small_layer_bank_kernel_sweep(backend):
    """conv_bank_small_kernel, reached by handing the launch the layer's fragment bank (mh_pack_weights)"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("conv_bank_small_kernel")
    r = _rng("bank_small/variants")
    for i, (B, H, W, Ci, Co, s, dil, mode, prec) in enumerate(BANK_SHAPES):
        L = Layer(13000 + 10 * i, B, H, W, Ci, Co, 3, s, dil, wscale=0.2 if Ci <= 136 else 0.1)
        bias, alpha, mask, acc, (coff, extra) = _epilogue(r, Co if mode == 0 else Ci, mode)
        keep = []
        wd = L.dev("w", dev, lambda: L.w.to(dev))
        planes = 2 if prec == 2 else 1
        bank = torch.zeros(ops.pack_bytes(wd, planes, mode) // 4, device=dev)
        ops.pack_weights(lib, [(wd, bank, planes, mode)], dev, keep)
        name, what, got = launch(backend, L, mode, prec, coff, extra, r.choice([0, 4]), bias, alpha, mask, acc, bank=bank)
        fam = ("conv_bank_small_kernel<%s,%s>" % ("dgrad" if mode else "fwd", "bf16x3" if prec == 2 else "bf16"),)
        check(W_, L, mode, name, "shape %d %s" % (i, what), got, bias, alpha, mask, acc, fam)
    W_.report(backend, len(BANK_SHAPES))


def _patch_shapes():
    """(B, H, W, Cin, Cout, dil, mode, precision, hook): mh_conv_patch_ok -- 3x3 stride 1, K, N >= 32, dilation up to 8; split-bf16 forward from 48 output columns;
    Cin in {36, 38, 70} in rows padded to a multiple of 4: forward operand rows, and the padded-row form of the input gradient (ConvArgs::vecCpad)"""
    r = _rng("patch")
    out = []
    grad_cin = [38, 70, 70, 38, 36, 64, 38, 70, 128, 96]          # the ten input gradients: six in padded rows (38 -> 40, 70 -> 72)
    for i in range(30):
        mode, prec = ((0, 1), (1, 1), (0, 2))[i % 3]
        for attempt in range(1000):
            Ci = grad_cin[i // 3] if mode == 1 else r.choice([36, 38, 70]) if i % 2 == 0 else r.choice([32, 40, 64, 96, 128])
            Co = r.choice([48, 64, 96, 128, 160] if prec == 2 else [32, 36, 48, 64, 96, 100, 128])
            dil = r.choice([1, 1, 2, 3, 4, 8])
            B, H, W = r.randint(1, 2), r.randint(1, 14), r.randint(1, 23)
            if Ci * Co <= 128 * 160 and 9 * Ci * Co * B * H * W <= MAC_BUDGET:
                break
        else:
            raise AssertionError("no geometry")
        out.append((B, H, W, Ci, Co, dil, mode, prec, r.choice([64, 128]) + r.choice([0, 256]) + r.choice([0, 2048])))
    return out


PATCH_SHAPES = _patch_shapes()


def test_conv_patch_kernel_sweep(backend):
    """conv_patch_kernel forced with mh_tune_conv_patch(64 | 128 [+ 256] [+ 2048]); an input gradient with Cin % 4 != 0 goes into rows of Cin rounded up to 4
    (ConvArgs::vecCpad): the padding columns hold zeros afterwards (six such launches, by turns plain and accumulating onto zeroed padding) and nothing
    behind them is written"""
    lib = backend.lib
    W_ = _Worst("conv_patch_kernel")
    r = _rng("patch/variants")
    padded = []
    for i, (B, H, W, Ci, Co, dil, mode, prec, hook) in enumerate(PATCH_SHAPES):
        L = Layer(15000 + 10 * i, B, H, W, Ci, Co, 3, 1, dil)
        N = Co if mode == 0 else Ci
        bias, alpha, mask, acc, (coff, extra) = _epilogue(r, N, mode)
        pad = FP.round_up(N, 4) - N if mode == 1 else 0
        if pad:
            coff, extra = r.choice([(0, pad + 4), (4, pad + 8), (8, pad)])
            acc = len(padded) % 2 == 1
            padded.append((Ci, acc))
        lib.tune_conv_patch(hook)
        try:
            name, what, got = launch(backend, L, mode, prec, coff, extra, r.choice([0, 4]), bias, alpha, mask, acc, pad=pad)
        finally:
            lib.tune_conv_patch(-1)
        fam = ("conv_patch_kernel", ",dgrad," if mode else ",fwd,") + (("bf16x3",) if prec == 2 else ())
        check(W_, L, mode, name, "shape %d hook %d %s" % (i, hook, what), got, bias, alpha, mask, acc, fam)
    assert sorted(padded) == [(38, False), (38, False), (38, True), (70, False), (70, True), (70, True)], padded
    W_.report(backend, len(PATCH_SHAPES))


# ---- 6. the plane kernels ------------------------------------------------------------------------------------------------------------------------------
PLANES_BUDGET = 40e6                   # taps * Cin * Cout * output pixels of one shape (emulator time)


def _split(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _planes_geometry(r, taps, K, N, stride=1, even=False):
    for attempt in range(1000):
        dil = r.choice([1, 1, 2, 3, 4, 8, 16]) if stride == 1 else 1
        B, H, W = r.randint(1, 2), r.randint(1, 14), r.randint(1, 45)
        if even:
            H, W = 2 * ((H + 1) // 2), 2 * ((W + 1) // 2)
        if taps * K * N * B * (H // stride) * (W // stride) <= PLANES_BUDGET:
            return B, H, W, dil
    raise AssertionError("no geometry")


def _planes_fwd_shapes():
    """(B, H, W, K, N, k, stride, dil, bf16, tile variant of mh_tune_conv_planes): what mh_conv2d_planes_ok documents -- MADNet's split-bf16 layers (N % 8 == 0,
    ceil(K / 16) in {2, 3, 4, 5, 6, 8}), the K-chunked one-plane bf16 form (K > 128), the stride-2 forward instances (3x3: K <= 16 -> 32, 17 .. 32 -> 64,
    49 .. 64 -> 96; 5x5: 49 .. 64 -> 128 in both arithmetics)"""
    r = _rng("planes_fwd")
    out = []
    for i in range(24):
        var = r.choice([0, 1, 2, 3, 4])
        if i < 14:
            k16 = (2, 3, 4, 5, 6, 8)[i % 6]
            K, N = r.randint(16 * k16 - 15, 16 * k16), 8 * r.randint(1, 16)
            B, H, W, dil = _planes_geometry(r, 9, K, N)
            out.append((B, H, W, K, N, 3, 1, dil, False, var))
        elif i < 18:
            K, N = r.choice([129, 136, 160, 210]), 8 * r.randint(1, 12)          # (not 193 .. 208: 13 K-steps keep a whole-K layout, split-bf16 only)
            B, H, W, dil = _planes_geometry(r, 9, K, N)
            out.append((B, H, W, K, N, 3, 1, dil, True, var))
        else:
            k, K, N, bf16 = ((3, r.randint(1, 16), 32, False), (3, r.randint(17, 32), 64, False), (3, r.randint(49, 64), 96, False), (5, r.randint(49, 64), 128, False),
                             (5, r.randint(49, 64), 128, True), (3, r.randint(17, 32), 64, False))[i - 18]
            B, H, W, dil = _planes_geometry(r, k * k, K, N, stride=2, even=True)
            out.append((B, H, W, K, N, k, 2, 1, bf16, var))
    # the staggered form (+ 16) of the 128-pixel tile (variants 1 / 3): its instances are (ceil(K / 16), 32-column waves) = (3, 4), (8, 4), (8, 3), (6, 2),
    # taken when the grid has at most 256 workgroups
    for K, N, v in ((38, 128, 1), (128, 104, 3), (120, 96, 1), (90, 64, 3), (113, 72, 1), (33, 120, 3)):
        out.append((r.randint(1, 2), r.randint(3, 12), r.randint(9, 40), K, N, 3, 1, r.choice([1, 1, 2]), False, v + 16))
    return out


PLANES_FWD_SHAPES = _planes_fwd_shapes()


def _guarded_shadow(dev, npix, N):
    return FP.Guarded(npix * ops.shadow_ld(N), torch.bfloat16, dev)


def test_conv_planes_forward_sweep(backend):
    """mh_conv2d_planes: the fp32 result in a 16-byte aligned slice with live neighbours, both result planes in rows of round_up(N, 32) whose padding channels
    hold a sentinel; planes == the split of the fp32 result bit for bit, padding untouched; random dilation up to 16, tile variants 0 .. 4; six pinned
    shapes reach the staggered form (+ 16), asserted by name; values: split-bf16 against the unrounded float64 oracle (4e-5), one-plane bf16 against bf16-rounded operands (3e-5)"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_conv2d_planes")
    r = _rng("planes_fwd/variants")
    for i, shp in enumerate(PLANES_FWD_SHAPES):
        B, H, W, K, N, k, s, dil, bf16, var = shp
        Ho, Wo = H // s, W // s
        x, w, b = _rand((B, H, W, K), 17000 + 3 * i), _rand((k, k, K, N), 17001 + 3 * i, 0.2 if K <= 128 else 0.05), _rand((N,), 17002 + 3 * i)
        bias, alpha = bool(r.getrandbits(1)), r.choice([0.2, 1.0])
        coff, extra = r.choice([(4, 4), (0, 4), (0, 0), (8, 4)])
        rd = _bf if bf16 else (lambda t: t)
        ref = T.conv2d(rd(x).double(), rd(w).double(), (b.double() if bias else None), stride=s, dilation=dil, alpha=alpha)
        assert tuple(ref.shape) == (B, Ho, Wo, N)
        xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
        keep = []
        xp = ops.Planes(ops.Shadow(B, H, W, K, dev), dev)
        ops.plane_split(lib, [(ops.view(xd), xp)], dev, keep)
        planes = 1 if bf16 else 2
        bank = torch.zeros(ops.pack_bytes(wd, planes, 2) // 4, device=dev)
        ops.pack_weights(lib, [(wd, bank, planes, 2)], dev, keep)
        npix, pld = B * Ho * Wo, ops.shadow_ld(N)
        g, ov = FP.slice_view(dev, B, Ho, Wo, N, coff, extra)
        ghi, glo = _guarded_shadow(dev, npix, N), _guarded_shadow(dev, npix, N)
        before = g.snapshot()
        pad = dil if s == 1 else (k - 2) // 2
        d = ops.conv_desc(B, H, W, Ho, Wo, K, N, k, k, s, dil, pad, pad, 0, 0, 0, ov.ld, alpha=alpha, precision=1 if bf16 else 2)
        assert lib.conv2d_planes_ok(C.byref(d)) == 1, shp
        lib.tune_conv_planes(var)
        try:
            rc = lib._raw_mh_conv2d_planes(C.byref(d), C.c_void_p(xp.hi.ptr), (None if bf16 else C.c_void_p(xp.lo.ptr)), xp.ld, P(bank), (P(bd) if bias else None),
                                           C.c_void_p(ov.ptr), C.c_void_p(ghi.ptr()), (None if bf16 else C.c_void_p(glo.ptr())), pld, None)
            name = lib.last_kernel().decode() if rc == 0 else "-"
        finally:
            lib.tune_conv_planes(0)
        backend.sync()
        what = "shape %d %s bias=%d alpha=%g coff=%d extra=%d [%s]" % (i, shp, bias, alpha, coff, extra, name)
        assert rc == 0, (what, lib.last_error())
        fam = "conv_planes_s2fwd_kernel" if s == 2 else "conv_planes_ck_kernel" if K > 128 else "conv_planes_kernel"
        assert fam in name and (",bf16>" in name or ",bf16," in name if bf16 else "bf16x3" in name), what
        assert ("staggered" in name) == bool(var & 16), what
        FP.assert_only_slice_written(g, ov, coff, before, what)
        out = FP.slice_of(g, ov, coff)
        W_.check(what, fam + (" bf16" if bf16 else " bf16x3"), out, ref, 3e-5 if bf16 else 4e-5)
        hi, lo = _split(out)
        for gs, want, used in ((ghi, hi, True), (glo, lo, not bf16)):
            gs.assert_guards(what)
            sb = gs.payload_bits().view(npix, pld)
            if used:
                assert torch.equal(sb[:, :N], FP.bits(want).view(npix, N)), what + ": plane != split of the stored fp32 result"
                assert (sb[:, N:] == FP.NAN16).all(), what + ": padding channels of a result plane were written"
            else:
                assert (sb == FP.NAN16).all(), what
    W_.report(backend, len(PLANES_FWD_SHAPES))


def _planes_bwd_shapes():
    """(B, Hz, Wz, Cin, Cout, k, stride, dil, mask range or None, accumulate, tile variant): what mh_conv2d_planes_bwd_ok documents -- stride 1: (ceil(Cout / 16),
    ceil(Cin / 32)) in {(8, 4), (6, 4), (4, 4), (4, 3), (4, 2), (2, 4), (2, 2), (2, 1)} and the K-chunked reduction (Cout > 128); stride 2 (with accumulation):
    3x3 with Cout in {32, 64}, Cin <= 32; 5x5 with Cout = 128, Cin 33 .. 64.  Hz x Wz = the size of dz"""
    r = _rng("planes_bwd")
    out = []
    pairs = [(8, 4), (6, 4), (4, 4), (4, 3), (4, 2), (2, 4), (2, 2), (2, 1)]
    for i in range(24):
        var = r.choice([0, 1, 2, 3, 4])
        if i < 12:
            k16, n32 = pairs[i % 8]
            Co, Ci = r.randint(16 * k16 - 15, 16 * k16), r.randint(32 * n32 - 31, 32 * n32)
            k, s = 3, 1
        elif i < 16:
            Co, Ci, k, s = r.choice([129, 136, 160]), r.randint(1, 128), 3, 1
        else:
            k, s = (3, 2) if i < 22 else (5, 2)
            Co, Ci = (r.choice([32, 64]), r.randint(1, 32)) if k == 3 else (128, r.randint(33, 64))
        B, H, W, dil = _planes_geometry(r, k * k, Ci, Co, stride=1)
        if s == 2:
            H, W, dil = (H + 1) // 2, (W + 1) // 2, 1
        mr = None
        if r.getrandbits(1) and Ci > 1:
            c0 = r.randint(0, Ci - 1)
            mr = (c0, r.randint(c0 + 1, Ci))
        out.append((B, H, W, Ci, Co, k, s, dil, mr, bool(s == 2 and r.getrandbits(1)), var))
    # the staggered form (+ 32) of the 128-pixel tile (variants 1 / 3): 97 .. 128 gradient columns, a reduction over ceil(Cout / 16) in {6, 8}, at most
    # 256 workgroups
    for Ci, Co, v, mr in ((128, 128, 1, None), (97, 96, 3, (8, 90)), (110, 113, 3, None), (128, 81, 1, (0, 64))):
        out.append((r.randint(1, 2), r.randint(3, 12), r.randint(9, 40), Ci, Co, 3, 1, r.choice([1, 1, 2]), mr, False, v + 32))
    return out


PLANES_BWD_SHAPES = _planes_bwd_shapes()


def test_conv_planes_input_gradient_sweep(backend):
    """mh_conv2d_planes_bwd: dx in a slice of rows that hold Cin rounded up to 8 (the padding columns receive zeros, nothing else is written), its bf16 shadow
    == bf16(dx) with zero padding, the leaky mask from the input's shadow over every channel or a sub-range, the stride-2 forms with accumulation
    ((old + gradient) * mask); against the float64 oracle on bf16-rounded operands (2e-5)"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_conv2d_planes_bwd")
    r = _rng("planes_bwd/variants")
    for i, shp in enumerate(PLANES_BWD_SHAPES):
        B, Hz, Wz, Ci, Co, k, s, dil, mrange, acc, var = shp
        H, W = Hz * s, Wz * s
        dz, w, x, old = _rand((B, Hz, Wz, Co), 19000 + 4 * i), _rand((k, k, Ci, Co), 19001 + 4 * i, 0.2 if Co <= 128 else 0.05), _rand((B, H, W, Ci), 19002 + 4 * i), _rand((B, H, W, Ci), 19003 + 4 * i)
        xin = torch.zeros(B, H, W, Ci, dtype=torch.float64, requires_grad=True)
        (ref,) = torch.autograd.grad(T.conv2d(xin, _bf(w).double(), None, stride=s, dilation=dil, alpha=1.0), xin, _bf(dz).double())
        mk = torch.where(x.double() > 0, 1.0, 0.2)
        if mrange is not None:
            mk[..., :mrange[0]] = 1.0
            mk[..., mrange[1]:] = 1.0
        ref = (ref + (old.double() if acc else 0)) * mk
        keep = []
        dzd, wd, xd = dz.to(dev), w.to(dev), x.to(dev)
        dzs, xs, dxs = ops.Shadow(B, Hz, Wz, Co, dev), ops.Shadow(B, H, W, Ci, dev), ops.Shadow(B, H, W, Ci, dev)
        ops.shadow_cast(lib, [(ops.view(dzd), dzs), (ops.view(xd), xs)], dev, keep)
        bank = torch.zeros(ops.pack_bytes(wd, 1, 3) // 4, device=dev)
        ops.pack_weights(lib, [(wd, bank, 1, 3)], dev, keep)
        pad = FP.round_up(Ci, 8) - Ci
        coff, extra = r.choice([0, 4, 8]), pad + r.choice([0, 4])
        g, dx = FP.slice_view(dev, B, H, W, Ci, coff, extra, prefill=(old if acc else None))
        if acc and pad:
            g.t.view(B, H, W, dx.ld)[..., coff + Ci:coff + Ci + pad] = 0.0        # (what the earlier contribution left there: the sum keeps the zeros)
        assert ops.conv2d_planes_bwd_ok(lib, dx, wd, dil, stride=s), shp
        before = g.snapshot()
        lib.tune_conv_planes(var)
        try:
            ops.conv2d_planes_bwd(lib, dzs, wd, bank, dx=dx, dx_shadow=dxs, mask_shadow=xs, mask_alpha=0.2, dil=dil, mask_range=(mrange or (0, 0)), stride=s, accumulate=acc)
            name = lib.last_kernel().decode()
        finally:
            lib.tune_conv_planes(0)
        backend.sync()
        what = "shape %d %s coff=%d extra=%d [%s]" % (i, shp, coff, extra, name)
        fam = "conv_planes_s2bwd_kernel" if s == 2 else "conv_planes_ck_kernel" if Co > 128 else "conv_planes_kernel"
        assert fam in name and "bf16x3" not in name, what
        assert ("staggered" in name) == bool(var & 32), what
        FP.assert_only_slice_written(g, dx, coff, before, what, zero_cols=pad)
        out = FP.slice_of(g, dx, coff)
        W_.check(what, fam + " bf16", out, ref, 2e-5)
        sh = dxs.t.cpu()
        assert torch.equal(FP.bits(sh[..., :Ci]), FP.bits(out.to(torch.bfloat16))) and not sh[..., Ci:].float().abs().sum(), what + ": the shadow of dx"
    W_.report(backend, len(PLANES_BWD_SHAPES))
