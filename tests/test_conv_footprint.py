"""What the conv entry points STORE, and where: every kernel family of mh_conv2d* with its result going into a channel slice of a wider
buffer with live neighbours (how the engines build tf.concat), guard zones around the allocation, everything compared on bits; the values
against the float64 oracle on operands rounded the way the dispatched kernel rounds them.  Store contracts of include/madnet_hip.h that are
asserted here: zeros in the row padding behind an input gradient whose channel count is no multiple of 4, untouched shadow padding,
MH_CONV_SHADOW_ONLY, mh_conv2d_head's extra slots, mh_conv2d_planes / _planes_bwd rows, mh_conv_image_fwd's out_ld."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import footprint as FP
from madnet_hip import ops
from oracle import tf_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _families():
    spec = importlib.util.spec_from_file_location("conv_dispatch_table", os.path.join(ROOT, "scripts", "conv_dispatch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FAMILIES)


# scripts/conv_dispatch_table.py's families + one odd-channel layer that only the scalar epilogue of the generic kernel serves
FAMILIES = _families() + [("scalar", 1, 9, 13, 38, 20, None, 0, 0, False)]
# (coff, extra): a 16-byte aligned slice with live neighbours on both sides, a misaligned slice, a slice at the start of an odd-sized row
PLACEMENTS = [(4, 4), (3, 5), (0, 3)]


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def P(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def _ld(c):
    return FP.round_up(c, 4) if c > 1 else 1


def _wide(x, dev, fill=0.0):
    """[B,H,W,C] -> the same values in rows of _ld(C) floats"""
    B, H, W, Cc = x.shape
    buf = torch.full((B, H, W, _ld(Cc)), fill)
    buf[..., :Cc] = x
    return buf.to(dev)


class _Layer(object):
    """operands + cached float64 oracles of one (family, mode)"""

    def __init__(self, fam, mode):
        tag, B, H, W, Ci, Co = fam[:6]
        self.tag, self.mode = tag, mode
        self.stride = 2 if tag.endswith("_s2") else 1
        Hs, Ws, self.pt, self.pl = ops.conv_geometry(H, W, 3, 3, self.stride, 1)
        self.B, self.Ci, self.Co = B, Ci, Co
        self.Hi, self.Wi, self.Ho, self.Wo, self.K, self.N = (H, W, Hs, Ws, Ci, Co) if mode == 0 else (Hs, Ws, H, W, Co, Ci)
        self.w = _rand((3, 3, Ci, Co), 1, 0.2)
        self.x = _rand((B, self.Hi, self.Wi, self.K), 2)
        self.mask = _rand((B, self.Ho, self.Wo, self.N), 3)
        self.bias = _rand((self.N,), 4)
        self.old = _rand((B, self.Ho, self.Wo, self.N), 5)
        self._ref = {}

    def ref(self, rounded, with_bias):
        """float64: mode 0 the PRE-activation conv2d(x, w) [+ bias]; mode 1 conv2d_backprop_input(x = dz, w)"""
        key = (rounded, with_bias)
        if key not in self._ref:
            x = (_bf(self.x) if rounded else self.x).double()
            w = (_bf(self.w) if rounded else self.w).double()
            if self.mode == 0:
                r = T.conv2d(x, w, self.bias.double() if with_bias else None, stride=self.stride, dilation=1, alpha=1.0)
            else:
                xin = torch.zeros(self.B, self.Ho, self.Wo, self.N, dtype=torch.float64, requires_grad=True)
                y = T.conv2d(xin, w, None, stride=self.stride, dilation=1, alpha=1.0)
                (r,) = torch.autograd.grad(y, xin, x)
            self._ref[key] = r.detach()
        return self._ref[key]

    def expected(self, rounded, var, c0, c1):
        r = self.ref(rounded, var == "bias")
        if self.mode == 0:
            r = T.leaky(r, 0.2)
        if var == "mask+acc":
            r = r + self.old.double()
        if var in ("mask", "mask+acc", "submask"):
            m = torch.where(self.mask.double() > 0, 1.0, 0.2)
            if (c0, c1) != (0, 0):
                m[..., :c0] = 1.0
                m[..., c1:] = 1.0
            r = r * m
        return r


_layers = {}


def _layer(fam, mode):
    key = (fam[0], mode)
    if key not in _layers:
        _layers[key] = _Layer(fam, mode)
    return _layers[key]


def _tolerance(name, prec):
    """(operands rounded to bf16 in the oracle?, relative bound) by the arithmetic of the kernel that ran (mh_last_kernel names it; the thin-layer
    kernel exists in bf16 only): the bounds of tests/test_conv_parity.py"""
    if "bf16x3" in name:
        return False, 4e-5
    if "bf16" in name or "conv_thin_kernel" in name:
        return True, 1e-4
    return False, 2e-5


def _family_expected(tag, mode, prec):
    """substring of mh_last_kernel() for the plain launch into a 16-byte aligned slice: the family the case was built to reach (the tuning hooks and the
    fragment banks act on the bf16 / split-bf16 kernels; precision 0, and 2 where the family has no split-bf16 instance, run the exact-fp32 tiled kernel)"""
    if tag == "head":
        return "conv_n1_fwd_kernel" if mode == 0 else "conv_k1_dgrad_kernel"
    if tag in ("tiled", "tiled_s2", "scalar"):
        return "conv_igemm_kernel"
    reached = prec == 1 or (prec == 2 and mode == 0)
    if tag == "thin" and mode == 1:
        reached = False                      # (4 gradient columns: no thin instance)
    if tag in ("thin", "thin16") and prec == 2:
        reached = False                      # (bf16 only)
    if not reached:
        return "conv_igemm_kernel"
    return {"rows": "conv_rows_kernel", "thin": "conv_thin_kernel", "thin16": "conv_thin_kernel", "bank_small": "conv_bank_small_kernel",
            "patch": "conv_patch_kernel", "patch38": "conv_patch_kernel"}[tag]


VARIANTS = ("plain", "bias", "mask", "mask+acc", "submask")


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_conv_family_stores_only_its_slice(backend, fam, mode, prec):
    """mh_conv2d_wb into channels [coff, coff + N) of rows of coff + N + extra floats: guards and neighbours bit-untouched, every element of the
    slice written, values = the float64 oracle.  Placements: a 16-byte aligned slice between live neighbours, a misaligned one (the vector
    epilogue must step aside), a slice at the row start of an odd-sized row; for an input gradient whose N is no multiple of 4, rows padded to
    a multiple of 4 (ConvArgs::vecCpad): the padding columns hold zeros or stay as they were, the patch-staged kernel stores zeros."""
    lib, dev = backend.lib, backend.device
    tag, hook, hook_on, hook_off, banked = fam[0], fam[6], fam[7], fam[8], fam[9]
    L = _layer(fam, mode)
    N, K = L.N, L.K
    w = L.w.to(dev)
    x = _wide(L.x, dev, fill=float("nan")) if _ld(K) != K else L.x.to(dev)         # channel padding of the input rows must not leak
    mask = _wide(L.mask, dev)
    bias = L.bias.to(dev)
    keep = []
    bank = None
    if banked and ((prec == 2 and mode == 0) or prec == 1):
        planes = 2 if prec == 2 else 1
        bank = torch.zeros(ops.pack_bytes(w, planes, mode) // 4, device=dev)
        ops.pack_weights(lib, [(w, bank, planes, mode)], dev, keep)
    places = [(c, e, 0) for c, e in PLACEMENTS]
    if mode == 1 and N % 4:
        pad = FP.round_up(N, 4) - N
        places += [(0, pad + 4, pad), (4, pad + 8, pad)]
    check_place = places[3][:2] if len(places) > 3 else (4, 4)       # (a padded-row gradient is vector-legal only with its rows rounded up to 4)
    worst, names = 0.0, set()
    for var in VARIANTS:
        if var == "bias" and mode == 1:
            continue
        masked = var in ("mask", "mask+acc", "submask")
        c0, c1 = (N // 4, N // 2) if (var == "submask" and N >= 4) else (0, 0)
        for coff, extra, pad in places:
            g, ov = FP.slice_view(dev, L.B, L.Ho, L.Wo, N, coff, extra, prefill=(L.old if var == "mask+acc" else None))
            d = ops.conv_desc(L.B, L.Hi, L.Wi, L.Ho, L.Wo, K, N, 3, 3, L.stride, 1, L.pt, L.pl, mode, mode, _ld(K), ov.ld, mask_ld=(_ld(N) if masked else 0),
                              accumulate=int(var == "mask+acc"), alpha=(0.2 if mode == 0 else 1.0), mask_alpha=0.2, mask_c0=c0, mask_c1=c1, precision=prec)
            before = g.snapshot()
            if hook:
                getattr(lib, hook)(hook_on)
            try:
                rc = lib._raw_mh_conv2d_wb(C.byref(d), P(x), P(w), P(bank), P(bias) if var == "bias" else None, C.c_void_p(ov.ptr), P(mask) if masked else None, None)
                name = lib.last_kernel().decode()
            finally:
                if hook:
                    getattr(lib, hook)(hook_off)
            backend.sync()
            what = "%s mode=%d prec=%d %s coff=%d extra=%d [%s]" % (tag, mode, prec, var, coff, extra, name)
            assert rc == 0, (what, lib.last_error())
            names.add(name.split("<")[0].split(" ")[0])
            if pad:
                # ConvArgs::vecCpad: the row padding N .. round_up(N, 4) - 1 receives zeros from the patch-staged kernel's 16-byte epilogue (accumulating:
                # what it held, so nothing is asserted about its value then); any other kernel leaves it alone
                now = FP.bits(g.all)[g.guard:g.guard + g.n].view(L.B, L.Ho, L.Wo, ov.ld)[..., coff + N:coff + N + pad]
                zeros, kept = bool((now == 0).all()), bool((now == FP.NAN32).all())
                if "conv_patch_kernel" in name:
                    assert zeros or var == "mask+acc", what + ": the padding columns must hold zeros"
                    FP.assert_only_slice_written(g, ov, coff, before, what, zero_cols=(pad if zeros else 0), free_cols=pad)
                else:
                    assert kept, what + ": the row padding was written"
                    FP.assert_only_slice_written(g, ov, coff, before, what)
            else:
                FP.assert_only_slice_written(g, ov, coff, before, what)
            rounded, tol = _tolerance(name, prec)
            exp = L.expected(rounded, var, c0, c1)
            got = FP.slice_of(g, ov, coff).double()
            err = (got - exp).abs().max().item() / max(1.0, exp.abs().max().item())
            worst = max(worst, err)
            assert err <= tol, (what, err, tol)
            if var == "plain" and (coff, extra) == check_place:
                assert _family_expected(tag, mode, prec) in name, what
    print("conv footprint %s mode=%d prec=%d: worst relative error %.3g, kernels %s" % (tag, mode, prec, worst, sorted(names)))


def _split(x):
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _guarded_shadow(dev, npix, N):
    """a bf16 shadow [npix][round_up(N, 32)] inside guards, EVERY element (the padding channels included) holding the bf16 sentinel"""
    g = FP.Guarded(npix * ops.shadow_ld(N), torch.bfloat16, dev)
    return g


SHADOW_FAMILIES = [f for f in FAMILIES if f[0] in ("head", "thin", "bank_small", "patch", "patch38", "tiled", "tiled_s2", "scalar")]


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fam", SHADOW_FAMILIES, ids=[f[0] for f in SHADOW_FAMILIES])
def test_conv_shadows_are_the_split_of_the_stored_result(backend, fam, mode, prec):
    """mh_conv2d_sh / mh_conv2d_sh4 with the fp32 result in a slice: hi = bf16(out), lo = bf16(out - hi) bit for bit, the shadows' padding channels
    [N, round_up(N, 32)) are not touched (sentinel, not zero, in front of the launch), nothing around the fp32 slice or the shadows is written."""
    lib, dev = backend.lib, backend.device
    tag, hook, hook_on, hook_off = fam[0], fam[6], fam[7], fam[8]
    L = _layer(fam, mode)
    N, K = L.N, L.K
    w = L.w.to(dev)
    x = _wide(L.x, dev)
    npix = L.B * L.Ho * L.Wo
    sld = ops.shadow_ld(N)
    for entry in ("sh", "sh4"):
        for coff, extra in ((4, 4), (3, 5)):
            g, ov = FP.slice_view(dev, L.B, L.Ho, L.Wo, N, coff, extra)
            ghi, glo = _guarded_shadow(dev, npix, N), _guarded_shadow(dev, npix, N)
            d = ops.conv_desc(L.B, L.Hi, L.Wi, L.Ho, L.Wo, K, N, 3, 3, L.stride, 1, L.pt, L.pl, mode, mode, _ld(K), ov.ld, alpha=(0.2 if mode == 0 else 1.0), precision=prec)
            before = g.snapshot()
            if hook:
                getattr(lib, hook)(hook_on)
            try:
                if entry == "sh":
                    rc = lib._raw_mh_conv2d_sh(C.byref(d), P(x), P(w), None, None, C.c_void_p(ov.ptr), None, C.c_void_p(ghi.ptr()), None)
                else:
                    rc = lib._raw_mh_conv2d_sh4(C.byref(d), P(x), P(w), None, None, C.c_void_p(ov.ptr), None, C.c_void_p(ghi.ptr()), C.c_void_p(glo.ptr()), None)
                name = lib.last_kernel().decode()
            finally:
                if hook:
                    getattr(lib, hook)(hook_off)
            backend.sync()
            what = "%s %s mode=%d prec=%d coff=%d [%s]" % (entry, tag, mode, prec, coff, name)
            assert rc == 0, (what, lib.last_error())
            FP.assert_only_slice_written(g, ov, coff, before, what)
            out = FP.slice_of(g, ov, coff)
            hi, lo = _split(out)
            for gs, want, used in ((ghi, hi, True), (glo, lo, entry == "sh4")):
                gs.assert_guards(what)
                sb = gs.payload_bits().view(npix, sld)
                if not used:
                    assert (sb == FP.NAN16).all()
                    continue
                assert torch.equal(sb[:, :N], FP.bits(want).view(npix, N)), what + ": shadow != split of the stored fp32 result"
                assert (sb[:, N:] == FP.NAN16).all(), what + ": %d padding channels of the shadow were written" % int((sb[:, N:] != FP.NAN16).sum())
            rounded, tol = _tolerance(name, prec)
            exp = L.expected(rounded, "plain", 0, 0)
            assert (out.double() - exp).abs().max().item() <= tol * max(1.0, exp.abs().max().item()), what


def test_conv_shadow_only_leaves_the_fp32_result_alone(backend):
    """mh_conv2d_sh3 with MH_CONV_SHADOW_ONLY on the patch-staged input gradient: the fp32 buffer (a slice here) is bit-untouched, the shadow holds what
    the launch without the flag stores as bf16(out)."""
    lib, dev = backend.lib, backend.device
    fam = [f for f in FAMILIES if f[0] == "patch"][0]
    L = _layer(fam, 1)
    N, K = L.N, L.K
    w = L.w.to(dev); x = L.x.to(dev)
    xs = torch.zeros(L.B, L.Hi, L.Wi, ops.shadow_ld(K), dtype=torch.bfloat16, device=dev); xs[..., :K] = x.bfloat16()
    npix = L.B * L.Ho * L.Wo
    res = {}
    lib.tune_conv_patch(128)
    try:
        for flags in (0, 1):
            g, ov = FP.slice_view(dev, L.B, L.Ho, L.Wo, N, 4, 4)
            gs = _guarded_shadow(dev, npix, N)
            d = ops.conv_desc(L.B, L.Hi, L.Wi, L.Ho, L.Wo, K, N, 3, 3, 1, 1, L.pt, L.pl, 1, 1, K, ov.ld, precision=1)
            assert lib.conv2d_takes_shadows(C.byref(d), P(x), P(w), None, C.c_void_p(ov.ptr), None) & 1
            before = g.snapshot()
            rc = lib._raw_mh_conv2d_sh3(C.byref(d), P(x), P(xs), P(w), None, None, C.c_void_p(ov.ptr), None, None, C.c_void_p(gs.ptr()), flags, None)
            name = lib.last_kernel().decode()
            backend.sync()
            assert rc == 0 and "patch" in name, (rc, name, lib.last_error())
            gs.assert_guards(name)
            if flags:
                FP.assert_untouched(g, before, "MH_CONV_SHADOW_ONLY [%s]" % name)
            else:
                FP.assert_only_slice_written(g, ov, 4, before, name)
                res["out"] = FP.slice_of(g, ov, 4)
            res[flags] = gs.payload_bits().view(npix, ops.shadow_ld(N)).clone()
    finally:
        lib.tune_conv_patch(-1)
    assert torch.equal(res[0], res[1])
    assert torch.equal(res[1][:, :N], FP.bits(res["out"].to(torch.bfloat16)).view(npix, N)) and (res[1][:, N:] == FP.NAN16).all()
    exp = L.expected(True, "plain", 0, 0)
    assert (res["out"].double() - exp).abs().max().item() <= 1e-4 * max(1.0, exp.abs().max().item())


@pytest.mark.parametrize("shape", [(1, 8, 16, 32), (2, 7, 13, 12)])
def test_conv2d_head_extra_slots(backend, shape):
    """mh_conv2d_head: the result also lands in one-channel slots of two wider buffers (a concat member, the buffer the next stage accumulates into):
    the three copies carry the same bits, the slots' neighbours and all guards are untouched."""
    lib, dev = backend.lib, backend.device
    B, H, W, K = shape
    x = _rand((B, H, W, K), 31); w = _rand((3, 3, K, 1), 32, 0.2); b = _rand((1,), 33)
    ref = T.conv2d(x.double(), w.double(), b.double(), 1, 1, 1.0)
    g1, v1 = FP.slice_view(dev, B, H, W, 1, 0, 0)
    g2, v2 = FP.slice_view(dev, B, H, W, 1, 5, 3)
    g3, v3 = FP.slice_view(dev, B, H, W, 1, 0, 2)
    snaps = [g.snapshot() for g in (g1, g2, g3)]
    ops.conv2d_head(lib, ops.view(x.to(dev)), w.to(dev), b.to(dev), v1, copies=(v2, v3))
    name = lib.last_kernel().decode()
    backend.sync()
    for g, v, coff, s in ((g1, v1, 0, snaps[0]), (g2, v2, 5, snaps[1]), (g3, v3, 0, snaps[2])):
        FP.assert_only_slice_written(g, v, coff, s, "head [%s]" % name)
    o1, o2, o3 = FP.slice_of(g1, v1, 0), FP.slice_of(g2, v2, 5), FP.slice_of(g3, v3, 0)
    assert torch.equal(FP.bits(o1), FP.bits(o2)) and torch.equal(FP.bits(o1), FP.bits(o3))
    err = (o1.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


# (B, H, W, K, N, dil): every N % 8 == 0 the MADNet instances serve that no layer of either net has, at the K-step counts 2 / 3 / 5 / 8
PLANES_CASES = [(1, 7, 45, 32, 8, 1), (1, 14, 19, 38, 16, 4), (2, 5, 21, 70, 24, 1), (1, 9, 33, 128, 40, 16), (1, 13, 17, 32, 56, 4), (1, 6, 41, 38, 72, 1),
                (1, 11, 23, 70, 88, 16), (1, 8, 37, 128, 104, 1), (1, 10, 29, 32, 120, 4),
                (1, 7, 21, 136, 40, 1)]              # K = 136: the K-chunked kernel, plain bf16 (precision 1)


@pytest.mark.parametrize("case", PLANES_CASES, ids=lambda c: "K%d_N%d_d%d" % (c[3], c[4], c[5]))
def test_conv2d_planes_into_slices(backend, case):
    """mh_conv2d_planes with its fp32 result in a 16-byte aligned slice (how dispnet_engine stores it into concat storages) and its planes in rows of
    round_up(N, 32): neighbours, the planes' padding channels and all guards untouched; planes == split of the fp32 result; values against the
    float64 oracle (4e-5: split-bf16; the chunked bf16 shape against bf16-rounded operands, 3e-5).  A misaligned slice is refused with MH_ERR_ALIGN
    ("out rows must be 16-byte aligned") and nothing is written."""
    lib, dev = backend.lib, backend.device
    B, H, W, K, N, dil = case
    bf16 = K > 128
    x = _rand((B, H, W, K), 211); w = _rand((3, 3, K, N), 212, 0.2 if not bf16 else 0.05); b = _rand((N,), 213)
    if bf16:
        ref = T.conv2d(_bf(x).double(), _bf(w).double(), b.double(), 1, dil, 0.2); tol = 3e-5
    else:
        ref = T.conv2d(x.double(), w.double(), b.double(), 1, dil, 0.2); tol = 4e-5
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    keep = []
    assert ops.conv2d_planes_ok(lib, ops.view(xd), wd, dil, bf16=bf16)
    xp = ops.Planes(ops.Shadow(B, H, W, K, dev), dev)
    ops.plane_split(lib, [(ops.view(xd), xp)], dev, keep)
    planes = 1 if bf16 else 2
    nbytes = ops.pack_bytes(wd, planes, 2)
    assert nbytes == lib.pack32_bytes(9, K, N) // (2 // planes)
    bank = torch.zeros(nbytes // 4, device=dev)
    ops.pack_weights(lib, [(wd, bank, planes, 2)], dev, keep)
    npix, pld = B * H * W, ops.shadow_ld(N)
    lib.tune_conv_planes(0)
    for coff, extra, ok in ((4, 4, True), (0, 4, True), (3, 5, False), (4, 3, False)):
        g, ov = FP.slice_view(dev, B, H, W, N, coff, extra)
        ghi, glo = _guarded_shadow(dev, npix, N), _guarded_shadow(dev, npix, N)
        before = g.snapshot()
        d = ops.conv_desc(B, H, W, H, W, K, N, 3, 3, 1, dil, dil, dil, 0, 0, 0, ov.ld, alpha=0.2, precision=1 if bf16 else 2)
        rc = lib._raw_mh_conv2d_planes(C.byref(d), C.c_void_p(xp.hi.ptr), (None if bf16 else C.c_void_p(xp.lo.ptr)), xp.ld, P(bank), P(bd), C.c_void_p(ov.ptr),
                                       C.c_void_p(ghi.ptr()), (None if bf16 else C.c_void_p(glo.ptr())), pld, None)
        name = lib.last_kernel().decode() if rc == 0 else "-"
        backend.sync()
        what = "planes K=%d N=%d dil=%d coff=%d extra=%d [%s]" % (K, N, dil, coff, extra, name)
        if not ok:
            assert rc == -2, (what, rc)                      # MH_ERR_ALIGN
            FP.assert_untouched(g, before, what); FP.assert_untouched(ghi, ghi.snapshot() * 0 + FP.NAN16, what)
            continue
        assert rc == 0, (what, lib.last_error())
        assert ("conv_planes_ck_kernel" in name) == bf16 and "conv_planes" in name, what
        FP.assert_only_slice_written(g, ov, coff, before, what)
        out = FP.slice_of(g, ov, coff)
        err = (out.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err <= tol, (what, err)
        hi, lo = _split(out)
        for gs, want, used in ((ghi, hi, True), (glo, lo, not bf16)):
            gs.assert_guards(what)
            sb = gs.payload_bits().view(npix, pld)
            if used:
                assert torch.equal(sb[:, :N], FP.bits(want).view(npix, N)), what + ": plane != split of the stored fp32 result"
                assert (sb[:, N:] == FP.NAN16).all(), what + ": padding channels of a result plane were written"
            else:
                assert (sb == FP.NAN16).all()
    lib.tune_conv_planes(0)
    print("planes K=%d N=%d dil=%d: relative error %.3g" % (K, N, dil, err))


# (B, H, W, Cin, Cout, dil, stride, mask range): dx rows of round_up(Cin, 8) floats with NOTHING behind the last row but the guard
PLANES_BWD_CASES = [(1, 9, 21, 33, 64, 1, 1, None), (1, 7, 19, 38, 64, 4, 1, (8, 30)), (2, 6, 17, 64, 32, 1, 1, (16, 48)), (1, 6, 10, 24, 32, 1, 2, None),
                    (1, 5, 20, 40, 136, 1, 1, (8, 24))]


@pytest.mark.parametrize("case", PLANES_BWD_CASES, ids=lambda c: "Cin%d_Cout%d_d%d_s%d" % (c[3], c[4], c[5], c[6]))
def test_conv2d_planes_bwd_rows_of_cin_rounded_up_to_8(backend, case):
    """mh_conv2d_planes_bwd: "dx rows must hold Cin rounded up to 8 ... the padding columns receive zeros" -- with the buffer ending exactly behind the
    last row's padding; sub-range leaky mask; one stride-2 layer; one K-chunked reduction (Cout = 136)."""
    lib, dev = backend.lib, backend.device
    B, Hz, Wz, Ci, Co, dil, stride, mrange = case
    H, W = Hz * stride, Wz * stride
    dz = _rand((B, Hz, Wz, Co), 411); w = _rand((3, 3, Ci, Co), 412, 0.2 if Co <= 128 else 0.05); x = _rand((B, H, W, Ci), 413)
    xin = torch.zeros(B, H, W, Ci, dtype=torch.float64, requires_grad=True)
    (g_ref,) = torch.autograd.grad(T.conv2d(xin, _bf(w).double(), None, stride=stride, dilation=dil, alpha=1.0), xin, _bf(dz).double())
    mk = torch.where(x.double() > 0, 1.0, 0.2)
    if mrange is not None:
        mk[..., :mrange[0]] = 1.0; mk[..., mrange[1]:] = 1.0
    g_ref = g_ref * mk
    keep = []
    dzd, wd, xd = dz.to(dev), w.to(dev), x.to(dev)
    dzs = ops.Shadow(B, Hz, Wz, Co, dev); xs = ops.Shadow(B, H, W, Ci, dev); dxs = ops.Shadow(B, H, W, Ci, dev)
    ops.shadow_cast(lib, [(ops.view(dzd), dzs), (ops.view(xd), xs)], dev, keep)
    bank = torch.zeros(ops.pack_bytes(wd, 1, 3) // 4, device=dev)
    assert ops.pack_bytes(wd, 1, 3) == lib.pack32_bytes(9, Co, Ci) // 2
    ops.pack_weights(lib, [(wd, bank, 1, 3)], dev, keep)
    pad = FP.round_up(Ci, 8) - Ci
    g, dx = FP.slice_view(dev, B, H, W, Ci, 0, pad)
    assert ops.conv2d_planes_bwd_ok(lib, dx, wd, dil, stride=stride)
    before = g.snapshot()
    lib.tune_conv_planes(0)
    ops.conv2d_planes_bwd(lib, dzs, wd, bank, dx=dx, dx_shadow=dxs, mask_shadow=xs, mask_alpha=0.2, dil=dil, mask_range=(mrange or (0, 0)), stride=stride)
    name = lib.last_kernel().decode()
    backend.sync()
    lib.tune_conv_planes(0)
    assert ("conv_planes_ck_kernel" in name) == (Co > 128) and ("s2bwd" in name) == (stride == 2), name
    FP.assert_only_slice_written(g, dx, 0, before, "planes_bwd [%s]" % name, zero_cols=pad)
    out = FP.slice_of(g, dx, 0)
    tol = 3e-5 if Co > 128 else 2e-5
    err = (out.double() - g_ref).abs().max().item() / max(1.0, g_ref.abs().max().item())
    print("planes_bwd %s: relative error %.3g [%s]" % (case, err, name))
    assert err <= tol, (err, name)
    assert torch.equal(dxs.t.cpu()[..., :Ci], out.to(torch.bfloat16)) and not dxs.t.cpu()[..., Ci:].float().abs().sum()


@pytest.mark.parametrize("case", [(2, 11, 14, 8, 2), (1, 30, 23, 16, 1)])
def test_conv_image_fwd_into_wider_rows(backend, case):
    """mh_conv_image_fwd with out_ld = 24 > N = 16: columns 16 .. 23 of every row and the guards are untouched"""
    lib, dev = backend.lib, backend.device
    NB, H0, W0, factor, stride = case
    frames = torch.floor(torch.rand(NB, H0, W0, 3, generator=torch.Generator().manual_seed(11)) * 256)
    w = _rand((3, 3, 3, 16), 12, 0.3); b = _rand((16,), 13)
    xp = T.pad_image(frames, factor)
    Hp, Wp = xp.shape[1], xp.shape[2]
    ref = T.conv2d(xp.double(), w.double(), b.double(), stride, 1, 0.2)
    Ho, Wo = ref.shape[1], ref.shape[2]
    g, ov = FP.slice_view(dev, NB, Ho, Wo, 16, 0, 8)
    assert ov.ld == 24
    before = g.snapshot()
    ops.conv_image_fwd(lib, frames.to(dev), Hp, Wp, (Hp - H0) // 2, (Wp - W0) // 2, w.to(dev), b.to(dev), ov, stride=stride, alpha=0.2)
    name = lib.last_kernel().decode()
    backend.sync()
    assert "conv_image_fwd_kernel" in name
    FP.assert_only_slice_written(g, ov, 0, before, name)
    err = (FP.slice_of(g, ov, 0).double() - ref).abs().max().item()
    assert err <= 2e-6 * max(1.0, ref.abs().max().item()), err          # the bound of test_conv_image_fwd_from_the_frames
