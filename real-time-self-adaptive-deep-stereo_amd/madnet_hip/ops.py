"""Host-side operator layer: torch tensors (storage only) -> C-ABI calls.

Mirrors the operator set of Nets/sharedLayers.py:23-92 and Data_utils/preprocessing.py /
Losses/loss_factory.py hot functions, with explicit forward and gradient entry points (the
reference gets its gradients from TF's autodiff; here every gradient is a hand-written kernel).

All tensors are float32 NHWC.  A `View` is (pointer, B, H, W, C, ld): a channel slice of a
possibly wider buffer, which is how tf.concat is made free.
"""
import ctypes as C
import torch
from . import _ffi


def same_pad(in_size, k, stride=1, dilation=1):
    """TF 'SAME': out=ceil(in/s), pad_total=max((out-1)*s+keff-in,0), before=total//2."""
    keff = (k - 1) * dilation + 1
    out = -(-in_size // stride)
    total = max((out - 1) * stride + keff - in_size, 0)
    return out, total // 2, total - total // 2


class View(object):
    __slots__ = ("t", "ptr", "B", "H", "W", "C", "ld")

    def __init__(self, t, B, H, W, C_, ld, coff=0):
        self.t, self.B, self.H, self.W, self.C, self.ld = t, B, H, W, C_, ld
        self.ptr = t.data_ptr() + 4 * coff

    @property
    def npix(self):
        return self.B * self.H * self.W

    def slice(self, c0, c1):
        v = View(self.t, self.B, self.H, self.W, c1 - c0, self.ld)
        v.ptr = self.ptr + 4 * c0
        return v


def view(t):
    """View of a plain contiguous [B,H,W,C] (or [B,H,W]) float32 tensor."""
    assert t.dtype == torch.float32 and t.is_contiguous(), "float32 contiguous tensors only"
    if t.dim() == 3:
        B, H, W = t.shape
        return View(t, B, H, W, 1, 1)
    B, H, W, Cc = t.shape
    return View(t, B, H, W, Cc, Cc)


def _p(x):
    if x is None:
        return None
    if isinstance(x, View):
        return C.c_void_p(x.ptr)
    if isinstance(x, torch.Tensor):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x)


def conv_desc(B, Hi, Wi, Ho, Wo, K, N, kh, kw, stride, dil, pad_t, pad_l, mode, w_trans,
              in_ld, out_ld, mask_ld=0, accumulate=0, alpha=1.0, mask_alpha=1.0, mask_c0=0, mask_c1=0, precision=None):
    return _ffi.ConvDesc(B, Hi, Wi, Ho, Wo, K, N, kh, kw, stride, dil, pad_t, pad_l, mode, w_trans,
                         in_ld, out_ld, mask_ld, accumulate, alpha, mask_alpha, mask_c0, mask_c1,
                         PRECISION if precision is None else precision)


# module-wide arithmetic mode of the conv family while a plan is being recorded (mh_conv_desc.precision codes):
#   0 = exact fp32 MFMA (the parity path)      1 = bf16 MFMA operands, fp32 accumulate (throughput)
#   2 = split-bf16 ("bf16x3"): every fp32 operand is carried as hi + lo bf16 and a product costs three bf16 MFMAs
#       (hi*hi + hi*lo + lo*hi, fp32 accumulate): ~2^-16 relative error per product instead of 2^-8.  Kernels without an x3
#       instance run exact fp32 for this code.
# PRECISION applies to the forward convolutions, PRECISION_BWD (None = same) to input and filter gradients.
# Engine precision names -> (forward, backward):
#   'fp32'  (0, 0)   'bf16' (1, 1)
#   'mixed' (2, 1)   forward within the 1e-3 px EPE tolerance of the fp32 oracle, gradients in bf16 (a gradient error moves
#                    the NEXT frame's weights by lr * |dg|; the disparity of the current frame never sees it)
PRECISION = 0
PRECISION_BWD = None
PRECISION_CODES = {"fp32": (0, 0), "bf16": (1, 1), "mixed": (2, 1)}


class precision_scope(object):
    """with precision_scope('mixed'): ... -- sets PRECISION / PRECISION_BWD while a plan is recorded."""

    def __init__(self, name):
        if name not in PRECISION_CODES:
            raise ValueError("precision must be one of %s" % sorted(PRECISION_CODES))
        self.codes = PRECISION_CODES[name]

    def __enter__(self):
        global PRECISION, PRECISION_BWD
        self.saved = (PRECISION, PRECISION_BWD)
        PRECISION, PRECISION_BWD = self.codes
        return self

    def __exit__(self, *a):
        global PRECISION, PRECISION_BWD
        PRECISION, PRECISION_BWD = self.saved
        return False


def _bwd_precision():
    return PRECISION if PRECISION_BWD is None else PRECISION_BWD


def conv_geometry(H, W, kh, kw, stride, dil):
    Ho, pt, _ = same_pad(H, kh, stride, dil)
    Wo, pl, _ = same_pad(W, kw, stride, dil)
    return Ho, Wo, pt, pl


def _fwd_desc(x, w, out, stride, dil, precision, **kw):
    """descriptor of the forward conv x -> out (Views; w: HWIO); precision None = the recording's forward code"""
    kh, kw_, cin, cout = w.shape
    Ho, Wo, pt, pl = conv_geometry(x.H, x.W, kh, kw_, stride, dil)
    assert (out.H, out.W, out.C) == (Ho, Wo, cout) and x.C == cin
    return conv_desc(x.B, x.H, x.W, Ho, Wo, cin, cout, kh, kw_, stride, dil, pt, pl, 0, 0, x.ld, out.ld, precision=precision, **kw)


def _dgrad_desc(dz, w, dx, stride, dil, precision, **kw):
    """descriptor of the input gradient dz -> dx of that conv; precision None = the recording's backward code"""
    kh, kw_, cin, cout = w.shape
    Ho, Wo, pt, pl = conv_geometry(dx.H, dx.W, kh, kw_, stride, dil)
    assert (dz.H, dz.W, dz.C) == (Ho, Wo, cout) and dx.C == cin
    return conv_desc(dx.B, Ho, Wo, dx.H, dx.W, cout, cin, kh, kw_, stride, dil, pt, pl, 1, 1, dz.ld, dx.ld,
                     precision=(_bwd_precision() if precision is None else precision), **kw)


def conv2d_takes_bank(qlib, x, w, out, stride, dil, mode, precision, mask_ref=None):
    """mh_conv2d_takes_bank (qlib = the real library): would conv2d_fwd (mode 0: x -> out) / conv2d_dgrad (mode 1: x = dz, out = dx) of this layer in
    this precision code read a fragment bank if it were given one?"""
    d = (_dgrad_desc if mode else _fwd_desc)(x, w, out, stride, dil, precision, mask_ld=(mask_ref.ld if mask_ref is not None else 0))
    return qlib.conv2d_takes_bank(C.byref(d), _p(x), _p(w), _p(out), _p(mask_ref)) == 1


def conv2d_fwd(lib, x, w, b, out, stride=1, dil=1, alpha=1.0, accumulate=False, mask_ref=None, mask_alpha=1.0,
               mask_range=(0, 0), stream=None, precision=None, wb=None, shadow=None, out_planes=None):
    """out (+)= leaky(conv2d_SAME(x, w) + b) [* leaky'(mask_ref)].  x,out: View; w: HWIO [kh,kw,Cin,Cout].
    wb: the layer's MFMA fragment bank (pack_weights) -- split-bf16 3x3 layers then stream their weights from it.
    out_planes: Planes of `out` (hi + lo) the launch writes too (mh_conv2d_sh4: the producer side of conv2d_planes)."""
    d = _fwd_desc(x, w, out, stride, dil, precision, alpha=alpha, mask_ld=(mask_ref.ld if mask_ref is not None else 0), accumulate=int(accumulate),
                  mask_alpha=mask_alpha, mask_c0=mask_range[0], mask_c1=mask_range[1])
    if out_planes is not None:
        assert (out_planes.B, out_planes.H, out_planes.W, out_planes.C) == (out.B, out.H, out.W, out.C)
        lib.conv2d_sh4(C.byref(d), _p(x), _p(w), _p(wb), _p(b), _p(out), _p(mask_ref), C.c_void_p(out_planes.hi.ptr), C.c_void_p(out_planes.lo.ptr), _p(stream))
    elif shadow is not None:     # shadow: ops.Shadow of `out` -- the epilogue also writes bf16(out) there (operand of wgrad_stream)
        assert (shadow.B, shadow.H, shadow.W, shadow.C) == (out.B, out.H, out.W, out.C)
        lib.conv2d_sh(C.byref(d), _p(x), _p(w), _p(wb), _p(b), _p(out), _p(mask_ref), C.c_void_p(shadow.ptr), _p(stream))
    elif wb is not None:
        lib.conv2d_wb(C.byref(d), _p(x), _p(w), _p(wb), _p(b), _p(out), _p(mask_ref), _p(stream))
    else:
        lib.conv2d(C.byref(d), _p(x), _p(w), _p(b), _p(out), _p(mask_ref), _p(stream))


PLANES_WHOLE_MAX = int(__import__("os").environ.get("MH_PLANES_WHOLE_MAX", "8"))      # must equal the library's build (csrc/conv_planes.hip: MH_PLANES_WHOLE_MAX)


def planes_kc16(K):
    """layout rule of the 32x32x16 bank images (mh_planes_kc16; tests assert that the two agree): 0 = whole-K, else the K-chunk in 16-channel steps"""
    k16 = (K + 15) // 16
    return 0 if (k16 <= PLANES_WHOLE_MAX or k16 == 13) else 4


def check_planes_rule(qlib):
    """the bank layout rule lives twice (here for sizing, in the library for the kernels): refuse to run on a library built with another rule"""
    for K in (16, 97, 112, 128, 129, 193, 208, 256, 385, 1025):
        if int(qlib.planes_kc16(K)) != planes_kc16(K):
            raise RuntimeError("libmadnet_hip: mh_planes_kc16(%d) = %d, host rule %d (MH_PLANES_WHOLE_MAX mismatch)" % (K, qlib.planes_kc16(K), planes_kc16(K)))


def _k16_padded(K):
    k16, kc = (K + 15) // 16, planes_kc16(K)
    return (k16 + kc - 1) // kc * kc if kc else k16


def pack_bytes(w, planes=2, trans=0):
    kh, kw, K, N = w.shape
    if trans == 2:          # the 32x32x16 register image of conv2d_planes (hi + lo, or hi only: plain bf16 forward)
        return kh * kw * _k16_padded(K) * ((N + 31) // 32) * 1024 * planes
    if trans == 3:          # ... of conv2d_planes_bwd: one plane, reduction over Cout, columns = Cin
        return kh * kw * _k16_padded(N) * ((K + 31) // 32) * 1024
    if trans:
        K, N = N, K
    return kh * kw * ((K + 31) // 32) * ((N + 15) // 16) * planes * 1024


def pack_weights(lib, pairs, device, keep, stream=None):
    """pairs: [(src HWIO tensor, dst tensor of pack_bytes(src, planes, trans) bytes[, planes = 2[, trans = 0]])] -> every dst = the MFMA
    fragment bank of src (include/madnet_hip.h: mh_pack_weights), ONE launch.  planes 2 = hi + lo (split-bf16 forward), 1 = bf16;
    trans 1 = the bank the input gradient reads (reduction over Cout).  `keep`: list that keeps the device table alive as long as the plan."""
    if not pairs:
        return
    arr = (_ffi.PackSeg * len(pairs))()
    blk = 0
    for i, pr in enumerate(pairs):
        src, dst = pr[0], pr[1]
        planes = pr[2] if len(pr) > 2 else 2
        trans = pr[3] if len(pr) > 3 else 0
        kh, kw, K, N = src.shape
        if trans in (1, 3):
            K, N = N, K
        assert dst.numel() * dst.element_size() >= pack_bytes(src, planes, trans) and dst.data_ptr() % 16 == 0
        assert (trans != 3 or planes == 1)
        arr[i].src, arr[i].dst, arr[i].taps, arr[i].K, arr[i].N = src.data_ptr(), dst.data_ptr(), kh * kw, K, N
        arr[i].planes, arr[i].blk0, arr[i].trans = planes, blk, trans
        arr[i].kc16 = planes_kc16(K) if trans in (2, 3) else 0
        if trans in (2, 3):
            blk += (kh * kw * _k16_padded(K) * ((N + 31) // 32) * 64 + 255) // 256
        else:
            blk += (kh * kw * ((K + 31) // 32) * ((N + 15) // 16) * 64 + 255) // 256
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    keep.append(table)
    lib.pack_weights(C.c_void_p(table.data_ptr()), len(pairs), blk, _p(stream))


def conv2d_dgrad(lib, dz, w, dx, stride=1, dil=1, accumulate=False, mask_ref=None, mask_alpha=1.0, mask_range=(0, 0),
                 stream=None, wb=None, shadow=None, dz_shadow=None, mask_shadow=None):
    """dx (+)= conv2d_backprop_input(dz, w); optionally fused dx *= leaky'(mask_ref).
    dz: View [B,Ho,Wo,Cout]; dx: View [B,H,W,Cin]; w: HWIO of the forward conv."""
    d = _dgrad_desc(dz, w, dx, stride, dil, None, mask_ld=(mask_ref.ld if mask_ref is not None else 0), accumulate=int(accumulate),
                    mask_alpha=mask_alpha, mask_c0=mask_range[0], mask_c1=mask_range[1])
    if dz_shadow is not None or mask_shadow is not None:
        # dz_shadow / mask_shadow: ops.Shadow of dz / of mask_ref that a producer already wrote: the patch-staged kernel stages the first instead of
        # converting dz and tests the sign of the second instead of reading the fp32 activation (other kernels ignore both)
        assert dz_shadow is None or (dz_shadow.B, dz_shadow.H, dz_shadow.W, dz_shadow.C) == (dz.B, dz.H, dz.W, dz.C)
        assert mask_shadow is None or (mask_ref is not None and (mask_shadow.B, mask_shadow.H, mask_shadow.W, mask_shadow.C) == (dx.B, dx.H, dx.W, dx.C))
        assert shadow is None or (shadow.B, shadow.H, shadow.W, shadow.C) == (dx.B, dx.H, dx.W, dx.C)
        sp = lambda sh: C.c_void_p(sh.ptr) if sh is not None else None
        lib.conv2d_sh3(C.byref(d), _p(dz), sp(dz_shadow), _p(w), _p(wb), None, _p(dx), _p(mask_ref), sp(mask_shadow), sp(shadow), 0, _p(stream))
    elif shadow is not None:   # shadow: ops.Shadow of dx, written by the epilogue (dx is the next layer's dz operand of wgrad_stream)
        assert (shadow.B, shadow.H, shadow.W, shadow.C) == (dx.B, dx.H, dx.W, dx.C)
        lib.conv2d_sh(C.byref(d), _p(dz), _p(w), _p(wb), None, _p(dx), _p(mask_ref), C.c_void_p(shadow.ptr), _p(stream))
    elif wb is not None:       # wb: pack_weights(trans=1, planes=1) bank of w -- the small-layer bank kernel takes it in the bf16 mode
        lib.conv2d_wb(C.byref(d), _p(dz), _p(w), _p(wb), None, _p(dx), _p(mask_ref), _p(stream))
    else:
        lib.conv2d(C.byref(d), _p(dz), _p(w), None, _p(dx), _p(mask_ref), _p(stream))


def conv2d_wgrad(lib, x, dz, dw, db, stride=1, dil=1, stream=None):
    """dw += conv2d_backprop_filter(x, dz) ; db += sum(dz).  dw: HWIO tensor (pre-zeroed)."""
    kh, kw, cin, cout = dw.shape
    Ho, Wo, pt, pl = conv_geometry(x.H, x.W, kh, kw, stride, dil)
    assert (dz.H, dz.W, dz.C) == (Ho, Wo, cout) and x.C == cin
    d = conv_desc(x.B, x.H, x.W, Ho, Wo, cin, cout, kh, kw, stride, dil, pt, pl, 0, 0, x.ld, dz.ld, precision=_bwd_precision())
    lib.conv2d_wgrad(C.byref(d), _p(x), _p(dz), dz.ld, _p(dw), _p(db), _p(stream))


class WgradWorkspace(object):
    """Arena for the per-split partial filter gradients of one training step + the segment table the single
    reduction launch walks (mh_conv2d_wgrad_partial / mh_wgrad_reduce).  The arena is transient within one plan
    execution, so every plan of an engine shares it (`reset()` at the start of each plan build); chunks are never
    freed or moved because recorded plans hold raw pointers into them."""
    CHUNK = 64 << 20            # floats per arena chunk (256 MiB)

    def __init__(self, device):
        self.device = device
        self.chunks = []
        self.reset()

    def reset(self):
        self.ci, self.off = 0, 0

    def alloc(self, nfloats):
        nfloats = (nfloats + 3) // 4 * 4
        while True:
            if self.ci == len(self.chunks):
                self.chunks.append(torch.empty(max(self.CHUNK, nfloats), dtype=torch.float32, device=self.device))
                self.off = 0
            c = self.chunks[self.ci]
            if self.off + nfloats <= c.numel():
                p = c.data_ptr() + 4 * self.off
                self.off += nfloats
                return p
            self.ci += 1
            self.off = 0

    @property
    def nbytes(self):
        return sum(c.numel() for c in self.chunks) * 4


def conv2d_wgrad_partial(lib, qlib, wsa, segs, x, dz, dw, db, stride=1, dil=1, stream=None, direct_ok=True):
    """Like conv2d_wgrad, but atomic-free: the pixel splits' partial sums go to the arena `wsa` and a segment
    (ws, dst=dw, size, splits) is appended to `segs` for the step's single wgrad_reduce launch.
    `qlib` is the real library (split-count query); `lib` may be a Recorder.  direct_ok=False: dw already receives
    another contribution in this step (shared weights) -- always go through a segment."""
    kh, kw, cin, cout = dw.shape
    Ho, Wo, pt, pl = conv_geometry(x.H, x.W, kh, kw, stride, dil)
    assert (dz.H, dz.W, dz.C) == (Ho, Wo, cout) and x.C == cin
    d = conv_desc(x.B, x.H, x.W, Ho, Wo, cin, cout, kh, kw, stride, dil, pt, pl, 0, 0, x.ld, dz.ld, precision=_bwd_precision())
    splits = C.c_int32(0)
    qlib.conv2d_wgrad_partial(C.byref(d), _p(x), _p(dz), dz.ld, None, C.byref(splits), None, None)
    size = dw.numel()
    if splits.value == 1 and direct_ok and dw.data_ptr() % 16 == 0:
        # a single split IS the gradient: let it store straight into dw (same [tap][K][N] layout), nothing to reduce
        lib.conv2d_wgrad_partial(C.byref(d), _p(x), _p(dz), dz.ld, C.c_void_p(dw.data_ptr()), C.byref(splits), _p(db), _p(stream))
        return
    # with several splits the kernels store the bias partial sums behind the filter partials, ws[splits][size] | [splits][cout] (no float atomics:
    # bit-identical replays); the same reduction launch sums them in split order
    nb = cout * splits.value if (db is not None and splits.value > 1) else 0
    ws = wsa.alloc(size * splits.value + nb)
    lib.conv2d_wgrad_partial(C.byref(d), _p(x), _p(dz), dz.ld, C.c_void_p(ws), C.byref(splits), _p(db), _p(stream))
    segs.append((ws, dw.data_ptr(), size, splits.value))
    if nb:
        segs.append((ws + 4 * size * splits.value, db.data_ptr(), cout, splits.value, 1))      # db += (the step zeroes its gradient ranges first)


def wgrad_reduce(lib, segs, device, keep, stream=None, accumulate=False):
    """One launch that sums the splits of every segment recorded by conv2d_wgrad_partial.  `keep`: list that
    keeps the device table alive as long as the plan.  accumulate: dst += sum (a weight used by a second conv --
    its segments go into a second launch after the first)."""
    if not segs:
        return
    assert len(set(s[1] for s in segs)) == len(segs), "a filter gradient may appear once per reduction"
    arr = (_ffi.WgradSeg * len(segs))()
    blk = 0
    for k, sg in enumerate(segs):
        ws, dst, size, splits = sg[:4]
        # a 5th field = the segment's own accumulate flag (bias partial sums: always dst += sum onto the zeroed gradient range, so that a single-split use
        # of a shared weight -- an atomic addend -- is never overwritten)
        arr[k].ws, arr[k].dst, arr[k].size, arr[k].splits, arr[k].blk0, arr[k].accumulate = ws, dst, size, splits, blk, int(sg[4] if len(sg) > 4 else accumulate)
        blk += (size + 1023) // 1024
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    table = host.to(device)
    keep.append(table)
    lib.wgrad_reduce(C.c_void_p(table.data_ptr()), len(segs), blk, _p(stream))


def shadow_ld(c):
    """channel stride of the bf16 shadow of a C-channel tensor: C rounded up to 32 (the padding channels stay zero)"""
    return (c + 31) // 32 * 32


class Shadow(object):
    """bf16 NHWC copy of an fp32 tensor for the streaming filter-gradient kernel (mh_wgrad_stream): [B,H,W,shadow_ld(C)], pad = 0."""
    __slots__ = ("t", "B", "H", "W", "C", "ld")

    def __init__(self, B, H, W, C_, device):
        self.B, self.H, self.W, self.C, self.ld = B, H, W, C_, shadow_ld(C_)
        self.t = torch.zeros(B, H, W, self.ld, dtype=torch.bfloat16, device=device)

    @property
    def ptr(self):
        return self.t.data_ptr()


class Planes(object):
    """An activation as TWO bf16 NHWC planes, hi = bf16(x) and lo = bf16(x - hi) ([B,H,W,shadow_ld(C)], pad = 0): the operand format of
    conv2d_planes (csrc/conv_planes.hip).  `hi` is an ordinary Shadow -- the one the streamed filter gradient and the input gradients read."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo=None):
        """lo: the lo plane's Shadow | None = hi only (the one-plane forms) | a device: the lo plane is allocated there"""
        self.hi = hi
        self.lo = lo if (lo is None or isinstance(lo, Shadow)) else Shadow(hi.B, hi.H, hi.W, hi.C, lo)

    B = property(lambda self: self.hi.B)
    H = property(lambda self: self.hi.H)
    W = property(lambda self: self.hi.W)
    C = property(lambda self: self.hi.C)
    ld = property(lambda self: self.hi.ld)


def as_planes(x):
    """the one handle of the plane wrappers: a Planes as it is, a bare Shadow as the hi-only Planes on it"""
    return x if isinstance(x, Planes) else Planes(x)


def conv2d_planes_ok(qlib, x, w, dil=1, bf16=False, stride=1):
    """does conv2d_planes have an instance for this 'SAME' layer -- stride 1: 3x3 (dilated); stride 2 (round 6): 3x3 / 5x5 on even sizes?  (qlib = the real
    library; bf16: the one-plane form)"""
    kh, kw, cin, cout = w.shape
    if stride == 2:
        if kh != kw or kh not in (3, 5) or dil != 1 or x.H % 2 or x.W % 2:
            return False
        pad = (kh - 2) // 2
        d = conv_desc(x.B, x.H, x.W, x.H // 2, x.W // 2, cin, cout, kh, kw, 2, 1, pad, pad, 0, 0, 0, 0, precision=1 if bf16 else 2)
        return qlib.conv2d_planes_ok(C.byref(d)) == 1
    if (kh, kw) != (3, 3) or stride != 1:
        return False
    d = conv_desc(x.B, x.H, x.W, x.H, x.W, cin, cout, 3, 3, 1, dil, dil, dil, 0, 0, 0, 0, precision=1 if bf16 else 2)
    return qlib.conv2d_planes_ok(C.byref(d)) == 1


def conv2d_planes(lib, xp, w, wb32, b, out=None, out_planes=None, dil=1, alpha=1.0, stream=None, bf16=False, stride=1):
    """leaky(conv2d_SAME(x, w) + b) in split-bf16 from the input's planes `xp` (Planes); results: `out` (fp32 View or None) and / or
    `out_planes` (Planes, or a bare Shadow = hi plane only).  wb32: pack_weights(trans = 2) bank of w.
    bf16: plain bf16 (one MFMA per product) from the hi plane alone -- xp may be a bare Shadow, wb32 the ONE-plane bank (pack planes = 1)."""
    kh, kw, cin, cout = w.shape
    assert xp.C == cin and ((kh, kw) == (3, 3) if stride == 1 else (stride == 2 and kh == kw and dil == 1 and xp.H % 2 == 0 and xp.W % 2 == 0))
    xp = Planes(as_planes(xp).hi) if bf16 else as_planes(xp)
    Ho, Wo = xp.H // stride, xp.W // stride
    pad = dil if stride == 1 else (kh - 2) // 2                  # TF 'SAME': stride 2 on even sizes pads (k - 2) // 2 in front
    d = conv_desc(xp.B, xp.H, xp.W, Ho, Wo, cin, cout, kh, kw, stride, dil, pad, pad, 0, 0, 0, (out.ld if out is not None else 0), alpha=alpha,
                  precision=1 if bf16 else 2)
    ohi = olo = None
    opld = 0
    if out_planes is not None:
        hi, lo = as_planes(out_planes).hi, as_planes(out_planes).lo
        assert (hi.B, hi.H, hi.W, hi.C) == (xp.B, Ho, Wo, cout)
        ohi, olo, opld = C.c_void_p(hi.ptr), (C.c_void_p(lo.ptr) if lo is not None else None), hi.ld
    if out is not None:
        assert (out.B, out.H, out.W, out.C) == (xp.B, Ho, Wo, cout)
    lib.conv2d_planes(C.byref(d), C.c_void_p(xp.hi.ptr), (C.c_void_p(xp.lo.ptr) if xp.lo is not None else None), xp.ld, _p(wb32), _p(b), _p(out), ohi, olo, opld,
                      _p(stream))


def conv2d_planes_bwd_ok(qlib, dx, w, dil=1, stride=1):
    """does conv2d_planes_bwd have an instance for the input gradient of this 'SAME' 3x3 layer (w: HWIO of the forward layer; stride 1, or stride 2 on
    even sizes)?"""
    kh, kw, cin, cout = w.shape
    if stride == 2:
        if kh != kw or kh not in (3, 5) or dil != 1 or dx.H % 2 or dx.W % 2:
            return False
        pad = (kh - 2) // 2
        d = conv_desc(dx.B, dx.H, dx.W, dx.H // 2, dx.W // 2, cin, cout, kh, kw, 2, 1, pad, pad, 0, 0, dx.ld, 0, precision=1)
    elif (kh, kw) != (3, 3):
        return False
    else:
        d = conv_desc(dx.B, dx.H, dx.W, dx.H, dx.W, cin, cout, 3, 3, 1, dil, dil, dil, 0, 0, dx.ld, 0, precision=1)
    return qlib.conv2d_planes_bwd_ok(C.byref(d)) == 1


def conv2d_planes_bwd(lib, dz_shadow, w, wb32t, dx=None, dx_shadow=None, mask_shadow=None, mask_alpha=1.0, dil=1, stream=None, mask_range=(0, 0), stride=1, accumulate=False):
    """dx = conv2d_backprop_input(dz, w) * leaky'(mask) from the bf16 shadow of dz (mh_conv2d_planes_bwd): w HWIO [3,3,Cin,Cout] of the forward layer,
    wb32t = pack_weights(trans = 3) bank; results: dx (fp32 View or None) and / or dx_shadow (Shadow); mask_shadow: Shadow of the layer's input."""
    kh, kw, cin, cout = w.shape
    assert dz_shadow.C == cout and ((kh, kw) == (3, 3) or (stride == 2 and kh == kw == 5))
    B, H, W = dz_shadow.B, dz_shadow.H * stride, dz_shadow.W * stride              # size of dx (stride 2: even sizes, 'SAME' pads (k - 2) // 2 in front)
    assert stride in (1, 2) and (stride == 1 or dil == 1)
    pad = dil if stride == 1 else (kh - 2) // 2
    d = conv_desc(B, H, W, dz_shadow.H, dz_shadow.W, cin, cout, kh, kw, stride, dil, pad, pad, 0, 0, (dx.ld if dx is not None else 0), 0, mask_alpha=mask_alpha,
                  precision=1, mask_c0=mask_range[0], mask_c1=mask_range[1], accumulate=int(bool(accumulate)))     # accumulate: (old + new) * mask -- the stride-2 5x5 form only
    for t in (dx, dx_shadow, mask_shadow):
        assert t is None or (t.B, t.H, t.W, t.C) == (B, H, W, cin)
    sp = lambda sh: C.c_void_p(sh.ptr) if sh is not None else None
    lib.conv2d_planes_bwd(C.byref(d), C.c_void_p(dz_shadow.ptr), dz_shadow.ld, _p(wb32t), sp(mask_shadow), (mask_shadow.ld if mask_shadow is not None else 0),
                          _p(dx), sp(dx_shadow), (dx_shadow.ld if dx_shadow is not None else 0), _p(stream))


def plane_split(lib, pairs, device, keep, stream=None):
    """pairs: [(View src, Planes or Shadow dst)] -> hi = bf16(src), lo = bf16(src - hi) (a bare Shadow: hi only), ONE launch (mh_plane_split)."""
    if not pairs:
        return
    arr = (_ffi.PlaneSeg * len(pairs))()
    blk = 0
    for i, (src, dst) in enumerate(pairs):
        hi, lo = as_planes(dst).hi, as_planes(dst).lo
        src2 = None
        if isinstance(src, (tuple, list)):      # (View a, View b): the planes of tf.concat([a, b], -1)
            src, src2 = src
            assert (src2.B, src2.H, src2.W) == (src.B, src.H, src.W)
        assert (src.B, src.H, src.W, src.C + (src2.C if src2 is not None else 0)) == (hi.B, hi.H, hi.W, hi.C), "planes / source geometry mismatch"
        arr[i].src, arr[i].hi, arr[i].lo, arr[i].npix, arr[i].C = src.ptr, hi.ptr, (lo.ptr if lo is not None else None), src.npix, src.C
        arr[i].src_ld, arr[i].dst_ld, arr[i].blk0 = src.ld, hi.ld, blk
        if src2 is not None:
            arr[i].src2, arr[i].C2, arr[i].src2_ld = src2.ptr, src2.C, src2.ld
        blk += (src.npix * (hi.ld // 8) + 255) // 256
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    keep.append(table)
    if hasattr(lib, "note_refs"):
        flat = [v for src, _ in pairs for v in (src if isinstance(src, (tuple, list)) else (src,))]
        lib.note_refs([(v.ptr, 4 * v.npix * v.ld) for v in flat])
    lib.plane_split(C.c_void_p(table.data_ptr()), len(pairs), blk, _p(stream))


class InputTable(object):
    """The frame table of mh_fetch_inputs: page-locked host memory the device reads through its device-side address, rewritten by the host between two replays of a
    captured step (after the previous replay has completed) -- no API call, no copy launch in front of the step.  set([tensor | None, ...]): entry k = the device
    tensor the step's k-th input buffer is filled from (uint8 or float32, contiguous), None = leave the buffer as it is."""

    def __init__(self, lib, device):
        cuda = torch.device(device).type == "cuda"
        self.buf = torch.zeros(C.sizeof(_ffi.InputTable), dtype=torch.uint8, pin_memory=cuda)
        self.tab = _ffi.InputTable.from_address(self.buf.data_ptr())
        if cuda:
            dp = C.c_void_p()
            lib.host_device_pointer(C.c_void_p(self.buf.data_ptr()), C.byref(dp))
            self.ptr = dp.value
        else:
            self.ptr = self.buf.data_ptr()
        self.held = []                 # keeps the tensors of the current entries alive

    def set(self, tensors):
        assert len(tensors) <= _ffi.FETCH_MAX
        for k in range(_ffi.FETCH_MAX):
            t = tensors[k] if k < len(tensors) else None
            self.tab.src[k] = t.data_ptr() if t is not None else None
            self.tab.u8[k] = 1 if (t is not None and t.dtype == torch.uint8) else 0
        self.held = [t for t in tensors if t is not None]

    def clear(self):
        self.set([])


def fetch_inputs(lib, table_ptr, dsts, stream=None):
    """the step's first node: every destination tensor (float32, contiguous) <- the tensor the table names for it (mh_fetch_inputs)"""
    n = len(dsts)
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
    cnt = (C.c_int64 * n)(*[d.numel() for d in dsts])
    assert all(d.dtype == torch.float32 and d.is_contiguous() for d in dsts)
    lib.fetch_inputs(C.c_void_p(table_ptr), dp, cnt, n, _p(stream))


class FrameTable(object):
    """The per-sample table of mh_frame_prepare (B x mh_frame_seg), like InputTable page-locked host memory the device reads through its device-side address: the
    host fills it without an API call; it must stay as it is until the call that reads it has run.  segs[b] = the ctypes record of sample b."""

    def __init__(self, lib, device, B, pinned=True):
        """pinned=False: plain host memory -- frame_prepare then reads a device copy made on the current stream (one-off calls: nothing to keep alive)"""
        cuda = torch.device(device).type == "cuda"
        self.B, self.device = int(B), torch.device(device)
        self.buf = torch.zeros(C.sizeof(_ffi.FrameSeg) * self.B, dtype=torch.uint8, pin_memory=cuda and pinned)
        self.segs = (_ffi.FrameSeg * self.B).from_address(self.buf.data_ptr())
        if cuda and not pinned:
            self.ptr = None
        elif cuda:
            dp = C.c_void_p()
            lib.host_device_pointer(C.c_void_p(self.buf.data_ptr()), C.byref(dp))
            self.ptr = dp.value
        else:
            self.ptr = self.buf.data_ptr()

    @classmethod
    def at(cls, host_address, device_address, B):
        """a table laid over memory the caller owns: B records at host_address, which the device will see at device_address (a staging buffer the caller
        copies up in front of the call)"""
        self = cls.__new__(cls)
        self.B, self.device, self.buf = int(B), None, None
        self.segs = (_ffi.FrameSeg * self.B).from_address(host_address)
        self.ptr = device_address
        return self

    def set(self, b, left, right, gt, Hs, Ws, r0, c0, gt_kind, active=0, delta=0.0, contrast=1.0, hue=1.0):
        """left / right / gt: device addresses of sample b's uint8 [Hs,Ws,3] frames and its [Hs,Ws] ground truth (gt_kind 0 float32, 1 uint16 / 256)"""
        s = self.segs[b]
        s.left, s.right, s.gt = left, right, gt
        s.Hs, s.Ws, s.r0, s.c0, s.gt_kind, s.active = int(Hs), int(Ws), int(r0), int(c0), int(gt_kind), int(active)
        s.delta, s.contrast, s.hue = float(delta), float(contrast), float(hue)

    def any_contrast(self):
        return any(self.segs[b].active & 2 for b in range(self.B))


def frame_prepare_ws(lib, B, H, W, device):
    """the partial-sum workspace of frame_prepare (float64 sums in a float32 tensor: torch allocations are 8-byte aligned)"""
    return torch.empty(int(lib.frame_prepare_ws_floats(B, H, W)), dtype=torch.float32, device=device)


def frame_prepare(lib, table, left, right, gt, ws=None, stream=None):
    """left, right [B,H,W,3], gt [B,H,W,1] (float32, contiguous, written in every element) <- the windows the FrameTable names, cropped, augmented and cast
    (mh_frame_prepare).  ws: frame_prepare_ws(...); needed only when a sample has the contrast bit set (without it the call is one launch)."""
    B, H, W, _ = left.shape
    assert table.B == B and tuple(right.shape) == (B, H, W, 3) and tuple(gt.shape) == (B, H, W, 1)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (left, right, gt))
    if table.any_contrast():
        assert ws is not None and ws.numel() >= lib.frame_prepare_ws_floats(B, H, W), "frame_prepare: a sample has the contrast bit set: pass ws"
    else:
        ws = None
    ptr = table.ptr
    if ptr is None:
        copy = table.buf.to(table.device)          # freed in stream order behind the launch
        ptr = copy.data_ptr()
    lib.frame_prepare(C.c_void_p(ptr), B, H, W, _p(left), _p(right), _p(gt), _p(ws), _p(stream))


def camera_model(K, D, R, P):
    """mh_camera_model of one view: K 3x3 (raw camera matrix, no skew), D up to 5 distortion terms in OpenCV's order (missing ones are 0), R 3x3 rectifying
    rotation, P 3x3 or 3x4 camera matrix of the rectified view (stereoRectify's; its fourth column is not read)"""
    K, R, P = ([[float(v) for v in row] for row in m] for m in (K, R, P))
    D = [float(v) for v in (D if D is not None else [])]
    assert len(K) == 3 and len(R) == 3 and len(P) == 3 and len(D) <= 5 and all(len(row) == 3 for row in K + R) and all(len(row) in (3, 4) for row in P)
    D = D + [0.0] * (5 - len(D))
    c = _ffi.CameraModel()
    c.fx, c.fy, c.cx, c.cy = K[0][0], K[1][1], K[0][2], K[1][2]
    c.k1, c.k2, c.p1, c.p2, c.k3 = D
    for k in range(9):
        c.R[k] = R[k // 3][k % 3]
    c.fxn, c.fyn, c.cxn, c.cyn = P[0][0], P[1][1], P[0][2], P[1][2]
    return c


def rectify_map(lib, cams, map_, stream=None):
    """map_ [V,Ho,Wo,2] (float32, contiguous, written in every element) <- the raw-view position of every rectified pixel, per view from its camera_model
    (mh_rectify_map: initUndistortRectifyMap's formula in fp32)"""
    V, Ho, Wo, two = map_.shape
    assert two == 2 and len(cams) == V and map_.dtype == torch.float32 and map_.is_contiguous()
    arr = (_ffi.CameraModel * V)(*cams)
    lib.rectify_map(arr, V, Ho, Wo, _p(map_), _p(stream))


def remap(lib, src, map_, out, stream=None):
    """out [V,Ho,Wo,3] (float32, contiguous, written in every element) <- src [V,Hs,Ws,Cs] (uint8 or float32, Cs = 1, 3 or 4) sampled bilinearly at
    map_ [V,Ho,Wo,2] = (x, y), zero outside the source (mh_remap)"""
    V, Hs, Ws, Cs = src.shape
    _, Ho, Wo, _ = out.shape
    assert tuple(map_.shape) == (V, Ho, Wo, 2) and tuple(out.shape) == (V, Ho, Wo, 3)
    assert src.dtype in (torch.uint8, torch.float32) and src.is_contiguous()
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (map_, out))
    lib.remap(_p(src), 1 if src.dtype == torch.uint8 else 0, _p(map_), _p(out), V, Hs, Ws, Cs, Ho, Wo, _p(stream))


def shadow_cast(lib, pairs, device, keep, stream=None):
    """pairs: [(View src, Shadow dst)] -> every dst = bf16(src), ONE launch (mh_shadow_cast).  `keep` keeps the device table alive."""
    if not pairs:
        return
    arr = (_ffi.ShadowSeg * len(pairs))()
    blk = 0
    for i, (src, dst) in enumerate(pairs):
        assert (src.B, src.H, src.W, src.C) == (dst.B, dst.H, dst.W, dst.C), "shadow / source geometry mismatch"
        arr[i].src, arr[i].dst, arr[i].npix, arr[i].C = src.ptr, dst.ptr, src.npix, src.C
        arr[i].src_ld, arr[i].dst_ld, arr[i].blk0 = src.ld, dst.ld, blk
        blk += (src.npix * (dst.ld // 8) + 255) // 256
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    keep.append(table)
    if hasattr(lib, "note_refs"):
        lib.note_refs([(src.ptr, 4 * src.npix * src.ld) for src, _ in pairs])
    lib.shadow_cast(C.c_void_p(table.data_ptr()), len(pairs), blk, _p(stream))


import os as _os
import threading

# serialises plan recording: recordings resolve process-wide tuning hooks (filter-gradient split targets) into the plan, and DispNet's recording
# scopes one of them (RLock: a recording may nest)
TUNE_LOCK = threading.RLock()

# waves per workgroup of the streaming filter-gradient kernel (0 = the caller's choice: the engines take 4 for a batch-1 step -- the
# kernel then shares the chip with the input-gradient chain, 1.870 -> 1.818 ms per step -- and 8 for batched streams: 163 -> 138 us per batch)
WGRAD_STREAM_WAVES = 0            # 0 = the caller's choice (4 waves at batch 1, 8 for batched streams: r03 #4)
WGRAD_STREAM_WGS = 256        # workgroups a batch is divided into (one per CU)


def wgrad_stream_ok(x, dz, dw, stride, dil):
    """layers the streaming kernel covers: 3x3 'SAME', stride 1 (dilation 1 .. 16) or stride 2 (dilation 1, even sizes: padding only behind); the
    channel stride of the input's shadow is its channel count rounded up to 32, so very thin inputs (the 3-channel image) stay on the tiled kernels"""
    kh, kw = dw.shape[0], dw.shape[1]
    if not (kh == 3 and kw == 3 and x.C >= 8):
        return False
    if stride == 1:
        return 1 <= dil <= 16 and (x.H, x.W) == (dz.H, dz.W)
    return stride == 2 and dil == 1 and x.H % 2 == 0 and x.W % 2 == 0 and (x.H, x.W) == (2 * dz.H, 2 * dz.W)


def wgrad_stream(lib, qlib, wsa, segs, items, device, keep, stream=None, target_wgs=None, nwaves=None):
    """Filter + bias gradients of a batch of stride-1 3x3 layers in ONE launch from bf16 shadows (mh_wgrad_stream).
    items: [(Shadow x, Shadow dz, dw tensor (HWIO, fp32), db tensor or None, dil)].  Per-split partial sums go to the arena `wsa` and a
    segment per layer is appended to `segs` for the batch's wgrad_reduce; a layer with ONE split stores straight into dw.
    `qlib` = the real library (host-side planner); `lib` may be a Recorder."""
    if not items:
        return
    # stride-2 layers: an instance of their own; together with stride-1 layers of dilation <= 8 (a pyramid batch) the mixed kernel, ONE launch
    s2 = [it for it in items if it[0].H == 2 * it[1].H]
    mixed = bool(s2) and len(s2) != len(items)
    if mixed and max(it[4] for it in items) > 8:
        wgrad_stream(lib, qlib, wsa, segs, [it for it in items if it[0].H != 2 * it[1].H], device, keep, stream, target_wgs, nwaves)
        items, mixed = s2, False
    stride = 2 if (s2 and not mixed) else 1
    n = len(items)
    arr = (_ffi.WgsLayer * n)()
    max_dil = 1
    for i, (xs, zs, dw, db, dil) in enumerate(items):
        kh, kw, K, N = dw.shape
        st_i = 2 if xs.H == 2 * zs.H else 1
        assert kh == 3 and kw == 3 and (xs.B, xs.H, xs.W) == (zs.B, st_i * zs.H, st_i * zs.W) and xs.C == K and zs.C == N and (mixed or st_i == stride)
        L = arr[i]
        L.x, L.dz, L.db = xs.ptr, zs.ptr, (db.data_ptr() if db is not None else None)
        L.B, L.H, L.W, L.K, L.N, L.dil, L.x_ld, L.dz_ld, L.stride = zs.B, zs.H, zs.W, K, N, dil, xs.ld, zs.ld, st_i
        max_dil = max(max_dil, dil)
    nw = WGRAD_STREAM_WAVES or nwaves or 8
    if max_dil > 8:
        nw = min(nw, 7)                   # 64-pixel row slots: 7 x 20 KB of rings fit the 160 KB LDS
    if stride == 2 or mixed:
        nw, max_dil = min(nw, 5), (-3 if mixed else -2)      # 80-pixel row slots, two new rows per step: 5 x 29 KB of rings
    nblk = C.c_int32(0)
    qlib.wgrad_stream_plan(arr, n, target_wgs or WGRAD_STREAM_WGS, nw, C.byref(nblk))
    for i, (xs, zs, dw, db, dil) in enumerate(items):
        L = arr[i]
        size = dw.numel()
        if L.splits == 1 and dw.data_ptr() % 16 == 0:
            L.ws = dw.data_ptr()
        else:
            # (splits > 1, or a dw that is not 16-byte aligned)  bias partial sums behind the filter partials, summed by the same reduction launch
            nb = L.N * L.splits if (db is not None and L.splits > 1) else 0
            L.ws = wsa.alloc(size * L.splits + nb)
            segs.append((L.ws, dw.data_ptr(), size, L.splits))
            if nb:
                segs.append((L.ws + 4 * size * L.splits, db.data_ptr(), L.N, L.splits, 1))
        if hasattr(lib, "tally_wgrad"):
            lib.tally_wgrad(zs.B, zs.H, zs.W, L.K, L.N, 9, L.splits)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    keep.append(table)
    lib.wgrad_stream(C.c_void_p(table.data_ptr()), n, nblk.value, nw, max_dil, _p(stream))


def conv2d_transpose_fwd(lib, x, w, b, out, stride=2, alpha=1.0, stream=None, precision=None):
    """tf.nn.conv2d_transpose(x, w[kh,kw,Cout,Cin], 'SAME') + b, leaky (sharedLayers.py:80-92):
    the input-gradient of a SAME conv with HWIO = [kh,kw,I=Cout,O=Cin]."""
    kh, kw, cout, cin = w.shape
    Ho, Wo = x.H * stride, x.W * stride
    _, _, pt, pl = conv_geometry(Ho, Wo, kh, kw, stride, 1)
    assert (out.H, out.W, out.C) == (Ho, Wo, cout) and x.C == cin
    d = conv_desc(x.B, x.H, x.W, Ho, Wo, cin, cout, kh, kw, stride, 1, pt, pl, 1, 1, x.ld, out.ld, alpha=alpha, precision=precision)
    lib.conv2d(C.byref(d), _p(x), _p(w), _p(b), _p(out), None, _p(stream))


def corr_fwd(lib, L, R, out, max_disp, stride=1, coff=0, u=None, copy_left=False, zero_tail=False, stream=None, precision=None):
    """precision: None = the forward code of the plan being recorded (PRECISION); only the large-D MFMA kernel uses it."""
    prec = PRECISION if precision is None else precision
    if prec == 0:
        lib.corr_fwd(_p(L), L.ld, _p(R), R.ld, _p(u), _p(out), out.ld, coff, L.B, L.H, L.W, L.C, max_disp, stride,
                     int(copy_left), int(zero_tail), _p(stream))
    else:
        lib.corr_fwd_prec(_p(L), L.ld, _p(R), R.ld, _p(u), _p(out), out.ld, coff, L.B, L.H, L.W, L.C, max_disp, stride,
                          int(copy_left), int(zero_tail), prec, _p(stream))


def level_front_fwd(lib, Vc, mul, L, R, out, Rw, u, max_disp, coff, zero_tail=True, stream=None, planes=None):
    """u = mul * resize(Vc) ; Rw = warp(R, u) ; out = [L | corr(L, Rw) | u | 0]  -- one launch (mh_level_front_fwd).
    Vc: [B,H,Wc] tensor; L, R, Rw: Views [B,H,W,C]; out: View of the estimator input; u: [B,H,W] tensor.
    planes: Planes (hi + lo) or Shadow (hi only) of `out` that the launch writes too."""
    if planes is None:
        lib.level_front_fwd(_p(Vc), Vc.shape[1], Vc.shape[2], mul, _p(L), L.ld, _p(R), R.ld, _p(out), out.ld, coff, _p(Rw), Rw.ld, _p(u),
                            L.B, L.H, L.W, L.C, max_disp, int(zero_tail), _p(stream))
        return
    hi, lo = as_planes(planes).hi, as_planes(planes).lo
    assert (hi.B, hi.H, hi.W) == (L.B, L.H, L.W) and hi.C == coff + 2 * max_disp + 2 and hi.ld >= hi.C
    lib.level_front_fwd_planes(_p(Vc), Vc.shape[1], Vc.shape[2], mul, _p(L), L.ld, _p(R), R.ld, _p(out), out.ld, coff, _p(Rw), Rw.ld, _p(u),
                               L.B, L.H, L.W, L.C, max_disp, int(zero_tail), C.c_void_p(hi.ptr), (C.c_void_p(lo.ptr) if lo is not None else None), hi.ld, _p(stream))


def level_front_head_fwd(lib, X, hw, hb, Vc, mul, L, R, out, Rw, u, max_disp, coff, zero_tail=True, stream=None, planes=None):
    """level_front_fwd whose coarse disparity Vc is COMPUTED in the launch: Vc = conv3x3(X, hw) + hb, the disparity head of the coarser level (mh_level_front_head_fwd).
    X: View [B,Hc,Wc,K]; hw: the head's [3,3,K,1] weights; hb: its bias tensor or None; Vc: [B,Hc,Wc] tensor (output)."""
    hi = lo = None
    if planes is not None:
        hi, lo = as_planes(planes).hi, as_planes(planes).lo
        assert (hi.B, hi.H, hi.W) == (L.B, L.H, L.W) and hi.C == coff + 2 * max_disp + 2 and hi.ld >= hi.C
    assert (X.B, X.H, X.W) == (L.B, Vc.shape[1], Vc.shape[2]) and tuple(hw.shape) == (3, 3, X.C, 1)
    lib.level_front_head_fwd(_p(X), X.ld, X.C, _p(hw), _p(hb), _p(Vc), Vc.shape[1], Vc.shape[2], mul, _p(L), L.ld, _p(R), R.ld, _p(out), out.ld, coff, _p(Rw), Rw.ld,
                             _p(u), L.B, L.H, L.W, L.C, max_disp, int(zero_tail), (C.c_void_p(hi.ptr) if hi is not None else None),
                             (C.c_void_p(lo.ptr) if lo is not None else None), (hi.ld if hi is not None else 0), _p(stream))


def corr_bwd(lib, g, L, R, dL, dR, max_disp, stride=1, coff=0, du=None, acc_l=False, acc_r=False, acc_u=False,
             copy_left=False, stream=None, precision=None):
    """precision: None = the backward code of the plan being recorded; only the large-D MFMA kernels use it (1 = bf16 operands)."""
    prec = _bwd_precision() if precision is None else precision
    lib.corr_bwd_prec(_p(g), g.ld, coff, _p(L), L.ld, _p(R), R.ld, _p(dL), dL.ld, int(acc_l), _p(dR), dR.ld, int(acc_r),
                      _p(du), int(acc_u), L.B, L.H, L.W, L.C, max_disp, stride, int(copy_left), int(prec), _p(stream))


def corr_warp_bwd(lib, g, L, Rw, img, u, dL, dimg, du, max_disp, stride=1, coff=0, acc_l=False, copy_left=False, stream=None, acc_img=True):
    """corr_bwd(g, L, Rw -> dL, dRw, du = g[disparity channel]) + warp_bwd(dRw, img, u -> dimg scatter, du += coordinate gradient) in one
    launch; dRw is never stored.  acc_img=True: dimg holds zeros / earlier contributions and is added to; False: this launch is dimg's first writer
    (overwritten, nothing read, no zero fill needed).  dimg or du may be None."""
    lib.corr_warp_bwd(_p(g), g.ld, coff, _p(L), L.ld, _p(Rw), Rw.ld, _p(img), img.ld, _p(u), _p(dL), dL.ld, int(bool(acc_l)) | (0 if acc_img else 2),
                      _p(dimg), dimg.ld if dimg is not None else img.ld, _p(du), L.B, L.H, L.W, L.C, max_disp, stride, int(copy_left), _p(stream))


def warp_fwd(lib, img, u, out, stream=None):
    lib.warp_fwd(_p(img), img.ld, _p(u), _p(out), out.ld, img.B, img.H, img.W, img.C, _p(stream))


def warp_bwd(lib, g, img, u, dimg, du=None, acc_u=False, stream=None):
    """dimg None: coordinate gradient only; du None: scatter only."""
    lib.warp_bwd(_p(g), g.ld, _p(img), img.ld, _p(u), _p(dimg), dimg.ld if dimg is not None else img.ld, _p(du), int(acc_u),
                 img.B, img.H, img.W, img.C, _p(stream))


def resize_fwd(lib, x, out, Hr, Wr, cy=0, cx=0, mul=1.0, mode=0, stream=None):
    """x: [B,Hi,Wi] tensor; out: [B,Ho,Wo] tensor (crop of the virtual [Hr,Wr] resize at (cy,cx))."""
    B, Hi, Wi = x.shape[0], x.shape[1], x.shape[2]
    Ho, Wo = out.shape[1], out.shape[2]
    lib.resize_fwd(_p(x), _p(out), B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode, _p(stream))


def resize_bwd(lib, g, x, dx, Hr, Wr, cy=0, cx=0, mul=1.0, mode=0, accumulate=False, stream=None):
    B, Hi, Wi = x.shape[0], x.shape[1], x.shape[2]
    Ho, Wo = g.shape[1], g.shape[2]
    lib.resize_bwd(_p(g), _p(x), _p(dx), int(accumulate), B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode, _p(stream))


def conv2d_head(lib, x, w, b, out, copies=(), alpha=1.0, stream=None):
    """Forward pass of a disparity head (3x3 Cin -> 1, mh_conv2d_head): out = conv(x, w) + b, ALSO stored at up to two more Views with C = 1
    (`copies`: a channel slot of a concatenated buffer, the buffer the next stage accumulates into)."""
    kh, kw, cin, cout = w.shape
    assert cout == 1 and x.C == cin and len(copies) <= 2 and all((c.B, c.H, c.W, c.C) == (out.B, out.H, out.W, 1) for c in copies)
    Ho, Wo, pt, pl = conv_geometry(x.H, x.W, kh, kw, 1, 1)
    d = conv_desc(x.B, x.H, x.W, Ho, Wo, cin, 1, kh, kw, 1, 1, pt, pl, 0, 0, x.ld, out.ld, alpha=alpha)
    c = list(copies) + [None, None]
    lib.conv2d_head(C.byref(d), _p(x), _p(w), _p(b), _p(out), _p(c[0]), (c[0].ld if c[0] is not None else 0),
                    _p(c[1]), (c[1].ld if c[1] is not None else 0), _p(stream))


def head_bwd(lib, w, dV, dx, mask_ref=None, mask_alpha=1.0, accumulate_dx=False, du=None, Hr=0, Wr=0, mul=1.0, addends=(), dV_shadow=None,
             dx_shadow=None, stream=None):
    """Backward front end of a disparity head (mh_head_bwd): dV [B,H,W] tensor <- either the resize gradient of the finer level's coordinate
    gradient `du` ([B,Ho,Wo] tensor; Hr, Wr, mul as resize_bwd mode 0) or the sum of up to two `addends` (Views with C = 1: channel slices are
    fine); dx (View [B,H,W,N]) (+)= conv2d_backprop_input(dV, w) * leaky'(mask_ref).  With accumulate_dx the mask applies to the SUM: dx = (gradient +
    old dx) * leaky'(mask_ref), the convention of mh_conv2d (mode 1, accumulate).  w: HWIO [3,3,N,1] of the head conv.  Shadows: ops.Shadow of
    dV (C = 1) / dx, written on the way."""
    B, H, W = dV.shape
    assert tuple(w.shape) == (3, 3, dx.C, 1) and (dx.B, dx.H, dx.W) == (B, H, W)
    d = _ffi.HeadBwdDesc()
    d.B, d.H, d.W, d.N = B, H, W, dx.C
    d.dx_ld, d.mask_ld, d.accumulate_dx, d.mask_alpha = dx.ld, (mask_ref.ld if mask_ref is not None else 0), int(accumulate_dx), mask_alpha
    if du is not None:
        d.kind, d.Hr, d.Wr, d.cy, d.cx, d.Ho, d.Wo, d.mul = 0, Hr, Wr, 0, 0, du.shape[1], du.shape[2], mul
        src0, src1 = _p(du), None
    else:
        assert 1 <= len(addends) <= 2 and all((a.B, a.H, a.W, a.C) == (B, H, W, 1) for a in addends)
        d.kind = 1
        d.src0_ld = addends[0].ld
        d.src1_ld = addends[1].ld if len(addends) > 1 else 0
        src0, src1 = _p(addends[0]), (_p(addends[1]) if len(addends) > 1 else None)
    for sh, c in ((dV_shadow, 1), (dx_shadow, dx.C)):
        assert sh is None or (sh.B, sh.H, sh.W, sh.C) == (B, H, W, c)
    lib.head_bwd(C.byref(d), src0, src1, _p(dV), (C.c_void_p(dV_shadow.ptr) if dV_shadow is not None else None), _p(w), _p(dx), _p(mask_ref),
                 (C.c_void_p(dx_shadow.ptr) if dx_shadow is not None else None), _p(stream))


def resize_image(lib, x, out, stream=None):
    """TF1-legacy bilinear resize of an NHWC image tensor [B,H,W,C] into out [B,Ho,Wo,C] (scale_tensor on the frames)."""
    B, H, W, Cc = x.shape
    lib.resize_image_fwd(_p(x), _p(out), B, H, W, Cc, out.shape[1], out.shape[2], _p(stream))


def conv_image_fwd(lib, frames, Hp, Wp, reflect_t, reflect_l, w, bias, out, stride=2, alpha=1.0, div=1.0, sub=0.0, shadow=None, stream=None):
    """out = leaky(conv3x3(reflect_pad(frames / div - sub), w) + bias) from the frames themselves (mh_conv_image_fwd): frames [NB,H0,W0,3] tensor, out a View
    [NB,ceil(Hp/stride),ceil(Wp/stride),16]; shadow: the Shadow of `out` the launch writes too."""
    NB, H0, W0, Cc = frames.shape
    kh, kw, cin, cout = w.shape
    assert (kh, kw, cin) == (3, 3, Cc) and cout == out.C
    Ho, Wo, pt, pl = conv_geometry(Hp, Wp, 3, 3, stride, 1)
    assert (out.B, out.H, out.W) == (NB, Ho, Wo)
    lib.conv_image_fwd(_p(frames), NB, H0, W0, Cc, Hp, Wp, reflect_t, reflect_l, div, sub, _p(w), _p(bias), cout, stride, pt, pl, alpha, _p(out), out.ld,
                       (C.c_void_p(shadow.ptr) if shadow is not None else None), (shadow.ld if shadow is not None else 0), _p(stream))


def pad_reflect(lib, x, out, pad_t, pad_l, div=1.0, sub=0.0, stream=None):
    """out = reflect_pad(x / div - sub).  x: [B,H,W,C] tensor; out: [B,Hp,Wp,out_ld] tensor."""
    B, H, W, Cc = x.shape
    lib.pad_reflect(_p(x), _p(out), B, H, W, Cc, out.shape[1], out.shape[2], pad_t, pad_l, out.shape[3], div, sub, _p(stream))


def bias_grad_partial(lib, qlib, wsa, segs, dz, db, stream=None):
    """db += column sums of dz without float atomics: per-workgroup partial sums into the arena + one more segment for the batch's wgrad_reduce
    (fixed summation order -- replays of a step are bit-identical).  `qlib` = the real library (grid query); `lib` may be a Recorder."""
    nb = qlib.bias_grad_blocks(dz.npix, dz.C)
    ws = wsa.alloc(nb * dz.C)
    lib.bias_grad_partial(_p(dz), dz.ld, dz.npix, dz.C, C.c_void_p(ws), nb, _p(stream))
    segs.append((ws, db.data_ptr(), dz.C, nb, 1))


def bias_grad(lib, dz, db, stream=None):
    """db += column sums of the View dz."""
    lib.bias_grad(_p(dz), dz.ld, dz.npix, dz.C, _p(db), _p(stream))


def smoothness_ws(lib, B, H, W, device):
    """the workspace of smoothness_loss: one float per tile (mh_smoothness_ws_floats), nothing to initialise"""
    return torch.empty(int(lib.smoothness_ws_floats(B, H, W)), dtype=torch.float32, device=device)


def smoothness_loss(lib, disp, image, ws, result, ddisp=None, weight=1.0, grad_scale=1.0, accumulate=False, stream=None, phase=0):
    """the reference's edge-aware smoothness(x, y) (Losses/loss_factory.py:183-220; mh_smoothness_loss): disp [B,H,W], image [B,H,W,C] (C = 3 or 1) in 0..255.
    result [4]: result[3] = weight * S, result[0] = (accumulate: +=) weight * S; ddisp (optional) = (accumulate: +=) grad_scale * weight * dS/ddisp.  Launched
    directly, never recorded: in a plan the term rides on the LOSS record (reprojection_loss(..., smoothness=))."""
    B, H, W = disp.shape[0], disp.shape[1], disp.shape[2]
    Cc = image.shape[3] if image.dim() == 4 else 1
    lib.smoothness_loss(_p(disp), _p(image), _p(ws), _p(result), _p(ddisp), float(weight), grad_scale, int(bool(accumulate)), B, H, W, Cc, phase, _p(stream))


def loss_set_valid(lib, ws, valid_l, valid_r):
    """copy the validity masks (uint8 [B,H,W], non-zero = valid) of a masked LOSS record into its workspace `ws`: the left mask at float offset
    mh_loss_valid_offset, the right one at the next 16-byte boundary (include/madnet_hip.h).  A torch copy on the current stream; the bytes may be rewritten
    between two replays of a captured plan."""
    B, H, W = valid_l.shape
    if valid_r.shape != valid_l.shape or valid_l.dtype != torch.uint8 or valid_r.dtype != torch.uint8:
        raise ValueError("validity masks: two uint8 tensors of one shape [B,H,W]")
    n = B * H * W
    if ws.numel() < int(lib.loss_ws_floats(B, H, W)):
        raise ValueError("validity masks: the workspace is smaller than mh_loss_ws_floats(%d, %d, %d)" % (B, H, W))
    raw = ws.view(torch.uint8)
    o = 4 * int(lib.loss_valid_offset(B, H, W))
    raw[o:o + n].copy_(valid_l.reshape(-1))
    o += (n + 15) // 16 * 16
    raw[o:o + n].copy_(valid_r.reshape(-1))


def reprojection_loss(lib, left, right, disp, ws, result, ddisp=None, grad_scale=1.0, stream=None, phase=0, smoothness=0.0, valid=None):
    """phase 0 = everything; 1 = warp + SSIM maps + gradient (what the backward pass waits for); 2 = the reduction of the loss value.
    valid: (valid_l, valid_r), uint8 [B,H,W]: the loss over the valid pixels (mh_reprojection_loss_masked).  Recorded: the flag in the LOSS record's `phase` slot
    (the recorder's state attribute `loss_masked`, put back afterwards) -- the replay reads the masks from ws (loss_set_valid), not from these tensors.
    smoothness: weight w of the edge-aware smoothness term of (disp, left): result[0] += w * S, result[3] = w * S (result then has 4 floats), ddisp += its
    gradient, each in the phase that writes the reprojection loss's share.  Recorded: the weight in the LOSS record's `smooth_weight` slot (the recorder's state
    attribute, put back afterwards); launched: the second call made here, its partial sums in the first floats of ws.  0: nothing more is launched or recorded."""
    B, H, W = disp.shape[0], disp.shape[1], disp.shape[2]
    smoothness = float(smoothness)
    recording = hasattr(lib, "note_refs")          # a plan.Recorder
    if recording:
        before, lib.smoothness = lib.smoothness, smoothness
        masked_before, lib.loss_masked = lib.loss_masked, valid is not None
    try:
        if valid is not None and not recording:
            lib.reprojection_loss_masked(_p(left), _p(right), _p(disp), _p(valid[0]), _p(valid[1]), _p(ws), _p(result), _p(ddisp), grad_scale, B, H, W, phase, _p(stream))
        elif phase == 0:
            lib.reprojection_loss(_p(left), _p(right), _p(disp), _p(ws), _p(result), _p(ddisp), grad_scale, B, H, W, _p(stream))
        else:
            lib.reprojection_loss_phase(_p(left), _p(right), _p(disp), _p(ws), _p(result), _p(ddisp), grad_scale, B, H, W, phase, _p(stream))
    finally:
        if recording:
            lib.smoothness = before
            lib.loss_masked = masked_before
    if smoothness != 0.0 and not recording:
        lib.smoothness_loss(_p(disp), _p(left), _p(ws), _p(result), _p(ddisp), smoothness, grad_scale, 1, B, H, W, 3, phase, _p(stream))


def _loss_id(loss):
    """a name of _ffi.LABEL_LOSS or its number -> the number (MH_LOSS_*)"""
    if isinstance(loss, str):
        if loss not in _ffi.LABEL_LOSS:
            raise ValueError("unknown label loss %r, pick one among: %s" % (loss, ", ".join(_ffi.LABEL_LOSS)))
        return _ffi.LABEL_LOSS[loss]
    return int(loss)


def _record_with_loss(rec, loss, method, *args):
    """record a PROXY_LOSS / PROXY_LOSS_SCALED op with `loss` in its slot (the recorder's state attribute, put back afterwards)"""
    before, rec.label_loss = rec.label_loss, loss
    try:
        method(*args)
    finally:
        rec.label_loss = before


def label_loss(lib, pred, label, ws, result, loss, rule, hi, dpred=None, weight=1.0, grad_scale=1.0, stream=None):
    """result[0] = weight * loss(pred, label, valid) for one of the six names of _ffi.LABEL_LOSS (the reference's scalar (x, y, mask) losses, mh_label_loss);
    rule 0: valid = !(label <= 0 | label >= hi) (get_proxy_loss), rule 1: valid = !(label == 0 | label >= hi) (get_supervised_loss); result[1] = sum(valid);
    dpred = its gradient (optional).  Workspace as proxy_loss.  Launched directly, never recorded (a plan carries the proxy rule: proxy_loss(..., loss=))."""
    B, H, W = pred.shape[0], pred.shape[1], pred.shape[2]
    lib.label_loss(_p(pred), _p(label), _p(ws), _p(result), _p(dpred), _loss_id(loss), int(rule), float(hi), weight, grad_scale, B, H, W, _p(stream))


def proxy_loss(lib, pred, proxy, ws, result, dpred=None, weight=0.01, grad_scale=1.0, stream=None, loss=0):
    """result[0] = weight * mean_l1(pred, proxy, valid) (loss_factory.get_proxy_loss); dpred = its gradient (optional).  loss: another name (or number) of
    _ffi.LABEL_LOSS under the same validity rule -- the same op kind with the number in its `loss` slot when recorded, mh_label_loss when launched."""
    B, H, W = pred.shape[0], pred.shape[1], pred.shape[2]
    loss = _loss_id(loss)
    args = (_p(pred), _p(proxy), _p(ws), _p(result), _p(dpred), weight, grad_scale, B, H, W, _p(stream))
    if loss == 0:
        lib.proxy_loss(*args)
    elif hasattr(lib, "note_refs"):          # a plan.Recorder
        _record_with_loss(lib, loss, lib.proxy_loss, *args)
    else:
        lib.label_loss(*(args[:5] + (loss, 0, 192.0) + args[5:]))


def sgm_proxy_ws(lib, B, H, W, D, device, paths=4, median=False, scale=1):
    """the workspace of sgm_proxy (census words, `paths` path volumes, the right view's winners, with the median the unfiltered labels; at scale 2 the half grays in
    front and the half-resolution labels behind those of the half frame): torch allocations are at least 16-byte aligned.  D is the full-resolution range."""
    return torch.empty(int(lib.sgm_ws_bytes_scaled(B, H, W, D, int(paths), int(bool(median)), int(scale))), dtype=torch.uint8, device=device)


def sgm_proxy(lib, left, right, ws, out, max_disp=128, p1=10, p2=120, uniq=95, lr_tol=1, stream=None, paths=4, median=False, scale=1):
    """left, right [B,H,W,3] uint8 or float32 (0..255) -> out [B,H,W] float32 proxy disparities, 0 = rejected (mh_sgm_proxy_scaled).  paths: 4 (rows and columns) or
    8 (the diagonals as well); median: a 3x3 median of the valid labels; scale: 1, or 2 = match the half-size gray frames over max_disp / 2 disparities and write
    every label, doubled, to its 2 x 2 pixels (max_disp stays the full-resolution range: 128, 256 or 384).  Called directly, never recorded."""
    B, H, W, c = left.shape
    assert c == 3 and right.shape == left.shape and right.dtype == left.dtype and left.dtype in (torch.uint8, torch.float32), "sgm_proxy: [B,H,W,3] uint8 or float32"
    assert left.is_contiguous() and right.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == B * H * W
    paths, median, scale = int(paths), int(bool(median)), int(scale)
    assert ws.numel() * ws.element_size() >= lib.sgm_ws_bytes_scaled(B, H, W, int(max_disp), paths, median, scale), "sgm_proxy: workspace too small"
    lib.sgm_proxy_scaled(_p(left), _p(right), int(left.dtype == torch.uint8), _p(ws), _p(out), B, H, W, int(max_disp), int(p1), int(p2), int(uniq), int(lr_tol),
                         paths, median, scale, _p(stream))
    return out


def sgm_speckle_ws(lib, B, H, W, device):
    """the workspace of sgm_speckle (a parent and a count word per pixel); torch allocations are at least 16-byte aligned"""
    return torch.empty(int(lib.sgm_speckle_ws_bytes(B, H, W)), dtype=torch.uint8, device=device)


def sgm_speckle(lib, labels, out, ws, max_size, max_diff=1.0, stream=None):
    """labels [B,H,W] float32 -> out: the labels of the 4-connected components (valid = label > 0, neighbours within max_diff) that hold more than max_size
    pixels, 0 elsewhere (mh_sgm_speckle).  out may be labels.  Called directly, never recorded."""
    assert labels.dim() == 3 and labels.dtype == torch.float32 and labels.is_contiguous(), "sgm_speckle: [B,H,W] float32"
    B, H, W = labels.shape
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == B * H * W and out.device == labels.device
    assert ws.numel() * ws.element_size() >= lib.sgm_speckle_ws_bytes(B, H, W), "sgm_speckle: workspace too small"
    lib.sgm_speckle(_p(labels), _p(out), _p(ws), B, H, W, int(max_size), float(max_diff), _p(stream))
    return out


CMAPS = {"gray": 0, "jet": 1}          # the colour maps of mh_colorize, by matplotlib's names


def colorize_ws(lib, B, H, W, device):
    """the workspace of colorize (partial ranges, partial image maxima, the codes of image 0); torch allocations are at least 16-byte aligned"""
    return torch.empty(int(lib.colorize_ws_bytes(B, H, W)), dtype=torch.uint8, device=device)


def colorize(lib, value, out, ws, cmap, out_kind, vmin=None, vmax=None, stream=None):
    """value [B,H,W] float32 through a colour map (mh_colorize): cmap 0 / 'gray' or 1 / 'jet'; out_kind 0: out = float32 [B,H,W,3], the reference's colorize_img;
    out_kind 1: out = uint8 [H,W,3], image 0 as TF's image summary writes it.  vmin / vmax: both None = the range of the finite elements of the whole tensor,
    otherwise both given.  Called directly, never recorded."""
    assert value.dim() == 3 and value.dtype == torch.float32 and value.is_contiguous(), "colorize: [B,H,W] float32"
    assert (vmin is None) == (vmax is None), "colorize: give both vmin and vmax or neither"
    B, H, W = value.shape
    cmap = CMAPS.get(cmap, cmap)
    want = (torch.float32, B * H * W * 3) if int(out_kind) == 0 else (torch.uint8, H * W * 3)
    assert out.is_contiguous() and out.device == value.device and (int(out_kind) not in (0, 1) or (out.dtype, out.numel()) == want), "colorize: wrong output tensor"
    assert ws.numel() * ws.element_size() >= lib.colorize_ws_bytes(B, H, W), "colorize: workspace too small"
    use = vmin is not None
    lib.colorize(_p(value), _p(out), _p(ws), B, H, W, int(cmap), int(out_kind), int(use), float(vmin) if use else 0.0, float(vmax) if use else 0.0, _p(stream))
    return out


def proxy_loss_scaled(lib, pred, proxy, ws, result, scale, dpred=None, weight=0.1, grad_scale=1.0, stream=None, loss=0):
    """proxy_loss of the prediction and the proxy labels both resized to (H // scale, W // scale), the labels divided by scale (a MAD block's loss under
    --reprojectionScale, Stereo_Continual_Adaptation.py:95-112) in one op; dpred = its gradient on the full-size grid (optional).  ws: proxy_scaled_ws_floats.
    loss: as for proxy_loss (mh_label_loss_scaled)."""
    B, H, W = pred.shape[0], pred.shape[1], pred.shape[2]
    loss = _loss_id(loss)
    args = (_p(pred), _p(proxy), _p(ws), _p(result), _p(dpred), weight, grad_scale, int(scale), B, H, W, _p(stream))
    if loss == 0:
        lib.proxy_loss_scaled(*args)
    elif hasattr(lib, "note_refs"):          # a plan.Recorder
        _record_with_loss(lib, loss, lib.proxy_loss_scaled, *args)
    else:
        lib.label_loss_scaled(*(args[:5] + (loss,) + args[5:]))


def supervised_loss(lib, pred, target, ws, result, dpred=None, weight=1.0, grad_scale=1.0, max_disp=192.0, stream=None):
    """result[0] = weight * mean_l1(pred, target, valid = !(target == 0 | target >= max_disp)) -- one scale of
    loss_factory.get_supervised_loss (Train.py:100); dpred = its gradient (optional).  Workspace as proxy_loss."""
    B, H, W = pred.shape[0], pred.shape[1], pred.shape[2]
    lib.supervised_loss(_p(pred), _p(target), _p(ws), _p(result), _p(dpred), weight, grad_scale, max_disp, B, H, W, _p(stream))


def adam(lib, var, m, v, grad, state, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, n=None, stream=None):
    """tf.train.AdamOptimizer apply; state = device float[2] {beta1_power, beta2_power} (see adam_advance)."""
    lib.adam(_p(var), _p(m), _p(v), _p(grad), n if n is not None else var.numel(), _p(state), lr, beta1, beta2, eps, grad_scale, _p(stream))


def adam_advance(lib, state, beta1=0.9, beta2=0.999, stream=None):
    lib.adam_advance(_p(state), beta1, beta2, _p(stream))


def metrics(lib, disp, gt, ws, result, pixel_th=3.0, stream=None):
    B, H, W = disp.shape[0], disp.shape[1], disp.shape[2]
    lib.metrics(_p(disp), _p(gt), _p(ws), _p(result), pixel_th, B, H, W, _p(stream))


def metrics_kitti(lib, disp, gt, ws, result, stream=None):
    """result = [EPE over gt > 0, KITTI D1-all in percent, #valid] (Stereo_Continual_Adaptation.py:245-249)"""
    B, H, W = disp.shape[0], disp.shape[1], disp.shape[2]
    lib.metrics_kitti(_p(disp), _p(gt), _p(ws), _p(result), B, H, W, _p(stream))


def momentum(lib, var, accum, grad, lr, mom=0.9, grad_scale=1.0, n=None, stream=None):
    lib.momentum(_p(var), _p(accum), _p(grad), n if n is not None else var.numel(), lr, mom, grad_scale, _p(stream))


def fill(lib, t, off, count, stream=None):
    """zero fill of t.flatten()[off:off + count]"""
    lib.fill(C.c_void_p(t.reshape(-1).data_ptr() + 4 * off), count, 0.0, _p(stream))


def copy_channels(lib, src, dst, nch=None, scale=1.0, accumulate=False, stream=None):
    lib.copy_channels(_p(src), src.ld, _p(dst), dst.ld, src.npix, nch if nch is not None else src.C, scale,
                      int(accumulate), _p(stream))


def leaky_bwd(lib, dy, y, alpha, stream=None):
    lib.leaky_bwd(_p(dy), dy.ld, _p(y), y.ld, dy.npix, dy.C, alpha, _p(stream))


def stamp(lib, slots, index, stream=None):
    """slots[index] (int64 device tensor) = the device wall clock when this op runs (mh_stamp)"""
    assert slots.dtype == torch.int64
    lib.stamp(C.c_void_p(slots.data_ptr() + 8 * index), _p(stream))
