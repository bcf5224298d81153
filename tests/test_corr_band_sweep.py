"""Seeded sweeps of the large-shift correlation kernels (csrc/corr.hip: the banded GEMM behind DispNet's 81-shift cost volume): corr_fwd_mfma<C/16>,
corr_fwd_mfma_bf16<C/32, bf16 | bf16x3>, corr_bwd_mfma<C/16>, corr_bwd_mfma_bf16_pair / _one<C/16> and the kernels the dispatcher falls back to.  One FIXED
list of shapes (the edges first, then a fill drawn once from a literal seed; a failure message carries the shape), operands as views into wider rows whose
padding holds NaN, every output in a guarded buffer prefilled with NaN (tests/footprint.py), the kernel the dispatcher chose asserted at every launch against
a test-side copy of its conditions, references in float64 that repeat the ARITHMETIC of the kernel that ran, so that only the summation order is left:
  exact fp32          the oracle (autograd for the gradients) on the unrounded operands, FWD = 2e-5 / GRAD = 5e-5 of tests/test_shape_sweep.py
  bf16                the oracle on bf16-rounded operands (products of bf16 values are exact in fp32), 2e-6 * max(1, |ref|max)
  split-bf16          corr(hiL, hiR) + corr(hiL, loR) + corr(loL, hiR) with hi = bf16(x), lo = bf16(x - hi): the three MFMA terms, same 2e-6 bound"""
import random

import pytest
import torch

import footprint as FP
from madnet_hip import ops
from oracle import tf_ops as T

SEED = 20240923
FWD, GRAD, BF = 2e-5, 5e-5, 2e-6
LDS = 150 * 1024
MDS = [5, 7, 8, 9, 15, 16, 17, 24, 32, 33, 40, 41]
MFMA_C = (16, 32, 64, 128, 256)


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the dispatcher's conditions (mh_corr_fwd_prec / mh_corr_bwd_prec, stride 1, no concat form, D > 9), restated ------------------------------------
def _fwd_dispatch(Cc, md, prec):
    """the prefix of mh_last_kernel's note after mh_corr_fwd_prec"""
    rows = 48 + 16 * ((2 * md + 31) // 16)
    if Cc in MFMA_C and rows * (Cc + 4) * 4 <= LDS:
        if prec != 0 and 32 <= Cc <= 256 and rows * (Cc + 16) * 2 * (2 if prec == 2 else 1) <= LDS:
            return "corr_fwd_mfma_bf16<C/32=%d,%s>" % (Cc // 32, "bf16x3" if prec == 2 else "bf16")
        return "corr_fwd_mfma<C/16=%d>" % (Cc // 16)
    return "corr_fwd_large<TW=32>"


def _bwd_dispatch(Cc, md, prec, pair=True):
    """the prefix of mh_last_kernel's note after mh_corr_bwd_prec"""
    D = 2 * md + 1
    if prec == 1 and Cc in (32, 64, 128, 256):
        rows = 48 + 32 * ((2 * md + 47) // 32)
        dph = (((D + 3) & ~3) + 7) & ~7
        if max(64 * (Cc + 4) * 4, (rows * (Cc + 16) + rows * dph) * 2) <= LDS:
            return "corr_bwd_mfma_bf16_%s<C/16=%d>" % ("pair" if pair else "one", Cc // 16)
    rows = 48 + 16 * ((2 * md + 31) // 16)
    if Cc in MFMA_C and (rows * (Cc + 4) + rows * ((D + 3) & ~3)) * 4 <= LDS:
        return "corr_bwd_mfma<C/16=%d>" % (Cc // 16)
    return "corr_bwd_kernel"


# ---- shapes (B, H, W, C, max_disp) --------------------------------------------------------------------------------------------------------------------
def _shapes():
    out = [
        (1, 1, 1, 32, 5), (1, 2, 2, 64, 7), (1, 3, 15, 128, 8), (2, 2, 16, 256, 9), (1, 5, 17, 16, 15), (2, 3, 63, 32, 16),      # 1 .. 6 workgroups
        (3, 5, 5, 64, 17),                           # W < max_disp, 15 workgroups
        (1, 1, 64, 128, 24), (1, 2, 65, 32, 32), (1, 1, 127, 64, 33), (1, 1, 128, 32, 40), (1, 1, 129, 128, 40), (1, 1, 130, 64, 41),
        (2, 4, 20, 32, 41), (3, 3, 30, 64, 40), (1, 5, 70, 32, 9),                                                         # 8, 9, 10 workgroups
        (1, 1, 200, 256, 24),                        # the last max_disp of the list at which the fp32 gradient pair holds C = 256 in LDS
        (1, 1, 17, 256, 32), (1, 2, 16, 256, 33),    # split-bf16 forward at C = 256: the last max_disp in LDS, the first that runs as fp32
        (1, 1, 33, 256, 40), (1, 1, 18, 256, 41),    # C = 256: the last max_disp of the MFMA forward kernels, the first of corr_fwd_large
        (1, 2, 21, 48, 16),                          # a channel count without an MFMA instance
        (1, 1, 65, 16, 40), (1, 2, 9, 16, 41), (2, 1, 100, 128, 41),
    ]
    r = random.Random("%d/corr_band" % SEED)
    while len(out) < 40:
        B, H, W = r.randint(1, 3), r.randint(1, 5), r.randint(1, 200)
        Cc, md = r.choice([16, 32, 32, 64, 64, 128, 128, 256]), r.choice(MDS)
        if B * H * W > 400 or (Cc == 256 and md >= 32):
            continue
        out.append((B, H, W, Cc, md))
    return out


SHAPES = _shapes()


def _nwg(shp):
    return shp[0] * shp[1] * ((shp[2] + 63) // 64)


def test_corr_band_shape_list():
    """the list holds what the sweep is there for: every channel count, shift count and width edge, every workgroup count mod 8, both sides of the LDS limits"""
    assert {s[3] for s in SHAPES} == set(MFMA_C) | {48} and {s[4] for s in SHAPES} == set(MDS)
    assert {1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129} <= {s[2] for s in SHAPES} and any(s[2] < s[4] for s in SHAPES)
    assert {_nwg(s) % 8 for s in SHAPES} == set(range(8)) and {1, 2, 3, 4, 5, 6} <= {_nwg(s) for s in SHAPES}
    assert all(s[0] * s[1] * s[2] <= 400 for s in SHAPES)
    assert sum(1 for s in SHAPES if s[3] == 256 and s[4] >= 32) == 4          # the four sides of the two forward LDS limits, one segment each
    assert _fwd_dispatch(256, 32, 2) == "corr_fwd_mfma_bf16<C/32=8,bf16x3>" and _fwd_dispatch(256, 33, 2) == "corr_fwd_mfma<C/16=16>"
    for prec in (0, 1, 2):
        assert "mfma" in _fwd_dispatch(256, 40, prec) and _fwd_dispatch(256, 41, prec) == "corr_fwd_large<TW=32>"
    assert _bwd_dispatch(256, 24, 0) == "corr_bwd_mfma<C/16=16>" and _bwd_dispatch(256, 32, 0) == "corr_bwd_kernel" and _bwd_dispatch(256, 40, 0) == "corr_bwd_kernel"
    assert _bwd_dispatch(128, 41, 0) == "corr_bwd_mfma<C/16=8>" and _bwd_dispatch(256, 41, 1) == "corr_bwd_mfma_bf16_pair<C/16=16>"


def _split(x):
    """hi = bf16(x), lo = bf16(x - hi) (mh_split_bf16x2; the subtraction is exact in fp32)"""
    hi = FP.bf16_round(x)
    return hi, FP.bf16_round(x - hi)


class _Case(object):
    """operands, layouts and float64 references of shape k -- built once, shared by the tests and the two backends, never modified"""

    def __init__(self, k, shp):
        self.k, self.shp = k, shp
        B, H, W, Cc, md = shp
        self.D = D = 2 * md + 1
        self.what = "shape %d %s D=%d" % (k, shp, D)
        self.L, self.R = _rand((B, H, W, Cc), 1000 + k), _rand((B, H, W, Cc), 2000 + k)
        self.g = _rand((B, H, W, D), 3000 + k)
        self.oldl, self.oldr = _rand((B, H, W, Cc), 4000 + k), _rand((B, H, W, Cc), 5000 + k)
        # layouts, rotated over the shapes
        self.l_ld, self.r_ld = Cc + (0, 4, 8)[k % 3], Cc + (0, 4, 8)[(k + 1) % 3]
        self.coff, self.extra = (0, 3, 4)[k % 3], (2, 1, 5)[(k // 3) % 3]
        self.gcoff = (0, 3, 4)[(k + k // 3) % 3]              # 3: the scalar staging of g; 0 / 4 with rows of a multiple of 4 floats: the 16-byte staging
        self.g_ld = self.gcoff + D + 2 if self.gcoff == 3 else FP.round_up(self.gcoff + D + 1, 4)
        self.acc_l, self.acc_r = (k >> 1) & 1, (k >> 2) & 1
        self.dl_ld, self.dr_ld = Cc + 8 * (k & 1), Cc + 8 * (((k >> 3) + k) & 1)
        self._fwd = self._bwd = None

    def fwd_ref(self, kernel):
        """the float64 volume in the arithmetic of `kernel`; [0] is the oracle on the unrounded operands"""
        if self._fwd is None:
            md = self.shp[4]
            L, R = self.L, self.R
            (hl, ll), (hr, lr) = _split(L), _split(R)
            c = lambda a, b: T.correlation(a.double(), b.double(), md, 1)
            self._fwd = (c(L, R), c(hl, hr), c(hl, hr) + c(hl, lr) + c(ll, hr))
        return self._fwd[2 if "bf16x3" in kernel else (1 if "bf16" in kernel else 0)]

    def bwd_ref(self, kernel):
        """(dL, dR) in float64 without the accumulated old values, in the arithmetic of `kernel`"""
        if self._bwd is None:
            md = self.shp[4]
            refs = []
            for rnd in (lambda t: t, FP.bf16_round):
                Lc, Rc = rnd(self.L).double().requires_grad_(True), rnd(self.R).double().requires_grad_(True)
                refs.append(torch.autograd.grad(T.correlation(Lc, Rc, md, 1), [Lc, Rc], rnd(self.g).double()))
            self._bwd = refs
        return self._bwd[1 if "bf16" in kernel else 0]


_cases = {}


def _case(k):
    if k not in _cases:
        _cases[k] = _Case(k, SHAPES[k])
    return _cases[k]


class _Worst(object):
    """worst absolute error per kernel instance"""

    def __init__(self, op):
        self.op, self.w = op, {}

    def check(self, what, kernel, part, got, ref):
        got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
        e = (got - ref).abs().max().item()
        sc = max(1.0, ref.abs().max().item())
        if "bf16" in kernel:
            bound = BF * sc
        else:
            bound = 2e-6 + (FWD if part == "fwd" else GRAD) * sc
        key = kernel + ("" if part == "fwd" else " " + part)
        self.w[key] = max(self.w.get(key, 0.0), e)
        assert e <= bound, "%s %s: %s %s error %.3g > %.3g" % (self.op, what, kernel, part, e, bound)

    def report(self, backend, n):
        print("%s (%s, %d shapes): worst abs error %s" % (self.op, backend.name, n, ", ".join("%s %.3g" % kv for kv in sorted(self.w.items()))))
        fam = {}
        for key, e in self.w.items():
            fam[_family(key)] = max(fam.get(_family(key), 0.0), e)
        print("%s (%s), over the instances of a kernel: %s" % (self.op, backend.name, ", ".join("%s %.3g" % kv for kv in sorted(fam.items()))))


def _family(key):
    """'corr_fwd_mfma_bf16<C/32=2,bf16x3>' -> 'corr_fwd_mfma_bf16[bf16x3]', 'corr_bwd_mfma<C/16=4> dL' -> 'corr_bwd_mfma dL'"""
    head, _, tail = key.partition("<")
    if not tail:
        return key
    inside, _, rest = tail.partition(">")
    return head + ("[bf16x3]" if "bf16x3" in inside else "") + rest


def _note(lib):
    return lib.last_kernel().decode()


# ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
def _run_fwd(backend, c, prec):
    """-> (the volume as a CPU tensor, the payload's bits, the note); the footprint is asserted here"""
    lib, dev = backend.lib, backend.device
    B, H, W, Cc, md = c.shp
    Lv = ops.View(FP.wide_rows(c.L, c.l_ld, dev), B, H, W, Cc, c.l_ld)
    Rv = ops.View(FP.wide_rows(c.R, c.r_ld, dev), B, H, W, Cc, c.r_ld)
    go, ov = FP.slice_view(dev, B, H, W, c.D, c.coff, c.extra)
    before = go.snapshot()
    ops.corr_fwd(lib, Lv, Rv, ov, md, 1, precision=prec)
    note = _note(lib)
    backend.sync()
    FP.assert_only_slice_written(go, ov, c.coff, before, "%s precision %d (%s)" % (c.what, prec, note))
    return FP.slice_of(go, ov, c.coff), go.payload_bits().clone(), note


def test_corr_band_fwd_sweep(backend):
    """mh_corr_fwd / mh_corr_fwd_prec at precisions 0, 1, 2: C in {16 .. 256} (48: no MFMA instance), max_disp on the edges of the block counts, W from 1 to
    200 (W < max_disp included), L / R rows of C, C + 4, C + 8 floats with NaN padding, the volume into a channel slice at offset 0 / 3 / 4; the dispatched
    kernel asserted (both LDS limits of C = 256 crossed), the result judged in the arithmetic that ran; every eighth shape launched twice (same bits)"""
    W_ = _Worst("mh_corr_fwd_prec")
    seen = set()
    for k in range(len(SHAPES)):
        c = _case(k)
        B, H, W, Cc, md = c.shp
        ref0 = c.fwd_ref("")
        outs = {}
        for prec in (0, 1, 2):
            what = "%s precision %d" % (c.what, prec)
            got, b0, note = _run_fwd(backend, c, prec)
            expect = _fwd_dispatch(Cc, md, prec)
            assert note.startswith(expect), "%s: ran %s, the dispatch conditions say %s" % (what, note, expect)
            seen.add(expect)
            W_.check(what, expect, "fwd", got, c.fwd_ref(expect))
            outs[prec] = (got, expect)
            if k % 8 == 0:
                _, b1, _ = _run_fwd(backend, c, prec)
                assert torch.equal(b0, b1), "%s: two launches of %s differ" % (what, expect)
        if "bf16>" in outs[1][1] and "bf16x3>" in outs[2][1]:
            e1 = (outs[1][0].double() - ref0).abs().max().item()
            e2 = (outs[2][0].double() - ref0).abs().max().item()
            print("%s: against the unrounded oracle bf16 %.3g, split-bf16 %.3g" % (c.what, e1, e2))
            assert e2 * 30 <= e1, "%s: split-bf16 %.3g is not 30x closer to the unrounded oracle than bf16 %.3g" % (c.what, e2, e1)
    W_.report(backend, len(SHAPES))
    need = ["corr_fwd_mfma<C/16=%d>" % n for n in (1, 2, 4, 8, 16)] + ["corr_fwd_mfma_bf16<C/32=%d,%s>" % (n, x) for n in (1, 2, 4, 8) for x in ("bf16", "bf16x3")]
    missing = [n for n in need + ["corr_fwd_large<TW=32>"] if n not in seen]
    assert not missing, "kernel instances the sweep never launched: %s (seen %s)" % (missing, sorted(seen))


# ---- gradient -----------------------------------------------------------------------------------------------------------------------------------------
def _grad_out(dev, c, ld, old):
    """a guarded gradient buffer in rows of ld floats: (Guarded, View of the C channels); old: the values it accumulates onto, or None = NaN sentinel"""
    B, H, W, Cc, _ = c.shp
    g = FP.Guarded(B * H * W * ld, torch.float32, dev)
    buf = g.t.view(B, H, W, ld)
    if old is not None:
        buf[..., :Cc] = old.to(dev)
    return g, ops.View(buf, B, H, W, Cc, ld)


def _rows_written(g, v, accumulated, what):
    """guards intact, the padding channels keep the sentinel, every one of the C channels was written; -> the C channels as a CPU tensor"""
    g.assert_guards(what)
    b = g.payload_bits().view(v.B, v.H, v.W, v.ld)
    pad = b[..., v.C:] != g.fill
    assert not pad.any(), "%s: %d padding channels behind the %d of rows of %d were written (first at %s)" % (what, int(pad.sum()), v.C, v.ld, pad.nonzero()[0].tolist())
    if not accumulated:
        left = b[..., :v.C] == g.fill
        assert not left.any(), "%s: %d of %d elements were never written (first at %s)" % (what, int(left.sum()), left.numel(), left.nonzero()[0].tolist())
    vals = g.t.view(v.B, v.H, v.W, v.ld)[..., :v.C].cpu()
    assert torch.isfinite(vals).all(), "%s: %d elements are not finite" % (what, int((~torch.isfinite(vals)).sum()))
    return vals


def _run_bwd(backend, c, prec):
    """-> (dL, dR as CPU tensors, their buffers' bits, the note); footprints asserted here"""
    lib, dev = backend.lib, backend.device
    B, H, W, Cc, md = c.shp
    Lv = ops.View(FP.wide_rows(c.L, c.l_ld, dev), B, H, W, Cc, c.l_ld)
    Rv = ops.View(FP.wide_rows(c.R, c.r_ld, dev), B, H, W, Cc, c.r_ld)
    gb = torch.full((B, H, W, c.g_ld), float("nan"))                      # every column outside the volume is NaN: none of them may reach a result
    gb[..., c.gcoff:c.gcoff + c.D] = c.g
    gv = ops.View(gb.to(dev), B, H, W, c.D, c.g_ld)
    gl, dL = _grad_out(dev, c, c.dl_ld, c.oldl if c.acc_l else None)
    gr, dR = _grad_out(dev, c, c.dr_ld, c.oldr if c.acc_r else None)
    ops.corr_bwd(lib, gv, Lv, Rv, dL, dR, md, 1, coff=c.gcoff, acc_l=bool(c.acc_l), acc_r=bool(c.acc_r), precision=prec)
    note = _note(lib)
    backend.sync()
    what = "%s precision %d g rows of %d at %d acc %d%d (%s)" % (c.what, prec, c.g_ld, c.gcoff, c.acc_l, c.acc_r, note)
    vl = _rows_written(gl, dL, c.acc_l, what + " dL")
    vr = _rows_written(gr, dR, c.acc_r, what + " dR")
    return vl, vr, (gl.payload_bits().clone(), gr.payload_bits().clone()), note


def _check_bwd(W_, c, what, kernel, vl, vr):
    rl, rr = c.bwd_ref(kernel)
    W_.check(what, kernel, "dL", vl, rl + (c.oldl.double() if c.acc_l else 0))
    W_.check(what, kernel, "dR", vr, rr + (c.oldr.double() if c.acc_r else 0))


def test_corr_band_bwd_sweep(backend):
    """mh_corr_bwd_prec at precisions 0 and 1 over the same shapes: g as a channel slice at offset 0 / 4 (16-byte staging) or 3 (scalar staging) of rows whose
    other columns are NaN, dL / dR in guarded rows of C or C + 8 floats, the four (acc_l, acc_r) combinations; the dispatched kernel asserted, the fp32
    pair's fall to the gather kernel at C = 256 included; every eighth shape launched twice (same bits)"""
    W_ = _Worst("mh_corr_bwd_prec")
    seen = set()
    assert {(_case(k).acc_l, _case(k).acc_r) for k in range(len(SHAPES))} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(_case(k).gcoff, _case(k).shp[3]) for k in range(len(SHAPES))} >= {(3, Cc) for Cc in (32, 64, 128, 256)}
    for k in range(len(SHAPES)):
        c = _case(k)
        B, H, W, Cc, md = c.shp
        for prec in (0, 1):
            what = "%s precision %d" % (c.what, prec)
            vl, vr, b0, note = _run_bwd(backend, c, prec)
            expect = _bwd_dispatch(Cc, md, prec)
            assert note.startswith(expect), "%s: ran %s, the dispatch conditions say %s" % (what, note, expect)
            if "bf16" in expect:
                assert "one grid" in note, note
            seen.add(expect)
            _check_bwd(W_, c, what, expect, vl, vr)
            if k % 8 == 0:
                _, _, b1, _ = _run_bwd(backend, c, prec)
                assert torch.equal(b0[0], b1[0]) and torch.equal(b0[1], b1[1]), "%s: two launches of %s differ" % (what, expect)
    W_.report(backend, len(SHAPES))
    need = ["corr_bwd_mfma<C/16=%d>" % n for n in (1, 2, 4, 8, 16)] + ["corr_bwd_mfma_bf16_pair<C/16=%d>" % n for n in (2, 4, 8, 16)] + ["corr_bwd_kernel"]
    missing = [n for n in need if n not in seen]
    assert not missing, "kernel instances the sweep never launched: %s (seen %s)" % (missing, sorted(seen))


# ---- the variants behind mh_tune_corr: workgroup order, one grid or two ---------------------------------------------------------------------------
def _variant_shapes():
    """about ten shapes the bf16 kernels serve: every channel count, one to fifteen workgroups, more than one segment per row"""
    ks, residues = [], set()
    for Cc in (32, 64, 128, 256):
        own = [k for k, s in enumerate(SHAPES) if s[3] == Cc and "bf16" in _fwd_dispatch(Cc, s[4], 2)]
        for n in range(2 if Cc == 256 else 3):
            # first a row of several segments, then workgroup counts mod 8 not yet taken
            rank = lambda k: (-((SHAPES[k][2] + 63) // 64 > 1) if n == 0 else 0, _nwg(SHAPES[k]) % 8 in residues, k)
            k = min((k for k in own if k not in ks), key=rank)
            ks.append(k)
            residues.add(_nwg(SHAPES[k]) % 8)
    return sorted(ks)


VARIANTS = _variant_shapes()


def test_corr_band_bwd_variants_bit_identical(backend):
    """precision 1 under mh_tune_corr 1, 1|2 (no XCD-aware workgroup order), 1|4 (corr_bwd_mfma_bf16_one: two grids), 1|2|4: every workgroup does the same
    arithmetic whatever its id or grid, so dL and dR are the same bits; likewise the forward at precisions 1 and 2 with the remap on and off"""
    lib = backend.lib
    W_ = _Worst("mh_corr_bwd_prec variants")
    seen = set()
    assert {SHAPES[k][3] for k in VARIANTS} == {32, 64, 128, 256} and len({_nwg(SHAPES[k]) % 8 for k in VARIANTS}) >= 4, VARIANTS
    try:
        for k in VARIANTS:
            c = _case(k)
            B, H, W, Cc, md = c.shp
            first = None
            for tune in (1, 1 | 2, 1 | 4, 1 | 2 | 4):
                lib.tune_corr(tune)
                what = "%s mh_tune_corr(%d)" % (c.what, tune)
                vl, vr, b, note = _run_bwd(backend, c, 1)
                expect = _bwd_dispatch(Cc, md, 1, pair=not (tune & 4))
                assert note.startswith(expect) and (("two grids" in note) if tune & 4 else ("one grid" in note)), "%s: ran %s, expected %s" % (what, note, expect)
                seen.add(expect)
                _check_bwd(W_, c, what, expect, vl, vr)
                if first is None:
                    first = b
                assert torch.equal(first[0], b[0]), "%s: dL differs from mh_tune_corr(1)" % what
                assert torch.equal(first[1], b[1]), "%s: dR differs from mh_tune_corr(1)" % what
            for prec in (1, 2):
                bits = []
                for tune in (1, 1 | 2):
                    lib.tune_corr(tune)
                    _, b, note = _run_fwd(backend, c, prec)
                    assert note.startswith(_fwd_dispatch(Cc, md, prec)) and "bf16" in note, note
                    bits.append(b)
                assert torch.equal(bits[0], bits[1]), "%s precision %d: the forward differs with the workgroup remap off" % (c.what, prec)
    finally:
        lib.tune_corr(1)
    W_.report(backend, len(VARIANTS))
    need = ["corr_bwd_mfma_bf16_%s<C/16=%d>" % (f, n) for f in ("pair", "one") for n in (2, 4, 8, 16)]
    missing = [n for n in need if n not in seen]
    assert not missing, "kernel instances the test never launched: %s (seen %s)" % (missing, sorted(seen))
