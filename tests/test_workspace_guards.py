"""Workspaces of EXACTLY the queried size: every entry point that takes a workspace, a bank or a table-described destination runs with that buffer
inside guard zones (tests/footprint.py), outputs guarded as well, results against float64 oracles.  A kernel that writes one element past the size
its query states, or leaves part of a "fully overwritten" workspace unwritten, fails here; the existing parity tests hand every kernel an arena or
a rounded-up allocation and cannot see either."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as FP
import sgm_oracle
from madnet_hip import _ffi, ops
from oracle import tf_ops as T


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _wide(x, ld, dev, fill=7.0):
    B, H, W, Cc = x.shape
    buf = torch.full((B, H, W, ld), fill)
    buf[..., :Cc] = x
    buf = buf.to(dev)
    return buf, ops.View(buf, B, H, W, Cc, ld)


def P(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


# ---- mh_conv2d_wgrad_partial / _group ---------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, k, stride, dil, precision)
WGRAD_CASES = [
    (1, 6, 20, 1, 16, 3, 1, 1, 0),          # one input channel
    (1, 9, 13, 3, 16, 3, 2, 1, 0),          # the image layer, odd size, stride 2
    (2, 20, 28, 3, 16, 5, 2, 1, 1),         # bf16, Cin <= 4 and 25 taps: the tap-flattened instance
    (1, 10, 12, 4, 1, 3, 1, 1, 0),          # one output channel
    (1, 7, 11, 38, 20, 3, 1, 1, 0),         # ragged on both sides (rows of 40 / 20)
    (1, 7, 11, 38, 20, 3, 1, 1, 1),
    (1, 12, 16, 4, 64, 3, 1, 4, 1),         # dilation 4
    (1, 8, 8, 3, 20, 5, 2, 1, 0),           # 5x5 stride 2
    (1, 5, 7, 64, 16, 1, 1, 1, 0),          # 1x1
    (1, 16, 40, 64, 64, 3, 1, 1, 1),        # 640 reduction pixels
    (1, 16, 40, 38, 64, 3, 1, 4, 0),
    (1, 65, 64, 72, 80, 3, 1, 1, 1),        # > 4096 pixels, > 64 channels both ways: the eight-wave 128x128 tile
]
_wgrad_ref = {}


def _wgrad_data(case):
    """operands (CPU) + float64 filter / bias gradients on the operands as the precision rounds them; made once per case"""
    if case not in _wgrad_ref:
        B, H, W, Ci, Co, k, s, dil, prec = case
        Ho, Wo, _, _ = ops.conv_geometry(H, W, k, k, s, dil)
        x = _rand((B, H, W, Ci), 11); gz = _rand((B, Ho, Wo, Co), 14)
        xr, zr = (_bf(x), _bf(gz)) if prec == 1 else (x, gz)
        w0 = torch.zeros(k, k, Ci, Co, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(T.conv2d(xr.double(), w0, None, stride=s, dilation=dil, alpha=1.0), [w0], zr.double())
        _wgrad_ref[case] = (x, gz, gw, gz.double().sum((0, 1, 2)))          # (the bias gradient is exact fp32 in every mode)
    return _wgrad_ref[case]


def _split_counts(lib, d, xv, zv, M):
    """the queried split count and one more legal count of the other kind (1 <-> several) where the geometry has one"""
    sp = C.c_int32(0)
    lib.conv2d_wgrad_partial(C.byref(d), ops._p(xv), ops._p(zv), zv.ld, None, C.byref(sp), None, None)
    out = [sp.value]
    for alt in ([1] if sp.value > 1 else [2, 3, 5]):
        if -(-M // -(-M // alt)) == alt:             # the library's rule: a forced count must reproduce itself
            out.append(alt)
            break
    return out


@pytest.mark.parametrize("group", [False, True], ids=["single", "group"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_partial_exact_workspace(backend, case, group):
    """ws of exactly splits * (taps*K*N + N) floats (taps*K*N with one split: the bias addend then goes to db): fully written, nothing behind it,
    the summed splits = the oracle's filter gradient (1e-4; 2e-4 for bf16 operands), the bias partials sum to the bias gradient, two calls give the
    same bits.  With the queried split count and with a forced one of the other kind (one <-> several)."""
    lib, dev = backend.lib, backend.device
    B, H, W, Ci, Co, k, s, dil, prec = case
    x, gz, gw, gb = _wgrad_data(case)
    Ho, Wo, pt, pl = ops.conv_geometry(H, W, k, k, s, dil)
    xb, xv = _wide(x, FP.round_up(Ci, 4), dev)
    zb, zv = _wide(gz, FP.round_up(Co, 4) if Co > 1 else 1, dev)
    d = ops.conv_desc(B, H, W, Ho, Wo, Ci, Co, k, k, s, dil, pt, pl, 0, 0, xv.ld, zv.ld, precision=prec)
    size = k * k * Ci * Co
    tolw = (1e-4 if prec == 0 else 2e-4) * max(1.0, gw.abs().max().item())
    tolb = 1e-4 * max(1.0, gb.abs().max().item())
    counts = _split_counts(lib, d, xv, zv, B * Ho * Wo)
    for ns in counts:
        runs = []
        for rep in range(2):
            nws = ns * size + (ns * Co if ns > 1 else 0)
            ws = FP.Guarded(nws, torch.float32, dev)
            db = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
            sp = C.c_int32(ns)
            if group:
                it = (_ffi.WgradItem * 1)()
                it[0].d, it[0].inp, it[0].dout, it[0].ws, it[0].db, it[0].dout_ld, it[0].splits = d, xv.ptr, zv.ptr, ws.ptr(), db.ptr(), zv.ld, ns
                rc = lib._raw_mh_conv2d_wgrad_partial_group(it, 1, None)
            else:
                rc = lib._raw_mh_conv2d_wgrad_partial(C.byref(d), ops._p(xv), ops._p(zv), zv.ld, C.c_void_p(ws.ptr()), C.byref(sp), C.c_void_p(db.ptr()), None)
            name = lib.last_kernel().decode()
            backend.sync()
            if rc != 0 and ns != counts[0] and b"does not match" in lib.last_error():
                break                                        # this geometry's kernel has no such split count: only the queried one is legal
            what = "%s splits=%d [%s]" % (case, ns, name)
            assert rc == 0, (what, lib.last_error())
            FP.assert_fully_written(ws, nws, what)
            db.assert_guards(what)
            wsv = ws.t.cpu()
            dw = wsv[:ns * size].view(ns, size).double().sum(0).view(k, k, Ci, Co)
            err = (dw - gw).abs().max().item()
            assert err <= tolw, (what, err, tolw)
            if ns > 1:
                assert (db.t.cpu() == 0).all(), what + ": db must not be touched when the bias partials go to the workspace"
                bsum = wsv[ns * size:].view(ns, Co).double().sum(0)
            else:
                bsum = db.t.cpu().double()
            assert (bsum - gb).abs().max().item() <= tolb, (what, (bsum - gb).abs().max().item())
            runs.append((ws.payload_bits().clone(), FP.bits(db.t).clone()))
        else:
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "%s splits=%d: two calls differ" % (case, ns)
            print("wgrad_partial %s %s splits=%d: |dw err| %.3g (bound %.3g) [%s]" % ("group" if group else "single", case, ns, err, tolw, name))


# ---- mh_wgrad_reduce ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
def test_wgrad_reduce_guarded_destinations(backend, accumulate):
    """sizes around the 1024-element block (1, 1023, 1024, 1025) and a real layer's 9*38*20, 1 / 2 / 13 splits, all in one table: every dst inside
    guards, dst = (old +) the float64 sum of the splits"""
    lib, dev = backend.lib, backend.device
    segs, keep, checks = [], [], []
    for i, (size, splits) in enumerate([(s, n) for s in (1, 1023, 1024, 1025, 9 * 38 * 20) for n in (1, 2, 13)]):
        ws = FP.Guarded(size * splits, torch.float32, dev).set(_rand((splits * size,), 100 + i))
        dst = FP.Guarded(size, torch.float32, dev)
        old = _rand((size,), 200 + i)
        if accumulate:
            dst.set(old)
        segs.append((ws.ptr(), dst.ptr(), size, splits))
        checks.append((ws, dst, ws.t.cpu().view(splits, size).double().sum(0) + (old.double() if accumulate else 0), ws.snapshot(), size, splits))
    ops.wgrad_reduce(lib, segs, dev, keep, accumulate=bool(accumulate))
    backend.sync()
    worst = 0.0
    for ws, dst, ref, snap, size, splits in checks:
        what = "reduce size=%d splits=%d acc=%d" % (size, splits, accumulate)
        FP.assert_untouched(ws, snap, what)
        FP.assert_fully_written(dst, size, what)
        err = (dst.t.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst = max(worst, err)
        assert err <= 1e-5, (what, err)           # <= 14 fp32 additions of O(1) values: 14 * 2^-24 * sqrt(13) ~ 3e-6
    print("wgrad_reduce acc=%d: worst relative error %.3g" % (accumulate, worst))


# ---- mh_wgrad_stream ------------------------------------------------------------------------------------------------------------------------
# (layers (B, H, W, Cin, Cout, dil, in_ld) with H, W the INPUT size, target workgroups, waves, stride)
STREAM_CASES = [
    ([(1, 12, 70, 38, 64, 1, 40), (1, 12, 70, 64, 1, 1, 64)], 12, 4, 1),       # STREAM_BATCHES[1] of tests/test_wgrad_stream.py
    ([(2, 7, 33, 32, 40, 1, 32)], 6, 8, 1),                                     # STREAM_BATCHES[2]
    ([(1, 6, 20, 64, 64, 1, 64)], 1, 4, 1),                                     # one workgroup: a single split stores straight into dw
    ([(1, 12, 64, 16, 32, 1, 16)], 4, 4, 2),                                    # stride 2
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=["38to64+head", "b2_n40", "one_split", "stride2"])
def test_wgrad_stream_exact_workspace(backend, case):
    """per layer ws = exactly splits * 9*K*N + splits * N floats (splits from mh_wgrad_stream_plan); with one split the kernel stores into dw itself,
    which is guarded then.  Filter gradients against the float64 oracle on bf16-rounded operands (2e-5, tests/test_wgrad_stream.py)."""
    lib, dev = backend.lib, backend.device
    layers, wgs, nw, stride = case
    n = len(layers)
    arr = (_ffi.WgsLayer * n)()
    keep, pairs, refs = [], [], []
    for i, (B, H, W, Ci, Co, dil, ild) in enumerate(layers):
        x = _rand((B, H, W, Ci), 700 + 2 * i); gz = _rand((B, H // stride, W // stride, Co), 701 + 2 * i)
        xb, xv = _wide(x, ild, dev, fill=7.5)
        zd = gz.to(dev)
        xs, zs = ops.Shadow(B, H, W, Ci, dev), ops.Shadow(B, H // stride, W // stride, Co, dev)
        pairs += [(xv, xs), (ops.view(zd) if Co > 1 else ops.view(zd[..., 0].contiguous()), zs)]
        keep += [xb, zd, xs, zs]
        w0 = torch.zeros(3, 3, Ci, Co, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(T.conv2d(_bf(x).double(), w0, None, stride=stride, dilation=dil, alpha=1.0), [w0], _bf(gz).double())
        refs.append((gw, _bf(gz).double().sum((0, 1, 2))))
        L = arr[i]
        L.x, L.dz = xs.ptr, zs.ptr
        L.B, L.H, L.W, L.K, L.N, L.dil, L.x_ld, L.dz_ld, L.stride = B, H // stride, W // stride, Ci, Co, dil, xs.ld, zs.ld, stride
    ops.shadow_cast(lib, pairs, dev, keep)
    nwaves = min(nw, 5) if stride == 2 else nw
    nblk = C.c_int32(0)
    lib.wgrad_stream_plan(arr, n, wgs, nwaves, C.byref(nblk))
    bufs = []
    for i, (B, H, W, Ci, Co, dil, ild) in enumerate(layers):
        L = arr[i]
        size = 9 * Ci * Co
        ws = FP.Guarded(L.splits * size + (L.splits * Co if L.splits > 1 else 0), torch.float32, dev)
        db = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
        L.ws, L.db = ws.ptr(), db.ptr()
        bufs.append((ws, db, size, L.splits))
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    lib.wgrad_stream(C.c_void_p(table.data_ptr()), n, nblk.value, nwaves, (-2 if stride == 2 else max(l[5] for l in layers)), None)
    name = lib.last_kernel().decode()
    backend.sync()
    assert "wgrad_stream_kernel" in name, name
    if case is STREAM_CASES[2]:
        assert bufs[0][3] == 1
    for (ws, db, size, ns), (gw, gb), lay in zip(bufs, refs, layers):
        what = "stream %s splits=%d [%s]" % (lay, ns, name)
        FP.assert_fully_written(ws, ws.n, what)
        db.assert_guards(what)
        Ci, Co = lay[3], lay[4]
        v = ws.t.cpu()
        dw = v[:ns * size].view(ns, size).double().sum(0).view(3, 3, Ci, Co)
        err = (dw - gw).abs().max().item()
        assert err <= 2e-5 * max(1.0, gw.abs().max().item()), (what, err)
        bsum = v[ns * size:].view(ns, Co).double().sum(0) if ns > 1 else db.t.cpu().double()
        if ns > 1:
            assert (db.t.cpu() == 0).all(), what
        assert (bsum - gb).abs().max().item() <= 1e-4 * max(1.0, gb.abs().max().item()), what
        print("%s: |dw err| %.3g" % (what, err))


# ---- mh_bias_grad_partial ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1000, 1, 1), (777, 3, 4), (513, 12, 16), (300, 64, 64), (129, 200, 200), (70, 1024, 1024), (5, 96, 100), (40000, 32, 32)])
def test_bias_grad_partial_exact_workspace(backend, case):
    """ws of exactly mh_bias_grad_blocks(npix, nch) * nch floats: fully written, nothing behind it, the rows sum to the column sums"""
    lib, dev = backend.lib, backend.device
    npix, nch, ld = case
    t = _rand((1, 1, npix, ld), 31)
    ref = t.double()[0, 0, :, :nch].sum(0)
    td = t.to(dev)
    nb = lib.bias_grad_blocks(npix, nch)
    assert 1 <= nb <= 1024
    ws = FP.Guarded(nb * nch, torch.float32, dev)
    lib.bias_grad_partial(P(td), ld, npix, nch, C.c_void_p(ws.ptr()), nb, None)
    backend.sync()
    FP.assert_fully_written(ws, nb * nch, "bias_grad_partial %s blocks=%d" % (case, nb))
    err = (ws.t.cpu().view(nb, nch).double().sum(0) - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, ref.abs().max().item()), err          # the bound of test_bias_grad_partial_column_sums


# ---- mh_pack_weights --------------------------------------------------------------------------------------------------------------------------
def _unpack32(bank, taps, K, N, planes, kc16):
    """the 32x32x16 register image back to [plane][tap][K16 * 16][N32 * 32] (bf16 values as float), by the layout include/madnet_hip.h states"""
    k16 = (K + 15) // 16
    k16p = FP.round_up(k16, kc16) if kc16 else k16
    n32 = (N + 31) // 32
    nchunk, steps = (k16p // kc16, kc16) if kc16 else (1, k16p)
    b = bank.view(nchunk, taps, steps, n32, planes, 64, 8)
    out = torch.zeros(planes, taps, k16p * 16, n32 * 32)
    for l in range(64):
        rows = torch.arange(8) + 8 * (l >> 5)
        for ch in range(nchunk):
            for st in range(steps):
                k0 = 16 * (ch * steps + st)
                # [taps, n32, planes, 8] -> out[plane, tap, k0 + rows, 32 * tile + (l & 31)]
                v = b[ch, :, st, :, :, l, :]
                for tl in range(n32):
                    out[:, :, k0 + rows, 32 * tl + (l & 31)] = v[:, tl].permute(1, 0, 2)
    return out


@pytest.mark.parametrize("K", [33, 128, 136, 385])
def test_pack_weights_exact_banks(backend, K):
    """banks of exactly mh_pack_bytes / mh_pack32_bytes (halved for one plane) bytes for trans 0, 1, 2 (two planes and one), 3, three segments per
    table: every bank fully written (zero padding included), nothing outside it; the bank in the middle does not touch its neighbours; the trans 2 / 3
    images decode to bf16(w) / the mirrored transposed bf16(w) with zeros in the padded reduction steps and columns."""
    lib, dev = backend.lib, backend.device
    N = 24 if K > 128 else 40
    w = _rand((3, 3, K, N), 5, 0.2)
    wd = w.to(dev)
    kc = lib.planes_kc16(K)
    assert kc == ops.planes_kc16(K)
    # (planes, trans, bytes by the library's own query)
    forms = [(2, 0, lib.pack_bytes(9, K, N, 2)), (1, 0, lib.pack_bytes(9, K, N, 1)), (1, 1, lib.pack_bytes(9, N, K, 1)),
             (2, 2, lib.pack32_bytes(9, K, N)), (1, 2, lib.pack32_bytes(9, K, N) // 2), (1, 3, lib.pack32_bytes(9, N, K) // 2)]
    for planes, trans, nbytes in forms:
        assert nbytes == ops.pack_bytes(wd, planes, trans) and nbytes % 2 == 0
        banks = [FP.Guarded(nbytes // 2, torch.bfloat16, dev) for _ in range(3)]
        keep = []
        ops.pack_weights(lib, [(wd, bk.t, planes, trans) for bk in banks], dev, keep)
        backend.sync()
        what = "pack K=%d N=%d planes=%d trans=%d" % (K, N, planes, trans)
        for bk in banks:
            bk.assert_guards(what)
            assert torch.equal(bk.payload_bits(), banks[0].payload_bits()), what + ": the three segments differ"
        v = banks[1].t.cpu().float()
        assert torch.isfinite(v).all(), what + ": part of the bank was not written"
        wq = _bf(w)
        if trans == 2:
            img = _unpack32(v, 9, K, N, planes, kc)
            exp = torch.zeros_like(img)
            exp[0, :, :K, :N] = wq.view(9, K, N)
            if planes == 2:
                exp[1, :, :K, :N] = _bf(w - wq).view(9, K, N)
            assert torch.equal(img, exp), what
        elif trans == 3:
            img = _unpack32(v, 9, N, K, 1, lib.planes_kc16(N))
            exp = torch.zeros_like(img)
            exp[0, :, :N, :K] = wq.view(9, K, N).flip(0).transpose(1, 2)
            assert torch.equal(img, exp), what
        else:
            # bank[(tap * ceil(K/32) + chunk)][16-column tile][plane][lane][8]: lane l holds w[tap][32 chunk + 8 (l >> 4) .. + 7][16 tile + (l & 15)]
            Kr, Nc = (K, N) if trans == 0 else (N, K)
            src = wq.view(9, K, N) if trans == 0 else wq.view(9, K, N).transpose(1, 2)
            lo = (_bf(w - wq).view(9, K, N) if trans == 0 else None)
            k32, n16 = (Kr + 31) // 32, (Nc + 15) // 16
            b = v.view(9, k32, n16, planes, 64, 8)
            full = torch.zeros(planes, 9, k32 * 32, n16 * 16)
            full[0, :, :Kr, :Nc] = src
            if planes == 2:
                full[1, :, :Kr, :Nc] = lo
            for l in range(64):
                rows = 8 * (l >> 4) + torch.arange(8)
                for ch in range(k32):
                    got = b[:, ch, :, :, l, :]                                             # [tap, tile, plane, 8]
                    want = full[:, :, 32 * ch + rows][..., (l & 15)::16]                   # [plane, tap, 8, tile]
                    assert torch.equal(got, want.permute(1, 3, 0, 2)), (what, l, ch)


# ---- mh_shadow_cast / mh_plane_split ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["shadow_cast", "plane_split"])
def test_shadow_tables_guarded(backend, split):
    """dst_ld wider than round_up(C, 32), a source that is a slice of wider rows, the concat form (plane_split: src | src2), and npix * dst_ld / 8 not a
    multiple of the 256-thread block: every destination exactly npix * dst_ld halfs inside guards, fully written (zero padding included), sources
    untouched"""
    lib, dev = backend.lib, backend.device
    # (B, H, W, C, src_ld, coff, dst_ld, C2)
    cases = [(1, 5, 7, 32, 32, 0, 32, 0), (2, 3, 9, 38, 48, 5, 64, 0), (1, 4, 6, 1, 3, 1, 32, 0), (1, 3, 5, 70, 72, 0, 128, 0), (1, 7, 11, 33, 40, 4, 40, 0)]
    if split:
        cases += [(1, 6, 9, 32, 32, 0, 64, 1), (2, 5, 7, 16, 24, 4, 32, 7)]
    if split:
        arr = (_ffi.PlaneSeg * len(cases))()
    else:
        arr = (_ffi.ShadowSeg * len(cases))()
    blk, keep, checks = 0, [], []
    for i, (B, H, W, Cc, sld, coff, dld, C2) in enumerate(cases):
        npix = B * H * W
        src = FP.Guarded(npix * sld, torch.float32, dev).set(_rand((npix * sld,), 40 + i))
        hi = FP.Guarded(npix * dld, torch.bfloat16, dev)
        lo = FP.Guarded(npix * dld, torch.bfloat16, dev) if split else None
        s2 = FP.Guarded(npix * (C2 + 2), torch.float32, dev).set(_rand((npix * (C2 + 2),), 60 + i)) if C2 else None
        a = arr[i]
        a.src, a.npix, a.C, a.src_ld, a.dst_ld, a.blk0 = src.ptr(coff), npix, Cc, sld, dld, blk
        if split:
            a.hi, a.lo = hi.ptr(), lo.ptr()
            if C2:
                a.src2, a.C2, a.src2_ld = s2.ptr(1), C2, C2 + 2
        else:
            a.dst = hi.ptr()
        blk += (npix * (dld // 8) + 255) // 256
        want = src.t.cpu().view(npix, sld)[:, coff:coff + Cc]
        if C2:
            want = torch.cat([want, s2.t.cpu().view(npix, C2 + 2)[:, 1:1 + C2]], 1)
        checks.append((src, s2, hi, lo, want, npix, dld, [g.snapshot() for g in (src, s2) if g is not None]))
    assert any((c[5] * (c[6] // 8)) % 256 for c in checks)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    (lib.plane_split if split else lib.shadow_cast)(C.c_void_p(table.data_ptr()), len(cases), blk, None)
    backend.sync()
    for k, (src, s2, hi, lo, want, npix, dld, snaps) in enumerate(checks):
        what = "%s case %d" % ("plane_split" if split else "shadow_cast", k)
        for g, sn in zip([g for g in (src, s2) if g is not None], snaps):
            FP.assert_untouched(g, sn, what)
        Cc = want.shape[1]
        exp_hi = torch.zeros(npix, dld, dtype=torch.bfloat16); exp_hi[:, :Cc] = want.to(torch.bfloat16)
        hi.assert_guards(what)
        assert torch.equal(hi.payload_bits(), FP.bits(exp_hi).view(-1)), what + ": hi plane"
        if lo is not None:
            exp_lo = torch.zeros(npix, dld, dtype=torch.bfloat16); exp_lo[:, :Cc] = (want - want.to(torch.bfloat16).float()).to(torch.bfloat16)
            lo.assert_guards(what)
            assert torch.equal(lo.payload_bits(), FP.bits(exp_lo).view(-1)), what + ": lo plane"


# ---- mh_sgm_proxy -----------------------------------------------------------------------------------------------------------------------------
SGM_CASES = [(1, 7, 9, 64), (2, 9, 17, 128), (3, 12, 65, 192), (1, 10, 129, 64)]
_sgm = {}


def _sgm_data(case):
    """a textured left view and the right view of a scene at disparity 3 (+ noise), uint8; the oracle's labels -- made once"""
    if case not in _sgm:
        B, H, W, D = case
        rng = np.random.default_rng(sum(case))
        l = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        r = np.roll(l, -3, axis=2)
        r = np.clip(r.astype(np.int32) + rng.integers(-6, 7, r.shape), 0, 255).astype(np.uint8)
        ref = sgm_oracle.sgm_proxy(l, r, D)
        ref.setflags(write=False)
        _sgm[case] = (l, np.ascontiguousarray(r), ref)
    return _sgm[case]


@pytest.mark.parametrize("case", SGM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_sgm_proxy_exact_workspace(backend, case):
    """ws of exactly mh_sgm_ws_bytes bytes, the labels guarded: the smallest legal frame (7 x 9), W < D, W one past 128, three images at D = 192.
    Pass rule of tests/test_sgm_proxy.py: valid mask and integer disparities equal the oracle's, the value within one float32 ulp."""
    lib, dev = backend.lib, backend.device
    B, H, W, D = case
    l, r, ref = _sgm_data(case)
    nbytes = lib.sgm_ws_bytes(B, H, W, D)
    outs = []
    for rep in range(2):
        ws = FP.Guarded(nbytes, torch.uint8, dev)
        out = FP.Guarded(B * H * W, torch.float32, dev)
        assert ws.ptr() % 16 == 0
        ops.sgm_proxy(lib, torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev), ws.t, out.t, D)
        backend.sync()
        ws.assert_guards("sgm ws %s (%d bytes)" % (case, nbytes))
        FP.assert_fully_written(out, B * H * W, "sgm labels %s" % (case,))
        outs.append(out.t.cpu().numpy().reshape(B, H, W))
    got = outs[0]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(got > 0, ref > 0), "valid masks differ at %d pixels" % np.count_nonzero((got > 0) != (ref > 0))
    assert np.all(got >= 0) and np.array_equal(np.floor(got), np.floor(ref))
    ulp = np.float64(2.0) ** -23 * 2.0 ** np.ceil(np.log2(np.maximum(ref.astype(np.float64), 1.0)))
    assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp)
    print("sgm %s: %d valid labels of %d" % (case, int((ref > 0).sum()), ref.size))


# ---- mh_frame_prepare -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(15, 22), (70, 80)], ids=["15x22", "70x80"])
def test_frame_prepare_exact_workspace(backend, shape):
    """ws of exactly mh_frame_prepare_ws_floats floats and the three outputs inside guards, all augmentations on (two launches: partial sums, apply);
    against the float64 restatement of tests/test_frame_prepare.py, within 2x the fp32 host augment's own distance from it (that module's rule)."""
    import test_frame_prepare as TF
    lib, dev = backend.lib, backend.device
    H, W = shape
    srcs = TF._sources([(90, 100), (75, 131)], seed=9)
    origins = [(11, 13), (5, 51)]
    B = 2
    table = ops.FrameTable(lib, dev, B)
    held = []
    for b, ((l, r, g), (r0, c0)) in enumerate(zip(srcs, origins)):
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev) for a in (l, r, g)]
        held.append(t)
        table.set(b, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), l.shape[0], l.shape[1], r0, c0, 1 if g.dtype == np.uint16 else 0, 7, TF.DELTA, TF.CONTRAST, TF.HUE)
    nws = lib.frame_prepare_ws_floats(B, H, W)
    ws = FP.Guarded(nws, torch.float32, dev)
    outs = [FP.Guarded(B * H * W * c, torch.float32, dev) for c in (3, 3, 1)]
    ops.frame_prepare(lib, table, outs[0].t.view(B, H, W, 3), outs[1].t.view(B, H, W, 3), outs[2].t.view(B, H, W, 1), ws.t)
    note = lib.last_kernel().decode()
    backend.sync()
    assert "2 launches" in note, note
    ws.assert_guards("frame_prepare ws (%d floats)" % nws)
    for o in outs:
        FP.assert_fully_written(o, o.n, "frame_prepare output")
    kl, kr, kg = (o.t.cpu().numpy().reshape(B, H, W, c) for o, c in zip(outs, (3, 3, 1)))
    host_d = kern_d = 0.0
    for b in range(B):
        wl, wr, wg = TF._host_windows(srcs[b], origins[b], H, W, "random_crop")
        assert np.array_equal(kg[b], wg)
        hl, hr = TF.data_reader.augment(wl, wr, TF.Fixed(TF._draws(7)))
        for k_img, h_img, w_img in ((kl[b], hl, wl), (kr[b], hr, wr)):
            y = TF.augment64(w_img, 7)
            host_d = max(host_d, float(np.abs(h_img.astype(np.float64) - y).max()))
            kern_d = max(kern_d, float(np.abs(k_img.astype(np.float64) - y).max()))
    print("frame_prepare %dx%d: host %.3g kernel %.3g from the float64 statement" % (H, W, host_d, kern_d))
    assert kern_d <= 2.0 * host_d


# ---- mh_proxy_loss_scaled / mh_metrics_kitti -----------------------------------------------------------------------------------------------------
def _proxy_case(B, H, W, s):
    """data of tests/test_proxy_scaled.py with the first seed at which no resized label sits on a threshold of the validity rule"""
    import test_proxy_scaled as TP
    for seed in range(1, 40):
        pred, px = TP._op_data(B, H, W, s, seed)
        try:
            valid = TP._assert_unambiguous(pred, px, s)
        except AssertionError:
            continue
        return TP, pred, px, valid
    raise AssertionError("no unambiguous seed")


@pytest.mark.parametrize("case", [(2, 37, 53, 2), (2, 37, 53, 4), (1, 260, 257, 2), (1, 260, 257, 4)], ids=lambda c: "%dx%dx%d_s%d" % c)
def test_proxy_loss_scaled_exact_workspace(backend, case):
    """ws of exactly mh_proxy_scaled_ws_floats floats at scale > 1, result and dpred guarded; the bounds of tests/test_proxy_scaled.py"""
    lib, dev = backend.lib, backend.device
    B, H, W, s = case
    TP, pred, px, valid = _proxy_case(B, H, W, s)
    pc = pred.clone().requires_grad_(True)
    p, q = TP._scaled(pc, px, s)
    ref = T.proxy_loss(p, q, 0.1)
    (gref,) = torch.autograd.grad(ref, [pc])
    nws = lib.proxy_scaled_ws_floats(B, H, W, s)
    ws = FP.Guarded(nws, torch.float32, dev)
    res = FP.Guarded(4, torch.float32, dev).set(torch.zeros(4))
    dp = FP.Guarded(B * H * W, torch.float32, dev)
    ops.proxy_loss_scaled(lib, pred.to(dev), px.to(dev), ws.t, res.t, s, dp.t, weight=0.1, grad_scale=1.0)
    backend.sync()
    what = "proxy_loss_scaled %s (%d floats)" % (case, nws)
    ws.assert_guards(what); res.assert_guards(what)
    FP.assert_fully_written(dp, B * H * W, what)
    r = res.t.cpu()
    assert abs(r[0].item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    assert r[1].item() == float(valid.sum().item())
    err = (dp.t.cpu().view(B, H, W) - gref).abs().max().item()
    assert err <= 1e-5 * gref.abs().max().item(), err


def test_metrics_kitti_exact_workspace(backend):
    """1 x 260 x 257 (66820 pixels: a ragged last workgroup) with ws of exactly mh_metrics_kitti_ws_floats floats; the bounds of tests/test_metrics_kitti.py"""
    import test_metrics_kitti as TM
    lib, dev = backend.lib, backend.device
    B, H, W = 1, 260, 257
    disp, gt = TM._data(B, H, W, 3)
    val = gt > 0
    diff = np.abs(gt[val] - disp[val])
    assert (np.abs(diff - 3.0) >= 1e-4).all() and (np.abs(diff / gt[val] - 0.05) >= 1e-4).all()
    epe, d1, nout, nval = TM._reference(disp, gt)
    nws = lib.metrics_kitti_ws_floats(B, H, W)
    ws = FP.Guarded(nws, torch.float32, dev)
    res = FP.Guarded(4, torch.float32, dev).set(torch.full((4,), -1.0))
    ops.metrics_kitti(lib, torch.from_numpy(disp).to(dev), torch.from_numpy(gt).to(dev), ws.t, res.t)
    backend.sync()
    ws.assert_guards("metrics_kitti ws (%d floats)" % nws); res.assert_guards("metrics_kitti result")
    r = res.t.cpu().numpy()
    assert r[2] == float(nval) and r[3] == -1.0
    assert round(float(r[1]) * nval / 100.0) == nout and abs(float(r[1]) - d1) <= 1e-6 * d1
    assert abs(float(r[0]) - float(epe)) <= 1e-6 * float(epe)
