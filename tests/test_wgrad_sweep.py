"""Seeded float64 sweeps of the filter-gradient kernels (csrc/wgrad.hip, csrc/wgrad_stream.hip), in the manner of tests/test_shape_sweep.py: every
list is FIXED, drawn once at import from the literal seed of that file (its _rng); every output and workspace lies in a guarded buffer prefilled with NaN (tests/footprint.py),
the channel padding of every fp32 input row holds NaN; references are autograd of the float64 oracle, on operands rounded to bf16 where the kernel
that ran (mh_last_kernel) rounds them.  The dispatch is host code: each launch asserts the kernel family and the tile shape the shape was built to
reach, restated here from wgrad_dispatch.  No shape is skipped or dropped at run time.

Bounds, relative to max(1, |ref|max): filter gradient 1e-4 (fp32 kernels) and 2e-4 (bf16 kernels against bf16-rounded operands), bias gradient 1e-4
(tests/test_workspace_guards.py); streamed filter gradient 2e-5, its bias gradient 1e-4 (tests/test_wgrad_stream.py)."""
import ctypes as C

import torch

import footprint as FP
from madnet_hip import _ffi, ops
from oracle import tf_ops as T
from test_conv_sweep import _Worst
from test_shape_sweep import _rand, _rng

_bf = FP.bf16_round


def _wide(x, ld, dev):
    """FP.wide_rows and the View of the channels in it"""
    buf = FP.wide_rows(x, ld, dev)
    return buf, ops.View(buf, x.shape[0], x.shape[1], x.shape[2], x.shape[3], ld)


# ---- mh_conv2d_wgrad / _partial / _partial_group ------------------------------------------------------------------------------------------------
# the 12 tile shapes of wgrad_dispatch by (Cin class, Cout class): (low end, high end) of the class.  A tuple = the two counts just above an edge of the
# dispatch, (ragged, 16-byte aligned): 17 / 20 behind 16, 33 / 36 behind 32, 65 / 68 behind 64; a list = a pool to draw from
_KCLASS = [([1, 3, 4, 8, 12], 16), ((17, 17), 32), ((33, 33), 64), ((65, 65), [70, 100])]
_NCLASS_THIN = [([2, 4, 8, 12], 16), ((17, 20), 64), ((65, 68), [72, 100])]            # Cin <= 32: edges at 16 and 64
_NCLASS_WIDE = [([3, 4, 8, 20], 32), ((33, 36), 64), ((65, 68), [72, 100])]            # Cin > 32: edges at 32 and 64
MAC_BUDGET = 24e6                                                                      # taps * Cin * Cout * pixels of one shape (emulator time)


def _pick(r, v, aligned):
    if isinstance(v, tuple):
        return v[1] if aligned else v[0]
    if isinstance(v, list):
        return r.choice([c for c in v if c % 4 == 0] if aligned else v)
    return v


def _wgrad_shapes():
    """(B, H, W, Cin, Cout, k, stride, dil, precision, extra floats per x row, hook): the four corners of every (Cin class, Cout class) cell -- both
    sides of each edge of the dispatch --, then the one-output-channel kernel, the tap-flattened kernel, 1x1 layers, the eight-wave tile and the two
    experimental tiles behind mh_tune_wgrad_wgs"""
    r = _rng("wgrad")
    out = []

    def geom(Ci, Co, ks):
        for attempt in range(100):
            k = r.choice(ks)
            s = r.choice([1, 1, 2])
            dil = r.choice([1, 1, 2, 4]) if (s == 1 and k in (3, 5)) else 1
            B, H, W = r.randint(1, 2), r.randint(1, 14), r.randint(1, 23)
            Ho, Wo, _, _ = ops.conv_geometry(H, W, k, k, s, dil)
            if k * k * Ci * Co * B * Ho * Wo <= MAC_BUDGET:
                return B, H, W, k, s, dil
        raise AssertionError("no geometry for %d x %d" % (Ci, Co))

    cell = 0
    for kc, (klo, khi) in enumerate(_KCLASS):
        for nlo, nhi in (_NCLASS_THIN if kc < 2 else _NCLASS_WIDE):
            for j, (kv, nv) in enumerate(((klo, nlo), (klo, nhi), (khi, nlo), (khi, nhi))):
                prec = (j + cell) % 2            # (the low Cout edge holds the ragged counts: fp32 there in even cells, bf16 in odd ones)
                # precision 1 reaches the bf16 kernel with 16-byte aligned rows on both sides: one such corner per cell always has them; corner 0 of
                # cells 1 and 7 keeps the ragged Cout (17 / 33) and must then run exact fp32; the later precision-0 corner takes x rows of any length
                aligned = prec == 1 and not (j == 0 and cell % 6 == 1)
                Ci, Co = _pick(r, kv, False), _pick(r, nv, aligned)
                B, H, W, k, s, dil = geom(Ci, Co, [1, 3, 3, 3, 4, 5, 7])
                out.append((B, H, W, Ci, Co, k, s, dil, prec, r.choice([0, 4, 1, 3]) if (prec == 0 and j >= 2) else r.choice([0, 4]), 0))
            cell += 1
    for Ci, prec in ((4, 0), (32, 1), (12, 1), (64, 0), (100, 1)):                    # N = 1, 3x3, Cin % 4 == 0: wgrad_n1_kernel (exact fp32 in every mode)
        B, H, W, _, _, _ = geom(Ci, 1, [3])
        s = r.choice([1, 2]); dil = r.choice([1, 2, 4]) if s == 1 else 1
        out.append((B, H, W, Ci, 1, 3, s, dil, prec, r.choice([0, 4]), 0))
    out.append((1, 9, 13, 6, 1, 3, 1, 1, 0, 0, 0))                                     # N = 1 but Cin % 4 != 0: the tiled kernel
    for Ci, Co, k, s in ((3, 16, 7, 2), (1, 32, 5, 1), (4, 64, 4, 2), (2, 20, 7, 1)):  # Cin <= 4, >= 16 taps, bf16: tap-flattened rows
        out.append((r.randint(1, 2), r.randint(5, 14), r.randint(5, 23), Ci, Co, k, s, 1, 1, 0, 0))
    out.append((1, 65, 64, 68, 72, 3, 1, 1, 1, 0, 0))                                  # > 4096 pixels, both sides > 64: eight waves of 32 x 64
    out.append((1, 9, 15, 68, 68, 3, 1, 1, 1, 0, 100000))                              # (experiment hooks) 64 x 64 tiles for a 128-wide layer
    out.append((1, 7, 19, 72, 80, 3, 1, 2, 1, 4, 200000))                              # ... 128 x 128 tile, eight waves of 64 x 32
    return out


WGRAD_SHAPES = _wgrad_shapes()


def _expected_wgrad_kernel(shp, vec):
    """wgrad_entry / wgrad_dispatch restated: the substrings mh_last_kernel() must hold for a single launch of this shape"""
    B, H, W, Ci, Co, k, s, dil, prec, xpad, hook = shp
    Ho, Wo, _, _ = ops.conv_geometry(H, W, k, k, s, dil)
    M = B * Ho * Wo
    vecA, vecB = vec
    if Co == 1 and k == 3 and vecA and Ci % 4 == 0:
        return ("wgrad_n1_kernel",)
    bf16 = prec == 1 and vecA and vecB
    flat = bf16 and Ci <= 4 and k * k >= 16
    K, N = (k * k * 4 if flat else Ci), Co
    if K > 64 and N > 64:
        t = (2, 2, 2, 2) if hook == 100000 else (2, 4, 4, 2) if hook == 200000 else (4, 2, 2, 4) if (M > 4096 and bf16) else (2, 2, 4, 4)
    elif K > 64:
        t = (2, 2, 4, 2) if N > 32 else (4, 1, 2, 1)
    elif K > 32:
        t = (2, 2, 2, 4) if N > 64 else (2, 2, 2, 2) if N > 32 else (4, 1, 1, 1)
    elif K > 16:
        t = (1, 4, 2, 2) if N > 64 else (2, 2, 1, 1) if N > 16 else (2, 1, 1, 1)
    else:
        t = (1, 4, 1, 2) if N > 64 else (1, 2, 1, 1) if N > 16 else (1, 1, 1, 1)
    kern = "wgrad_bf16_kernel<%d,%d,%d,%d>" % t if bf16 else "wgrad_kernel<%d,%d,%d,%d,PT=32,%s>" % (t + ("vec" if (vecA and vecB) else "scalar",))
    return (kern, "tile %dx%d " % (t[0] * t[2] * 16, t[1] * t[3] * 16)) + ((" flat",) if flat else ())


class _WgradCase(object):
    """operands on the device + float64 references of one shape, made once and shared by the three tests"""

    def __init__(self, idx, shp, dev):
        B, H, W, Ci, Co, k, s, dil, prec, xpad, hook = shp
        self.shp, self.idx = shp, idx
        self.Ho, self.Wo, self.pt, self.pl = ops.conv_geometry(H, W, k, k, s, dil)
        x, gz = _rand((B, H, W, Ci), 9000 + 2 * idx), _rand((B, self.Ho, self.Wo, Co), 9001 + 2 * idx)
        self.ref = {}
        for rounded in (False, True):
            xr, zr = (_bf(x), _bf(gz)) if rounded else (x, gz)
            w0 = torch.zeros(k, k, Ci, Co, dtype=torch.float64, requires_grad=True)
            (gw,) = torch.autograd.grad(T.conv2d(xr.double(), w0, None, stride=s, dilation=dil, alpha=1.0), [w0], zr.double())
            self.ref[rounded] = gw
        self.gb = gz.double().sum((0, 1, 2))                          # (the bias gradient is exact fp32 in every mode)
        xld = FP.round_up(Ci, 4) + xpad
        zld = FP.round_up(Co, 4) if Co > 1 else 1
        self.xb, self.xv = _wide(x, xld, dev)
        self.zb, self.zv = _wide(gz, zld, dev)
        self.vec = (xld % 4 == 0, zld % 4 == 0 and Co % 4 == 0)
        self.d = ops.conv_desc(B, H, W, self.Ho, self.Wo, Ci, Co, k, k, s, dil, self.pt, self.pl, 0, 0, xld, zld, precision=prec)
        self.size = k * k * Ci * Co
        self.expected = _expected_wgrad_kernel(shp, self.vec)
        self.what = "shape %d %s" % (idx, shp)

    def tolerance(self, name):
        """(bf16-rounded operands in the oracle?, bound) by the kernel that ran"""
        return (True, 2e-4) if "wgrad_bf16_kernel" in name else (False, 1e-4)

    def query(self, lib):
        sp = C.c_int32(0)
        lib.conv2d_wgrad_partial(C.byref(self.d), ops._p(self.xv), ops._p(self.zv), self.zv.ld, None, C.byref(sp), None, None)
        return sp.value

    def ws_floats(self, ns):
        return ns * self.size + (ns * self.shp[4] if ns > 1 else 0)


_cases = {}


def _case(idx, dev):
    if (idx, dev) not in _cases:
        _cases[(idx, dev)] = _WgradCase(idx, WGRAD_SHAPES[idx], dev)
    return _cases[(idx, dev)]


def _assert_family(cs, name):
    for sub in cs.expected:
        assert sub in name, "%s: expected %s, ran [%s]" % (cs.what, cs.expected, name)


def test_wgrad_shape_list_reaches_every_tile():
    """the fixed list holds every one of the 15 tile shapes of wgrad_dispatch in fp32 and in bf16 form where it has one, the one-channel kernel and the
    tap-flattened rows (decided on the host: nothing is launched)"""
    tiles = set()
    for idx, shp in enumerate(WGRAD_SHAPES):
        Ci, Co, xpad = shp[3], shp[4], shp[9]
        vec = ((FP.round_up(Ci, 4) + xpad) % 4 == 0, Co % 4 == 0)
        tiles.add(_expected_wgrad_kernel(shp, vec)[0].split(",PT")[0].rstrip(">"))
    shapes = ["2,2,4,4", "2,2,4,2", "4,1,2,1", "2,2,2,4", "2,2,2,2", "4,1,1,1", "1,4,2,2", "2,2,1,1", "2,1,1,1", "1,4,1,2", "1,2,1,1", "1,1,1,1"]
    for t in shapes:
        assert "wgrad_bf16_kernel<" + t in tiles and "wgrad_kernel<" + t in tiles, (t, sorted(tiles))
    assert "wgrad_bf16_kernel<4,2,2,4" in tiles and "wgrad_bf16_kernel<2,4,4,2" in tiles and "wgrad_n1_kernel" in tiles, sorted(tiles)
    assert len(WGRAD_SHAPES) >= 60


def test_wgrad_atomic_sweep(backend):
    """mh_conv2d_wgrad: dw += the filter gradient, db += the bias gradient, into zeroed buffers inside guards; values by the kernel that ran"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_conv2d_wgrad")
    for idx, shp in enumerate(WGRAD_SHAPES):
        cs = _case(idx, dev)
        Co, k, hook = shp[4], shp[5], shp[10]
        dw = FP.Guarded(cs.size, torch.float32, dev).set(torch.zeros(cs.size))
        db = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
        lib.tune_wgrad_wgs(hook)
        try:
            rc = lib._raw_mh_conv2d_wgrad(C.byref(cs.d), ops._p(cs.xv), ops._p(cs.zv), cs.zv.ld, C.c_void_p(dw.ptr()), C.c_void_p(db.ptr()), None)
            name = lib.last_kernel().decode()
        finally:
            lib.tune_wgrad_wgs(0)
        backend.sync()
        what = "%s [%s]" % (cs.what, name)
        assert rc == 0, (what, lib.last_error())
        _assert_family(cs, name)
        dw.assert_guards(what); db.assert_guards(what)
        rounded, tol = cs.tolerance(name)
        key = name.split("<")[0].split(" ")[0] + (" bf16" if rounded else " fp32")
        W_.check(what, key, dw.t.view(k, k, shp[3], Co), cs.ref[rounded], tol)
        W_.check(what, "bias", db.t, cs.gb, 1e-4)
    W_.report(backend, len(WGRAD_SHAPES))


def _partial(lib, backend, cs, ns, what):
    """one mh_conv2d_wgrad_partial launch with `ns` splits into a workspace of exactly the documented size -> (Guarded ws, Guarded db, kernel name)"""
    Co, dev = cs.shp[4], backend.device
    ws = FP.Guarded(cs.ws_floats(ns), torch.float32, dev)
    db = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
    sp = C.c_int32(ns)
    rc = lib._raw_mh_conv2d_wgrad_partial(C.byref(cs.d), ops._p(cs.xv), ops._p(cs.zv), cs.zv.ld, C.c_void_p(ws.ptr()), C.byref(sp), C.c_void_p(db.ptr()), None)
    name = lib.last_kernel().decode()
    backend.sync()
    assert rc == 0, (what, ns, lib.last_error())
    return ws, db, name


def test_wgrad_partial_reduce_sweep(backend):
    """mh_conv2d_wgrad_partial + mh_wgrad_reduce with the split count the query returns under the default heuristic and under mh_tune_wgrad_wgs(8) and
    (64): workspace of exactly splits * (taps*K*N + N) floats fully written and nothing behind it, the reduction's dw / db (db += onto zeros) against
    the oracle, two calls give the same bits (no atomics in this form)"""
    lib, dev = backend.lib, backend.device
    W_ = _Worst("mh_conv2d_wgrad_partial + mh_wgrad_reduce")
    counts = set()
    for idx, shp in enumerate(WGRAD_SHAPES):
        cs = _case(idx, dev)
        Ci, Co, k, hook = shp[3], shp[4], shp[5], shp[10]
        for wgs in (0, 8, 64):
            lib.tune_wgrad_wgs(hook + wgs)
            try:
                ns = cs.query(lib)
                runs = []
                for rep in range(2):
                    what = "%s wgs=%d splits=%d" % (cs.what, wgs, ns)
                    ws, db, name = _partial(lib, backend, cs, ns, what)
                    runs.append((ws, db))
            finally:
                lib.tune_wgrad_wgs(0)
            what += " [%s]" % name
            _assert_family(cs, name)
            assert "splits %d " % ns in name, what
            counts.add(min(ns, 3))
            for ws, db in runs:
                FP.assert_fully_written(ws, ws.n, what)
                db.assert_guards(what)
            assert torch.equal(runs[0][0].payload_bits(), runs[1][0].payload_bits()) and torch.equal(FP.bits(runs[0][1].t), FP.bits(runs[1][1].t)), what + ": two calls differ"
            ws, db = runs[0]
            dw = FP.Guarded(cs.size, torch.float32, dev)
            segs, keep = [(ws.ptr(), dw.ptr(), cs.size, ns)], []
            if ns > 1:
                assert (db.t.cpu() == 0).all(), what + ": db must not be touched when the bias partials go to the workspace"
                segs.append((ws.ptr(ns * cs.size), db.ptr(), Co, ns, 1))
            before = ws.snapshot()
            ops.wgrad_reduce(lib, segs, dev, keep)
            backend.sync()
            FP.assert_untouched(ws, before, what)
            FP.assert_fully_written(dw, cs.size, what); db.assert_guards(what)
            rounded, tol = cs.tolerance(name)
            key = name.split("<")[0].split(" ")[0] + (" bf16" if rounded else " fp32")
            W_.check(what, key, dw.t.view(k, k, Ci, Co), cs.ref[rounded], tol)
            W_.check(what, "bias", db.t, cs.gb, 1e-4)
    assert counts == {1, 2, 3}, "the list must hold single-split, two-split and many-split launches: %s" % sorted(counts)
    W_.report(backend, len(WGRAD_SHAPES))


def _groups():
    """batches of 2 .. 10 shapes of WGRAD_SHAPES (indices; a shape may appear in several batches, never twice in one), every shape in at least one"""
    r = _rng("wgrad_group")
    plain = [i for i, s in enumerate(WGRAD_SHAPES) if s[10] == 0]            # (the experiment hooks are process-wide: those shapes stay out of the batches)
    order = plain[:]
    r.shuffle(order)
    out = []
    while order:
        n = min(len(order), r.randint(2, 10))
        g, order = order[:n], order[n:]
        while len(g) < 2:
            g.append(r.choice([i for i in plain if i not in g]))
        out.append(g)
    for n in (10, 9, 2):
        out.append(r.sample(plain, n))
    return out


WGRAD_GROUPS = _groups()


def test_wgrad_partial_group_sweep(backend):
    """mh_conv2d_wgrad_partial_group over 2 .. 10 layers of the list (bf16 tiles that share one grid, the one-channel kernel, exact-fp32 layers and
    narrow tiles that go out alone): every layer's workspace -- the filter partials AND the bias partials stored behind them -- bit for bit what the
    layer's own launch stores, single-split bias gradients to 1e-4, nothing written outside; two group launches give the same bits"""
    lib, dev = backend.lib, backend.device
    grouped = 0
    for gi, group in enumerate(WGRAD_GROUPS):
        single = {}
        for idx in group:
            cs = _case(idx, dev)
            ns = cs.query(lib)
            ws, db, name = _partial(lib, backend, cs, ns, cs.what)
            _assert_family(cs, name)
            single[idx] = (ns, ws.payload_bits().clone(), db.t.cpu().clone(), name)
        runs = []
        for rep in range(2):
            items = (_ffi.WgradItem * len(group))()
            bufs = []
            for j, idx in enumerate(group):
                cs = _case(idx, dev)
                ns = single[idx][0]
                ws = FP.Guarded(cs.ws_floats(ns), torch.float32, dev)
                db = FP.Guarded(cs.shp[4], torch.float32, dev).set(torch.zeros(cs.shp[4]))
                it = items[j]
                it.d, it.inp, it.dout, it.ws, it.db, it.dout_ld, it.splits = cs.d, cs.xv.ptr, cs.zv.ptr, ws.ptr(), db.ptr(), cs.zv.ld, ns
                bufs.append((ws, db))
            rc = lib._raw_mh_conv2d_wgrad_partial_group(items, len(group), None)
            name = lib.last_kernel().decode()
            backend.sync()
            assert rc == 0, (gi, group, lib.last_error())
            runs.append(bufs)
        for j, idx in enumerate(group):
            cs = _case(idx, dev)
            ns, wbits, dbv, sname = single[idx]
            what = "group %d %s: %s splits=%d [single: %s]" % (gi, group, cs.what, ns, sname)
            ws, db = runs[0][j]
            FP.assert_fully_written(ws, ws.n, what); db.assert_guards(what)
            assert torch.equal(ws.payload_bits(), wbits), what + ": %d workspace elements differ from the single launch" % int((ws.payload_bits() != wbits).sum())
            assert torch.equal(ws.payload_bits(), runs[1][j][0].payload_bits()) and torch.equal(FP.bits(db.t), FP.bits(runs[1][j][1].t)), what + ": two group launches differ"
            if ns > 1:
                assert (db.t.cpu() == 0).all(), what
            else:
                e = (db.t.cpu().double() - cs.gb).abs().max().item()
                assert e <= 1e-4 * max(1.0, cs.gb.abs().max().item()), (what, e)
                assert (db.t.cpu() - dbv).abs().max().item() <= 1e-4 * max(1.0, cs.gb.abs().max().item()), what
        grouped += int("wgrad_group_kernel" in name)
    assert grouped >= 3, "the batches must reach the shared grid (wgrad_group_kernel): %d of %d did in their last launch" % (grouped, len(WGRAD_GROUPS))
    print("mh_conv2d_wgrad_partial_group (%s): %d batches, %d layers, bit-equal to the single launches" % (backend.name, len(WGRAD_GROUPS), sum(map(len, WGRAD_GROUPS))))


# ---- mh_wgrad_stream ----------------------------------------------------------------------------------------------------------------------------
STREAM_BUDGET = 2.5e6                    # Cin * Cout * output pixels of one layer (emulator time)


def _stream_tables():
    """[(layers [(B, H, W, Cin, Cout, dil, stride, extra floats per x row)] with H x W the OUTPUT size, target workgroups, waves)]: 14 stride-1 tables
    (dilation 1 .. 16), 12 stride-2 tables, 14 mixed ones (dilation <= 8)"""
    r = _rng("wgrad_stream")
    out = []
    for i in range(40):
        kind = "s1" if i < 14 else "s2" if i < 26 else "mixed"
        n = r.randint(1, 3) if kind != "mixed" else r.randint(2, 3)
        layers = []
        for j in range(n):
            st = {"s1": 1, "s2": 2}.get(kind, 2 if j == 0 else 1 if j == 1 else r.choice([1, 2]))
            K = r.choice([8, 9, 12, 16, 31, 32, 33, 38, 40, 64, 65, 70])
            N = r.choice([1, 1, 2, 7, 8, 16, 17, 32, 33, 40, 64, 65, 96])
            dil = 1 if st == 2 else r.choice([1, 1, 2, 3, 4, 5, 8] + ([] if kind == "mixed" else [11, 16, 16]))
            for attempt in range(200):
                B, H, W = r.randint(1, 2), r.randint(1, 30), r.randint(1, 90 // st)
                if K * N * B * H * W <= STREAM_BUDGET and (attempt > 150 or K * N * B * H * W >= STREAM_BUDGET / 40 or H * W <= 4):
                    break
            else:
                raise AssertionError("no geometry")
            layers.append((B, H, W, K, N, dil, st, r.choice([0, 0, 1, 4, 6])))
        out.append((layers, r.choice([1, 3, 8, 40, 256]), r.randint(4, 8)))
    # one-row, one-column and one-pixel outputs
    out[0][0][0] = (1, 1, 37, 32, 16, 1, 1, 0)
    out[1][0][0] = (2, 23, 1, 12, 33, 2, 1, 4)
    out[14][0][0] = (1, 1, 1, 16, 8, 1, 2, 0)
    return out


STREAM_TABLES = _stream_tables()


def _stream_run(backend, table, data):
    """shadow_cast + wgrad_stream + wgrad_reduce of one table -> ([(Guarded dw, Guarded db)], kernel name)"""
    lib, dev = backend.lib, backend.device
    layers, wgs, nw = table
    items, pairs, outs, keep = [], [], [], []
    for (B, H, W, K, N, dil, st, xpad), (x, gz) in zip(layers, data):
        xb, xv = _wide(x, K + xpad, dev)
        zd = gz.to(dev)
        xs, zs = ops.Shadow(B, H * st, W * st, K, dev), ops.Shadow(B, H, W, N, dev)
        xs.t.fill_(3.0); zs.t.fill_(3.0)                                       # stale contents: the cast must overwrite the padding channels with zeros
        pairs += [(xv, xs), (ops.view(zd) if N > 1 else ops.view(zd[..., 0].contiguous()), zs)]
        dw = FP.Guarded(9 * K * N, torch.float32, dev)
        db = FP.Guarded(N, torch.float32, dev).set(torch.zeros(N))
        items.append((xs, zs, dw.t.view(3, 3, K, N), db.t, dil))
        outs.append((dw, db)); keep += [xb, zd]
    wsa = ops.WgradWorkspace(dev); wsa.CHUNK = 1 << 20
    segs = []
    ops.shadow_cast(lib, pairs, dev, keep)
    ops.wgrad_stream(lib, lib, wsa, segs, items, dev, keep, target_wgs=wgs, nwaves=nw)
    name = lib.last_kernel().decode()
    ops.wgrad_reduce(lib, segs, dev, keep)
    backend.sync()
    return outs, name


def test_wgrad_stream_sweep(backend):
    """mh_shadow_cast + mh_wgrad_stream_plan + mh_wgrad_stream + mh_wgrad_reduce on 40 random tables of 1 .. 3 layers: stride 1 with dilation 1 .. 16,
    stride 2, mixed tables; ragged channel counts (K >= 8, N >= 1), fp32 x rows wider than K with NaN behind the channels; dw and db inside guards;
    values against the float64 oracle on bf16-rounded operands, and a second run of the table gives the same bits"""
    W_ = _Worst("mh_wgrad_stream")
    for ti, table in enumerate(STREAM_TABLES):
        layers, wgs, nw = table
        data, refs = [], []
        for li, (B, H, W, K, N, dil, st, xpad) in enumerate(layers):
            x, gz = _rand((B, H * st, W * st, K), 20000 + 10 * ti + 2 * li), _rand((B, H, W, N), 20001 + 10 * ti + 2 * li)
            w0 = torch.zeros(3, 3, K, N, dtype=torch.float64, requires_grad=True)
            (gw,) = torch.autograd.grad(T.conv2d(_bf(x).double(), w0, None, stride=st, dilation=dil, alpha=1.0), [w0], _bf(gz).double())
            data.append((x, gz)); refs.append((gw, _bf(gz).double().sum((0, 1, 2))))
        strides = set(l[6] for l in layers)
        runs = [_stream_run(backend, table, data) for rep in range(2)]
        name = runs[0][1]
        what = "table %d %s wgs=%d waves=%d [%s]" % (ti, layers, wgs, nw, name)
        want = "wgrad_stream_mixed_kernel layers %d" % len(layers) if len(strides) == 2 else ",s%d> layers %d" % (strides.pop(), len(layers))
        assert want in name and "wgrad_stream" in name, what
        for li, ((dw, db), (dw2, db2), (gw, gb)) in enumerate(zip(runs[0][0], runs[1][0], refs)):
            lw = "%s layer %d" % (what, li)
            FP.assert_fully_written(dw, dw.n, lw); db.assert_guards(lw)
            assert torch.equal(dw.payload_bits(), dw2.payload_bits()) and torch.equal(FP.bits(db.t), FP.bits(db2.t)), lw + ": two runs differ"
            W_.check(lw, name.split("<")[0].split(" ")[0] + " filter", dw.t.view(gw.shape), gw, 2e-5)
            W_.check(lw, name.split("<")[0].split(" ")[0] + " bias", db.t, gb, 1e-4)
    W_.report(backend, len(STREAM_TABLES))
