"""The scheduling rules of plan_run_impl (csrc/lib.hip): side lanes, deferred side-lane launches and their flushes, MH_OP_JOIN, the lane-mask joins,
MH_OP_NODEFER, the batches of consecutive partial filter gradients, the error path; eagerly on both backends and as a captured hipGraph on the MI355X.

The plans are built from fill, momentum and copy_channels (elementwise, order-deterministic, swept in test_shape_sweep.py) and, for the batches, from the
small filter-gradient layers of test_conv_parity.py.  A scenario is a function that issues its ops to a target: the library (the direct calls, in program
order on the caller's stream: the expected values) or a plan.Recorder (the same calls with lanes and joins set).  Every buffer is a footprint.Guarded
allocation; a replay is compared with the direct run over the WHOLE allocation, guards included, on bits.  The only tolerance is the bias gradient of the
filter-gradient batches (fp32 atomics across workgroups): the 1e-4 of test_wgrad_partial_group_matches_single_launches.

What the ordering scenarios (test_fork_edge_and_joins) can and cannot show.  The producer is a momentum update over PRODUCER_N = 1 << 25 elements
(640 MB of traffic), measured on the MI355X with mh_event_* around the direct call: 134.1 and 116.5 us in two runs; 1 << 24 took 51.3 us, too close to the
50 us wanted (several times the 15-20 us cross-queue hop plan_run_impl's comment records), so the size was doubled.  The consumer on a side lane reads the LAST 1024 elements the producer writes, so a consumer that started early
would PROBABLY read old values and the test would fail: without the fork edge or a join the test is likely, not certain, to fail, and a pass does not
prove the ordering -- it is evidence only.  On the CPU emulator launches run to completion in issue order and a deferred op is issued after the next
lane-0 op: there the scenarios check that the plans are legal in issue order (every op finds its inputs written), nothing about streams.
"""
import ctypes as C

import pytest
import torch

import footprint as FP
from madnet_hip import _ffi, ops, plan as PL

LANES = _ffi.MAX_LANES
PRODUCER_N = 1 << 25            # elements of the producer of test_fork_edge_and_joins on the MI355X: 117 .. 134 us measured (the test prints it)
EMUL_PRODUCER_N = 1 << 15       # the emulator runs launches to completion in issue order: size adds nothing there
TAIL = 1024


def _P(g, off=0):
    return C.c_void_p(g.ptr(off))


def _lane(tgt, lane=0, join=False, mask=0, nodefer=False):
    """scheduling state of the op issued next (a direct call has none)"""
    if isinstance(tgt, PL.Recorder):
        tgt.lane, tgt.join_next, tgt.join_lanes_next, tgt.nodefer = lane, join, mask, nodefer


_values = {}


def _buf(dev, n, seed=None, scale=1.0):
    g = FP.Guarded(n, torch.float32, dev)
    if seed is not None:
        if (n, seed) not in _values:          # (drawn once: the producer's 2^24 elements are made several times)
            _values[(n, seed)] = torch.randn(n, generator=torch.Generator().manual_seed(seed))
        g.set(_values[(n, seed)] * scale if scale != 1.0 else _values[(n, seed)])
    return g


def _ibits(g):
    return g.all.view(torch.int32)


def _assert_same(got, want, what):
    """every allocation of the two states equal on bits, guards included (compared where the buffers live)"""
    assert list(got) == list(want)
    for name in want:
        a, b = _ibits(got[name]), _ibits(want[name])
        assert torch.equal(a, b), "%s: buffer %s differs from the direct calls in %d elements (first at %d of [guard %d | %d | guard])" % (
            what, name, int((a != b).sum()), int((a != b).nonzero()[0]), want[name].guard, want[name].n)


class Scenario(object):
    """make(dev) -> {name: Guarded} (the same bits every time); prog(tgt, st, lib, dev, keep): issue the ops; check(st): properties of the direct result"""

    def __init__(self, name, make, prog, check=None, nops=None, loose=()):
        self.name, self.make, self.prog, self.check, self.nops, self.loose = name, make, prog, check, nops, loose


def _direct(backend, sc):
    st, keep = sc.make(backend.device), []
    sc.prog(backend.lib, st, backend.lib, backend.device, keep)
    backend.sync()
    for name, g in st.items():
        g.assert_guards("%s direct %s" % (sc.name, name))
    if sc.check:
        sc.check(st)
    return st


def _record(backend, sc, st, keep):
    rec = PL.Recorder()
    sc.prog(rec, st, backend.lib, backend.device, keep)
    plan = rec.compile()
    assert sc.nops is None or plan.n == sc.nops, (sc.name, plan.n)
    return plan


def _compare(sc, got, want, what):
    strict = {k: v for k, v in want.items() if k not in sc.loose}
    _assert_same({k: got[k] for k in strict}, strict, what)
    for name in sc.loose:             # bias gradients of the filter-gradient batches: fp32 atomics across workgroups
        got[name].assert_guards(what)
        a, b = got[name].t.cpu(), want[name].t.cpu()
        assert torch.isfinite(a).all() and (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item()), (what, name)


def _eager(backend, sc):
    want = _direct(backend, sc)
    st, keep = sc.make(backend.device), []
    plan = _record(backend, sc, st, keep)
    plan.run(backend.lib, None)
    backend.sync()
    _compare(sc, st, want, "%s (%s, eager plan)" % (sc.name, backend.name))
    return want


def _captured(hip, sc):
    """the plan as a captured hipGraph on a stream of its own, launched twice from the same initial state: both results equal the direct calls"""
    want = _direct(hip, sc)
    st, keep = sc.make(hip.device), []
    first = {k: g.all.clone() for k, g in st.items()}
    plan = _record(hip, sc, st, keep)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.capture(hip.lib, s.cuda_stream)
        s.synchronize()
        for k, g in st.items():               # (capturing launches nothing)
            assert torch.equal(_ibits(g), first[k].view(torch.int32)), (sc.name, k)
        for turn in range(2):
            for k, g in st.items():
                g.all.copy_(first[k])
            s.synchronize()
            plan.launch(hip.lib, s.cuda_stream)
            s.synchronize()
            _compare(sc, st, want, "%s (captured graph, launch %d)" % (sc.name, turn))


# ---- 1. nothing is lost: 70 deferred side-lane fills (the flush at 60, the final flush, the final join) --------------------------------------------
def _fills(middle, count=70):
    """middle: None | 'lane0' | 'join' -- one lane-0 op after the 35th fill, with join_next or without"""
    def make(dev):
        st = {"b%02d" % k: _buf(dev, 5 + k) for k in range(count)}
        st["mid"] = _buf(dev, 9)
        return st

    def prog(tgt, st, lib, dev, keep):
        for k in range(count):
            if middle and k == 35:
                _lane(tgt, 0, join=(middle == "join"))
                tgt.fill(_P(st["mid"]), 9, -3.5, None)
            _lane(tgt, 1 + k % (LANES - 1))
            tgt.fill(_P(st["b%02d" % k]), 5 + k, 0.25 * (k + 1), None)

    def check(st):
        for k in range(count):
            assert bool((st["b%02d" % k].t == 0.25 * (k + 1)).all()), k
        assert bool((st["mid"].t == -3.5).all()) == bool(middle)

    return Scenario("%d side-lane fills, middle=%s" % (count, middle), make, prog, check, nops=count + bool(middle))


# 300: five times the flush threshold -- a list that is never flushed runs far past its 64 entries (70 run past it by six, which need not show)
FILLS = [_fills(None), _fills("lane0"), _fills("join"), _fills(None, count=300)]


# ---- 2. a lane keeps its order: six momentum updates of one variable, deferred and at once in turn ---------------------------------------------------
MOMENTA = [(1e-2, 0.9, 0.5), (3e-2, 0.5, 1.0), (5e-3, 0.7, 2.0), (2e-2, 0.3, 0.25), (7e-3, 0.8, 1.5), (1e-3, 0.6, 3.0)]       # (lr, mom, gs): no two alike


def _order(middle, lane=3, tag=0):
    n = 1001

    def make(dev):
        return {"var": _buf(dev, n, 11 + tag), "accum": _buf(dev, n, 12 + tag), "grad": _buf(dev, n, 13 + tag), "mid": _buf(dev, 7)}

    def prog(tgt, st, lib, dev, keep):
        for k, (lr, mom, gs) in enumerate(MOMENTA):
            if middle and k == 3:
                _lane(tgt, 0)
                tgt.fill(_P(st["mid"]), 7, 4.0, None)
            _lane(tgt, lane, nodefer=(k % 2 == 0))
            tgt.momentum(_P(st["var"]), _P(st["accum"]), _P(st["grad"]), n, lr, mom, gs, None)

    def check(st):
        assert torch.isfinite(st["var"].t).all() and torch.isfinite(st["accum"].t).all()

    return Scenario("six momentum updates on lane %d, middle=%s" % (lane, middle), make, prog, check, nops=6 + bool(middle))


ORDER = [_order(False), _order(True)]


def test_lane_order_matters_for_the_chosen_parameters():
    """host only: the six (lr, mom, gs) are pairwise different in every component, so two updates that change places change the result"""
    for c in range(3):
        assert len({m[c] for m in MOMENTA}) == len(MOMENTA)


# ---- 3. fork edge and joins -----------------------------------------------------------------------------------------------------------------------------
def _chain(form, n):
    """form 'a': lane-0 producer, lane-2 consumer of its last TAIL elements, lane-0 reader behind join_next; 'b': the reader joins lane 2 by mask, lane 3
    carries an independent fill; 'c': a lane-4 op joins lane 2 into its own lane, lane 0 then joins lane 4"""
    def make(dev):
        st = {"var": _buf(dev, n, 21), "accum": _buf(dev, n, 22), "grad": _buf(dev, n, 23), "copy": _buf(dev, TAIL), "final": _buf(dev, TAIL)}
        if form == "b":
            st["side"] = _buf(dev, 333)
        if form == "c":
            st["mid"] = _buf(dev, TAIL)
        return st

    def prog(tgt, st, lib, dev, keep):
        _lane(tgt, 0)
        tgt.momentum(_P(st["var"]), _P(st["accum"]), _P(st["grad"]), n, 1e-2, 0.9, 0.5, None)
        _lane(tgt, 2)
        tgt.copy_channels(_P(st["var"], n - TAIL), 1, _P(st["copy"]), 1, TAIL, 1, 1.0, 0, None)
        if form == "a":
            _lane(tgt, 0, join=True)
            tgt.copy_channels(_P(st["copy"]), 1, _P(st["final"]), 1, TAIL, 1, 2.0, 0, None)
        elif form == "b":
            _lane(tgt, 3)
            tgt.fill(_P(st["side"]), 333, 6.5, None)
            _lane(tgt, 0, mask=1 << 2)
            tgt.copy_channels(_P(st["copy"]), 1, _P(st["final"]), 1, TAIL, 1, 2.0, 0, None)
        else:
            _lane(tgt, 4, mask=1 << 2)
            tgt.copy_channels(_P(st["copy"]), 1, _P(st["mid"]), 1, TAIL, 1, 3.0, 0, None)
            _lane(tgt, 0, mask=1 << 4)
            tgt.copy_channels(_P(st["mid"]), 1, _P(st["final"]), 1, TAIL, 1, 2.0, 0, None)

    def check(st):
        f = st["final"].t.cpu()
        assert torch.isfinite(f).all() and f.unique().numel() > TAIL // 2
        assert torch.equal(f, st["var"].t[n - TAIL:].cpu() * (6.0 if form == "c" else 2.0))
        if form == "b":
            assert bool((st["side"].t == 6.5).all())

    return Scenario("producer / side-lane consumer / join, form %s, n=%d" % (form, n), make, prog, check, nops={"a": 3, "b": 4, "c": 4}[form])


def _producer_time(hip, n):
    """microseconds of the direct producer call alone (mh_event_* around it, the second of two calls)"""
    st = _chain("a", n).make(hip.device)
    e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    hip.lib.event_create(C.byref(e0)); hip.lib.event_create(C.byref(e1))
    for _ in range(2):
        hip.lib.event_record(e0, None)
        hip.lib.momentum(_P(st["var"]), _P(st["accum"]), _P(st["grad"]), n, 1e-2, 0.9, 0.5, None)
        hip.lib.event_record(e1, None)
        hip.sync()
        hip.lib.event_elapsed_ms(e0, e1, C.byref(ms))
    hip.lib.event_destroy(e0); hip.lib.event_destroy(e1)
    return 1e3 * ms.value


# ---- 4. batches of partial filter gradients: 35 consecutive ops of one lane go out as 16 + 16 + 3 --------------------------------------------------
# (H, W, Cin, Cout, stride, dil, precision): small bf16 layers in the manner of test_conv_parity.py's GROUP_LAYERS, odd sizes and the Cout = 1 reduction
# included (all take the grouped grid: test_batch_layers_take_the_grouped_grid), and its exact-fp32 layer, which goes out alone
SMALL = [(6, 10, 64, 32, 1, 1, 1), (6, 10, 32, 64, 1, 1, 1), (5, 7, 32, 32, 1, 1, 1), (12, 20, 32, 1, 1, 1, 1)]
EXACT = (12, 20, 16, 32, 1, 1, 0)
BATCH_LAYERS = [EXACT if k == 9 else SMALL[k % len(SMALL)] for k in range(35)]


def _wgrads(lane_change):
    """35 consecutive WGRAD_PARTIAL ops on lane 1 (lane_change: the last 15 on lane 2), one wgrad_reduce on lane 0 behind a join"""
    def make(dev):
        st = {}
        for li, (H, W, Ci, Co, s, d, prec) in enumerate(BATCH_LAYERS):
            Ho, Wo, _, _ = ops.conv_geometry(H, W, 3, 3, s, d)
            st["x%02d" % li] = _buf(dev, H * W * Ci, 100 + li)
            st["z%02d" % li] = _buf(dev, Ho * Wo * Co, 200 + li)
            st["dw%02d" % li] = _buf(dev, 9 * Ci * Co)
            st["db%02d" % li] = FP.Guarded(Co, torch.float32, dev).set(torch.zeros(Co))
        return st

    def prog(tgt, st, lib, dev, keep):
        wsa = ops.WgradWorkspace(dev); wsa.CHUNK = 1 << 20
        keep.append(wsa)
        segs = []
        for li, (H, W, Ci, Co, s, d, prec) in enumerate(BATCH_LAYERS):
            Ho, Wo, _, _ = ops.conv_geometry(H, W, 3, 3, s, d)
            xv = ops.View(st["x%02d" % li].t.view(1, H, W, Ci), 1, H, W, Ci, Ci)
            zv = ops.View(st["z%02d" % li].t.view(1, Ho, Wo, Co), 1, Ho, Wo, Co, Co)
            _lane(tgt, 2 if (lane_change and li >= 20) else 1)
            ops.PRECISION = ops.PRECISION_BWD = prec
            try:
                ops.conv2d_wgrad_partial(tgt, lib, wsa, segs, xv, zv, st["dw%02d" % li].t.view(3, 3, Ci, Co), st["db%02d" % li].t, stride=s, dil=d)
            finally:
                ops.PRECISION, ops.PRECISION_BWD = 0, None
        _lane(tgt, 0, join=True)
        ops.wgrad_reduce(tgt, segs, dev, keep)

    def check(st):
        for li in range(len(BATCH_LAYERS)):
            dw = st["dw%02d" % li].t.cpu()
            assert torch.isfinite(dw).all() and dw.unique().numel() > dw.numel() // 2, li

    return Scenario("35 partial filter gradients, lane change=%s" % lane_change, make, prog, check, nops=36, loose=["db%02d" % li for li in range(35)])


WGRADS = [_wgrads(False), _wgrads(True)]


def test_batch_layers_take_the_grouped_grid(backend):
    """every bf16 layer of BATCH_LAYERS is eligible for the grouped grid: two items of it in one mh_conv2d_wgrad_partial_group call note the grouped kernel"""
    lib, dev = backend.lib, backend.device
    for a, b in [(l, l) for l in SMALL]:
        items = (_ffi.WgradItem * 2)()
        keep = []
        for it, (H, W, Ci, Co, s, d, prec) in zip(items, (a, b)):
            Ho, Wo, pt, pl = ops.conv_geometry(H, W, 3, 3, s, d)
            x, z = torch.zeros(1, H, W, Ci, device=dev), torch.zeros(1, Ho, Wo, Co, device=dev)
            it.d = ops.conv_desc(1, H, W, Ho, Wo, Ci, Co, 3, 3, s, d, pt, pl, 0, 0, Ci, Co, precision=prec)
            sp = C.c_int32(0)
            lib.conv2d_wgrad_partial(C.byref(it.d), ops._p(x), ops._p(z), Co, None, C.byref(sp), None, None)
            ws = torch.zeros(9 * Ci * Co * sp.value + Co * sp.value, device=dev)
            it.inp, it.dout, it.ws, it.db, it.dout_ld, it.splits = x.data_ptr(), z.data_ptr(), ws.data_ptr(), None, Co, sp.value
            keep += [x, z, ws]
        lib.conv2d_wgrad_partial_group(items, 2, None)
        backend.sync()
        assert lib.last_kernel().decode().startswith("wgrad_group_kernel layers 2"), (a, b, lib.last_kernel())


# ---- the eager runs, both backends ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", FILLS, ids=lambda s: s.name)
def test_nothing_is_lost(backend, sc):
    _eager(backend, sc)


@pytest.mark.parametrize("sc", ORDER, ids=lambda s: s.name)
def test_a_lane_keeps_its_order(backend, sc):
    want = _eager(backend, sc)
    # the order is observable: the same six updates backwards give other bits
    st = sc.make(backend.device)
    for lr, mom, gs in reversed(MOMENTA):
        backend.lib.momentum(_P(st["var"]), _P(st["accum"]), _P(st["grad"]), 1001, lr, mom, gs, None)
    backend.sync()
    assert not torch.equal(_ibits(st["var"]), _ibits(want["var"]))


@pytest.mark.parametrize("form", ["a", "b", "c"])
def test_fork_edge_and_joins(backend, form):
    """see the module docstring for what this can show"""
    n = PRODUCER_N if backend.name == "hip" else EMUL_PRODUCER_N
    if backend.name == "hip" and form == "a":
        us = _producer_time(backend, n)
        print("producer mh_momentum over %d elements: %.1f us" % (n, us))
        assert us >= 50.0, "the producer (%.1f us) is too short for a missing edge to show: raise PRODUCER_N" % us
    _eager(backend, _chain(form, n))


@pytest.mark.parametrize("sc", WGRADS, ids=lambda s: s.name)
def test_partial_filter_gradient_batches(backend, sc):
    _eager(backend, sc)
    if not sc.name.endswith("True"):
        return
    # the uninterrupted and the lane-changed plan batch differently (16 + 16 + 3 against 16 + 4 | 15): same partial sums
    a, b = sc.make(backend.device), WGRADS[0].make(backend.device)
    ka, kb = [], []
    _record(backend, sc, a, ka).run(backend.lib, None)
    _record(backend, WGRADS[0], b, kb).run(backend.lib, None)
    backend.sync()
    _compare(sc, a, b, "lane change against uninterrupted")


# ---- 5. error path (eager only) -----------------------------------------------------------------------------------------------------------------------
def test_a_refused_op_names_its_index_and_the_stream_stays_usable(backend):
    """op 1 is a momentum update over 0 elements (refused: test_error_paths.py) behind a deferred side-lane fill: mh_plan_run returns that entry's code,
    the message names the op, and a valid plan on the same stream then gives the right result.  Whether the deferred fill ran is left open."""
    lib, dev = backend.lib, backend.device
    a, v = _buf(dev, 64), _buf(dev, 64, 5)
    rec = PL.Recorder()
    _lane(rec, 1)
    rec.fill(_P(a), 64, 1.5, None)
    _lane(rec, 0)
    rec.momentum(_P(v), _P(v), _P(v), 0, 1e-4, 0.9, 1.0, None)
    bad = rec.compile()
    rc = getattr(lib, "_raw_mh_plan_run")(bad.arr, bad.n, None)
    assert rc == -1, rc
    assert ("plan op 1 (kind %d)" % _ffi.OP_MOMENTUM) in lib.last_error().decode(), lib.last_error()
    backend.sync()
    _eager(backend, ORDER[1])
    a.assert_guards("fill in front of the refused op"); v.assert_guards("refused momentum")


# ---- 6. captured graph = eager replay (MI355X only) -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sc", FILLS + ORDER + WGRADS, ids=lambda s: s.name)
def test_captured_graph_equals_the_direct_calls(hip, sc):
    _captured(hip, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["a", "b", "c"])
def test_captured_fork_edge_and_joins(hip, form):
    _captured(hip, _chain(form, PRODUCER_N))


def _multiplan(backend, scs):
    want = [_direct(backend, sc) for sc in scs]
    sts, keep = [sc.make(backend.device) for sc in scs], []
    first = [{k: g.all.clone() for k, g in st.items()} for st in sts]
    return want, sts, first, keep, PL.MultiPlan([_record(backend, sc, st, keep) for sc, st in zip(scs, sts)])


def test_multiplan_of_three_order_plans(backend):
    """mh_plans_run, eagerly: three copies of the lane-order plan on lanes 1 .. 3 (at most MH_MAX_LANES - 2: the last lane is the branch stream), each on
    buffers of its own and, from the second on, with a lane set of its own (plan_run_impl's `fixed`): every plan ends where it ends alone.
    NOT captured: the side lane of a plan that itself runs on a branch stream -- a fork inside a forked branch -- records fine and then crashes
    hipStreamEndCapture / hipGraphInstantiate on this ROCm (profiles/r03_experiments.txt #15; met again when this test was first written as a captured
    graph), which is why the engines give every branch a serial chain.  The captured form is test_captured_multiplan_of_three_serial_plans."""
    scs = [_order(True, lane=1 + k, tag=10 * k) for k in range(3)]
    assert all(1 + k <= LANES - 2 for k in range(3))
    want, sts, _, keep, mp = _multiplan(backend, scs)
    mp.run(backend.lib, None)
    backend.sync()
    for sc, st, w in zip(scs, sts, want):
        _compare(sc, st, w, "%s (MultiPlan, eager, %s)" % (sc.name, backend.name))


@pytest.mark.gpu
def test_captured_multiplan_of_three_serial_plans(hip):
    """three copies of the six-update plan as parallel branches of ONE captured graph, every chain serial on its branch (lane 0: see
    test_multiplan_of_three_order_plans), launched twice from the same state: every branch ends where its plan ends alone"""
    scs = [_order(True, lane=0, tag=10 * k) for k in range(3)]
    want, sts, first, keep, mp = _multiplan(hip, scs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mp.capture(hip.lib, s.cuda_stream)
        for turn in range(2):
            for st, f in zip(sts, first):
                for k, g in st.items():
                    g.all.copy_(f[k])
            s.synchronize()
            mp.launch(hip.lib, s.cuda_stream)
            s.synchronize()
            for sc, st, w in zip(scs, sts, want):
                _compare(sc, st, w, "%s (MultiPlan, launch %d)" % (sc.name, turn))
