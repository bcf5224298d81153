"""The packing of every plan op kind (mh_op: kind, i[27], f[4], p[12], n) is byte for byte what tests/golden/plan_packing.json records.

The fixture was written by `python tests/test_plan_packing.py` on the commit BEFORE the field layout moved into madnet_hip/oplayout.py, when every
Recorder method still packed positional lists by hand: `produce()` below runs on both sides of that change because the Recorder call surface
(names and argument order of _ffi.Lib) is the same.  It is a recording, not an expectation derived from the table: regenerate it only for a
deliberate change of the packing (together with run_op() of csrc/lib.hip and MH_ABI_VERSION).

Sentinels: argument k of a call is the integer 1000 + k, the pointer 0x10000 * (k + 1) or the float k + 0.5, by its type in _ffi.SIGNATURES; a
descriptor has every field different.  No library and no GPU are needed: nothing is launched."""
import ctypes as C
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_packing.json")

# not op-recording: bookkeeping of the recorder itself
NOT_OPS = {"note_refs", "cut", "tally_wgrad", "compile", "compile_parts"}


def _conv_desc(_ffi):
    d = _ffi.ConvDesc()
    for k, (name, typ) in enumerate(_ffi.ConvDesc._fields_):
        setattr(d, name, 0.25 + k if typ is C.c_float else 101 + k)
    return d


def _head_desc(_ffi):
    d = _ffi.HeadBwdDesc()
    for k, (name, typ) in enumerate(_ffi.HeadBwdDesc._fields_):
        setattr(d, name, 0.25 + k if typ is C.c_float else 201 + k)
    return d


def _sentinels(_ffi, name):
    """one value per argument of mh_<name>, by its declared type"""
    out = []
    for k, t in enumerate(_ffi.SIGNATURES["mh_" + name][1]):
        if t is C.c_void_p:
            out.append(0x10000 * (k + 1))
        elif t is C.c_float:
            out.append(k + 0.5)
        elif t in (C.c_int32, C.c_int64):
            out.append(1000 + k)
        elif t is C.POINTER(_ffi.ConvDesc):
            out.append(C.byref(_conv_desc(_ffi)))
        elif t is C.POINTER(_ffi.HeadBwdDesc):
            out.append(C.byref(_head_desc(_ffi)))
        elif t is C.POINTER(C.c_int32):
            out.append(C.byref(C.c_int32(1000 + k)))
        elif t in (C.POINTER(C.c_void_p), C.POINTER(C.c_int64)):
            out.append(None)            # the counted tails: every call that has one supplies its arrays (_tail)
        else:
            raise AssertionError("no sentinel for argument %d of mh_%s (%r)" % (k, name, t))
    return out


def _tail(n, k0):
    """the counted tail of allreduce_sum / fetch_inputs: n pointers and n counts as ctypes arrays"""
    return (C.c_void_p * n)(*[0x10000 * (k0 + 1) + 0x100 * (j + 1) for j in range(n)]), (C.c_int64 * n)(*[1000 + k0 + 10 * (j + 1) for j in range(n)])


def _calls(_ffi):
    """[(label, method name, {argument name: value} overriding the sentinel, recorder state)]"""
    calls = []
    for sh_in in (False, True):
        for sh_mask in (False, True):
            for flags in (0, 1):
                over = {"bias": None, "flags": flags}
                if not sh_in:
                    over["in_shadow"] = None
                if not sh_mask:
                    over["mask_shadow"] = None
                calls.append(("conv2d_sh3[in=%d,mask=%d,flags=%d]" % (sh_in, sh_mask, flags), "conv2d_sh3", over, None))
    for n in (1, _ffi.ALLREDUCE_MAX_BUFS):
        bufs, counts = _tail(n, 0)
        calls.append(("allreduce_sum[%d]" % n, "allreduce_sum", {"bufs": bufs, "counts": counts, "n": n}, None))
    for n in (1, _ffi.FETCH_MAX):
        dst, counts = _tail(n, 1)
        calls.append(("fetch_inputs[%d]" % n, "fetch_inputs", {"dst": dst, "counts": counts, "n": n}, None))
    calls.append(("conv2d_wgrad_partial[ws=None]", "conv2d_wgrad_partial", {"ws": None}, None))
    calls.append(("conv2d_planes[precision=1]", "conv2d_planes", {"precision": 1}, None))
    calls.append(("fill[lane 2, join, lane mask, nodefer]", "fill", {}, dict(lane=2, join_next=True, join_lanes_next=0b10110, nodefer=True)))
    calls.append(("fill[lane 0, nodefer]", "fill", {}, dict(nodefer=True)))
    calls.append(("warp_fwd[lane 4]", "warp_fwd", {}, dict(lane=4)))
    return calls


def produce():
    """[{"call", "kind", "i", "f", "p", "n"}]: every op-recording Recorder method once with sentinel arguments, then the variants of _calls()"""
    from madnet_hip import _ffi
    from madnet_hip.plan import Recorder
    names = sorted(n for n, f in inspect.getmembers(Recorder, inspect.isfunction) if not n.startswith("_") and n not in NOT_OPS)
    calls = [(n, n, {}, None) for n in names if n not in ("conv2d_sh3", "allreduce_sum", "fetch_inputs")] + _calls(_ffi)
    out = []
    for label, name, over, state in calls:
        params = list(inspect.signature(getattr(Recorder, name)).parameters)[1:]
        args = _sentinels(_ffi, name)
        assert len(args) == len(params), name
        over = dict(over)
        if "precision" in over and "precision" not in params:        # a field of the descriptor
            d = _conv_desc(_ffi); d.precision = over.pop("precision")
            args[0] = C.byref(d)
        for k, v in over.items():
            args[params.index(k)] = v
        r = Recorder()
        for k, v in (state or {}).items():
            setattr(r, k, v)
        getattr(r, name)(*args)
        assert len(r.ops) == 1, label
        o = r.ops[0]
        out.append({"call": label, "kind": int(o.kind), "i": [int(v) for v in o.i], "f": [float(v) for v in o.f], "p": [int(v or 0) for v in o.p], "n": int(o.n)})
    return out


def test_packing_matches_the_recorded_fixture():
    got = produce()
    want = json.load(open(GOLDEN))
    assert [g["call"] for g in got] == [w["call"] for w in want]
    for g, w in zip(got, want):
        assert (g["kind"], tuple(g["i"]), tuple(g["f"]), tuple(g["p"]), g["n"]) == (w["kind"], tuple(w["i"]), tuple(w["f"]), tuple(w["p"]), w["n"]), g["call"]


def test_every_kind_of_the_table_is_produced():
    from madnet_hip import _ffi, oplayout
    made = {g["kind"] for g in produce()}
    assert made == set(oplayout.LAYOUT) - {_ffi.OP_RESERVED_25}


def test_table_kinds_are_the_ffi_constants():
    from madnet_hip import _ffi, oplayout
    consts = {n: v for n, v in vars(_ffi).items() if n.startswith("OP_") and n not in ("OP_JOIN", "OP_NODEFER")}
    assert {"OP_" + L.name: k for k, L in oplayout.LAYOUT.items()} == consts
    assert len(consts) == 41 and sorted(consts.values()) == list(range(1, 42))


def test_recorder_and_library_take_the_same_arguments():
    from madnet_hip import _ffi
    from madnet_hip.plan import Recorder
    both = [n for n, f in inspect.getmembers(Recorder, inspect.isfunction) if "mh_" + n in _ffi.SIGNATURES]
    assert len(both) >= 50
    for n in both:
        assert len(inspect.signature(getattr(Recorder, n)).parameters) - 1 == len(_ffi.SIGNATURES["mh_" + n][1]), n
    assert {n for n, f in inspect.getmembers(Recorder, inspect.isfunction) if not n.startswith("_")} - set(both) == NOT_OPS


def test_pack_refuses_an_int_that_does_not_fit_its_slot():
    """mh_fetch_inputs / mh_allreduce_sum take int64 counts, the record carries them in int32 slots: a count of 2^32 + 5 used to be recorded as 5 (ctypes
    stores the low bits without a word) and the replay moved 5 elements where the direct call moved 2^32 + 5.  The error names kind and slot."""
    import pytest
    from madnet_hip import _ffi
    from madnet_hip.plan import Recorder
    for bad in (1 << 31, (1 << 32) + 5, -(1 << 31) - 1):
        dst, counts = _tail(2, 1)
        counts[1] = bad
        with pytest.raises(ValueError, match=r"FETCH_INPUTS: count1 = %d .*i\[2\]" % bad):
            Recorder().fetch_inputs(0x10000, dst, counts, 2, None)
        bufs, counts = _tail(3, 0)
        counts[0] = bad
        with pytest.raises(ValueError, match=r"ALLREDUCE: count0 = %d .*i\[1\]" % bad):
            Recorder().allreduce_sum(bufs, counts, 3, 0x10000, None)
        with pytest.raises(ValueError, match=r"WARP_FWD: W = %d .*i\[4\]" % bad):
            Recorder().warp_fwd(0x10000, 4, 0x20000, 0x30000, 4, 1, 2, bad, 4, None)
        r = Recorder()
        with pytest.raises(ValueError):
            r.copy_channels(0x10000, bad, 0x20000, 4, 10, 2, 1.0, 0, None)
        assert r.ops == []                      # nothing half-recorded


def test_pack_keeps_the_int32_limits_and_the_bit_cast_grad_scale():
    """the two ends of the range go in as they are; adam's grad_scale travels as a SIGNED 32-bit pattern (negative for a negative scale) and comes back
    bit for bit"""
    import struct
    from madnet_hip import oplayout
    from madnet_hip.plan import Recorder
    for v in (-(1 << 31), (1 << 31) - 1, -1, 0):
        dst, counts = _tail(1, 1)
        counts[0] = v
        r = Recorder()
        r.fetch_inputs(0x10000, dst, counts, 1, None)
        assert oplayout.fields(r.ops[0]).count0 == v
    for gs in (-0.5, 1.0, -3.0e38, 1e-45, float("inf"), -0.0):
        r = Recorder()
        r.adam(0x10000, 0x20000, 0x30000, 0x40000, 77, 0x50000, 1e-3, 0.9, 0.999, 1e-8, gs, None)
        bits_ = oplayout.fields(r.ops[0]).gs_bits
        assert struct.pack("<i", bits_) == struct.pack("<f", gs), gs


if __name__ == "__main__":
    open(GOLDEN, "w").write("[\n" + ",\n".join(json.dumps(rec, separators=(",", ":")) for rec in produce()) + "\n]\n")
