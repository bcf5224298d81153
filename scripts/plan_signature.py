"""Signature of the recorded plans: per op its kind, integer / float fields (the lane / join / no-defer word i[26] included), n, and which pointer
slots are set and which of them alias (pointer VALUES replaced by their rank of first appearance in the plan), plus the work statistics and the
elided stores.  One line per (engine, configuration, build_plan call): two commits record the same steps when their outputs are equal line for line.
CPU only (tests/emul/libmadnet_emul.so).  usage: plan_signature.py [H W]   (default: 128 256 and 375 1242)"""
import dataclasses
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-self-adaptive-deep-stereo_amd")
sys.path[:0] = [ROOT, PKG]
from madnet_hip import _ffi, ops, engine as E, dispnet_engine as DE      # noqa: E402
from madnet_hip.schedule import Schedule, DispNetSchedule                # noqa: E402

FLIPS = ("SIDE_LOSS", "ONE_FILL", "FUSE_BACK", "HEAD_IN_FRONT", "IMAGE_CONV", "EARLY_UPDATE", "USE_PLANES", "FUSE_SPLITS", "PLANES_DGRAD", "SHADOW_DGRAD", "FUSE_HEAD")
DN_FLIPS = ("EARLY_UPDATE", "PRODUCER_SHADOWS", "PLANES_S2", "DETERMINISTIC")


def signature(plans):
    """(number of ops, hash) of a plan or of the list of plans build_plan(part='grad_split') returns"""
    rank, rows = {}, []
    rk = lambda q: -1 if not q else rank.setdefault(int(q), len(rank))
    for plan in (plans if isinstance(plans, list) else [plans]):
        for k in range(plan.n):
            o = plan.arr[k]
            rows.append((o.kind, tuple(o.i), tuple(float(x) for x in o.f), tuple(rk(q) for q in o.p), int(o.n)))
        rows.append((sorted(plan.stats.items()), sorted(plan.work.items()), [(rank.get(int(a), "new"), int(nb)) for a, nb in plan.elided]))
    return sum(1 for row in rows if len(row) == 5), hashlib.sha256(repr(rows).encode()).hexdigest()[:16]


def block_vars(layers):
    """variable names of a block of block_config/MadNet_*.json (the layer names of Nets/MadNet.py)"""
    out = []
    for layer in layers:
        m = re.match(r"fgc-volume-filtering-(\d)/disp(\d)$|left/conv(\d+)$|context(\d)$", layer)
        base = E.est_name(int(m.group(1)), int(m.group(2))) if m.group(1) else (E.pyr_name(int(m.group(3))) if m.group(3) else E.ctx_name(int(m.group(4))))
        out += [base + "/weights", base + "/biases"]
    return out


def main(H, W):
    lib = _ffi.Lib(os.path.join(ROOT, "tests", "emul", "libmadnet_emul.so"))
    lib.ensure_init()
    cfgs = {f[7:-5]: json.load(open(os.path.join(PKG, "block_config", f))) for f in ("MadNet_full.json", "MadNet_piramid_only.json")}

    def show(*tag_and_plan):
        print("%dx%d" % (H, W), *(tag_and_plan[:-1] + signature(tag_and_plan[-1])))
        sys.stdout.flush()

    def madnet(tag, prec, setup=None, B=1, full_only=True, **kw):
        eng = E.MadNetEngine(lib, H, W, B=B, device="cpu", precision=prec, **kw)
        if setup:
            setup(eng)
        show("madnet", prec, tag, "FULL", eng.build_plan("FULL", lr=1e-4))
        if not full_only:
            show("madnet", prec, tag, "FULL again", eng.build_plan("FULL", lr=1e-4))
            show("madnet", prec, tag, "NONE", eng.build_plan("NONE"))
            for part in ("grad", "grad_split", "update"):
                show("madnet", prec, tag, "FULL " + part, eng.build_plan("FULL", lr=1e-4, part=part))
            show("madnet", prec, tag, "FULL adam", eng.build_plan("FULL", lr=1e-4, optimizer="adam"))
            show("madnet", prec, tag, "FULL inputs", eng.build_plan("FULL", lr=1e-4, inputs=ops.InputTable(lib, "cpu")))
            show("madnet", prec, tag, "TRAIN", eng.build_plan("TRAIN", lr=1e-4))
        for name, cfg in sorted(cfgs.items()):
            blocks = [(lv, block_vars(layers)) for lv, layers in zip(E.LEVELS, cfg)]
            for lv, bv in (blocks if not full_only else blocks[-1:]):
                show("madnet", prec, tag, "MAD%d %s" % (lv, name), eng.build_plan("MAD", lr=1e-4, block_level=lv, block_vars=bv))
            show("madnet", prec, tag, "MAD two blocks %s" % name, eng.build_plan("MAD", lr=1e-4, blocks=[blocks[1], blocks[4]]))
        show("madnet", prec, tag, "FULL after MAD", eng.build_plan("FULL", lr=1e-4))
        eng.close()

    for prec in ("fp32", "mixed", "bf16"):
        madnet("default", prec, full_only=False)
        madnet("B=4", prec, B=4)
        madnet("warping=False", prec, warping=False)
        madnet("reprojection_scale=2", prec, setup=lambda e: e.set_reprojection_scale(2))
        madnet("proxy", prec, setup=lambda e: setattr(e, "loss_kind", "proxy"))
        madnet("deterministic", prec, schedule=Schedule(DETERMINISTIC=True))
    for f in FLIPS:
        madnet("%s=%s" % (f, not getattr(Schedule(), f)), "mixed", schedule=dataclasses.replace(Schedule(), **{f: not getattr(Schedule(), f)}))
    for attr, val in (("fuse_shadows", False), ("partial_wgrad", False), ("wgrad_lanes", 0), ("wgrad_lanes", 2)):
        madnet("eng.%s=%s" % (attr, val), "mixed", setup=lambda e: setattr(e, attr, val))

    def dispnet(tag, prec, **kw):
        eng = DE.DispNetEngine(lib, H, W, B=1, device="cpu", precision=prec, **kw)
        for what, args in (("FULL", {}), ("FULL again", {}), ("NONE", {}), ("TRAIN", {}), ("FULL adam", {"optimizer": "adam"}), ("FULL after TRAIN", {})):
            show("dispnet", prec, tag, what, eng.build_plan(what.split()[0], lr=1e-4, **args))
        eng.close()

    for prec in ("fp32", "mixed", "bf16"):
        dispnet("default", prec)
        for f in DN_FLIPS:
            dispnet("%s=%s" % (f, not getattr(DispNetSchedule(), f)), prec, schedule=dataclasses.replace(DispNetSchedule(), **{f: not getattr(DispNetSchedule(), f)}))


if __name__ == "__main__":
    for hw in ([tuple(map(int, sys.argv[1:3]))] if len(sys.argv) > 2 else [(128, 256), (375, 1242)]):
        main(*hw)
