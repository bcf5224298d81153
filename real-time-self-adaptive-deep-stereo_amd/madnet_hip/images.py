"""The bf16 images of an engine's fp32 tensors: which View has a shadow (hi plane), which a lo plane too, and which of them a producer of the plan
being recorded has already written -- so that no cast / split launch is queued in front of a reader.  Storage and freshness only: WHETHER a producer
should write an image is the engines' decision (MadNetEngine._out_shadow / _fresh_shadow, DispNetEngine's reader sets)."""
from . import ops


class Bf16Images(object):
    def __init__(self, device):
        self.dev = device
        self.shadows = {}               # key(v) -> ops.Shadow, allocated once per engine
        self._planes = {}               # key(v) -> ops.Planes whose hi plane IS the entry of self.shadows
        self._fresh = set()             # keys whose shadow a producer of this plan wrote
        self._fresh_lo = set()          # ... and whose lo plane too

    @staticmethod
    def key(v):
        return (v.ptr, v.B, v.H, v.W, v.C)

    def shadow(self, v):
        """the ops.Shadow of View v (allocated on first use)"""
        key = self.key(v)
        sh = self.shadows.get(key)
        if sh is None:
            sh = self.shadows[key] = ops.Shadow(v.B, v.H, v.W, v.C, self.dev)
        return sh

    def planes(self, v):
        """the hi + lo ops.Planes of View v (allocated on first use); its hi plane is shadow(v): what a plane kernel wrote, the backward pass reads without a cast"""
        key = self.key(v)
        pl = self._planes.get(key)
        if pl is None:
            pl = self._planes[key] = ops.Planes(self.shadow(v), self.dev)
        return pl

    def begin_plan(self):
        """a new recording: nothing is fresh (the buffers stay)"""
        self._fresh.clear()
        self._fresh_lo.clear()

    def mark(self, v, lo=False):
        """a producer recorded in this plan writes the shadow of v (lo: both planes)"""
        self._fresh.add(self.key(v))
        if lo:
            self._fresh_lo.add(self.key(v))

    def fresh(self, v):
        """the Shadow of v if a producer of this plan wrote it, else None"""
        return self.shadows.get(self.key(v)) if self.key(v) in self._fresh else None

    def fresh_planes(self, v):
        return self.key(v) in self._fresh_lo

    def queue_cast(self, v, casts):
        """the Shadow of v; appends its cast (v, shadow) to `casts` unless a producer wrote it or that list already holds it"""
        sh = self.shadow(v)
        if self.fresh(v) is None and not any(c[1] is sh for c in casts):
            casts.append((v, sh))
        return sh
