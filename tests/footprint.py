"""Store-footprint helpers of the op-level tests (no tests here): buffers with guard zones on both sides, prefilled with a NaN bit
pattern, and checks on BITS -- so a kernel that stores a value equal to what was there, or stores outside the elements it owns, does not
hide.  Used by test_conv_footprint.py, test_workspace_guards.py and the test_*_sweep.py files."""
import torch

from madnet_hip import ops

GUARD = 4096                              # elements in front of and behind the payload (the guard of tests/test_loss_tiles.py)
NAN32 = 0x7FC0BEEF                        # a quiet fp32 NaN no arithmetic produces
NAN16 = 0x7FC5                            # a quiet bf16 NaN (as int16)
_INT = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}
_FILL = {4: NAN32, 2: NAN16, 1: 0xA5, 8: 0x7FF8BEEF7FC0BEEF}


def round_up(n, m):
    return (n + m - 1) // m * m


def bf16_round(t):
    """the values a bf16 kernel sees: rounded to bf16, in the tensor's own type"""
    return t.to(torch.bfloat16).to(t.dtype)


def wide_rows(x, ld, dev, fill=float("nan")):
    """[B,H,W,C] -> the same values in rows of ld floats on the device, `fill` (NaN: it must never reach a result) in the channel padding"""
    B, H, W, Cc = x.shape
    buf = torch.full((B, H, W, ld), fill)
    buf[..., :Cc] = x
    return buf.to(dev)


def bits(t):
    """the tensor's elements as integers of the same width (CPU copy)"""
    t = t.detach().contiguous().cpu()
    return t.view(_INT[t.element_size()])


class Guarded(object):
    """One flat allocation [guard | payload of n elements | guard]; guards and payload are prefilled with the sentinel bit pattern.
    `t` is the payload (a view: its data_ptr lies inside the allocation; with the default guard it keeps the allocation's 16-byte alignment)."""

    def __init__(self, n, dtype=torch.float32, device="cpu", guard=GUARD):
        self.n, self.guard = int(n), int(guard)
        es = torch.empty(0, dtype=dtype).element_size()
        self.fill = _FILL[es]
        raw = torch.full((self.n + 2 * self.guard,), self.fill, dtype=_INT[es])
        self.all = raw.view(dtype).to(device)
        self.t = self.all[self.guard:self.guard + self.n]

    def ptr(self, off=0):
        return self.t.data_ptr() + off * self.t.element_size()

    def set(self, values):
        """payload <- values (same element count), guards stay"""
        self.t.copy_(values.reshape(-1).to(self.t.device))
        return self

    def snapshot(self):
        return bits(self.all).clone()

    def payload_bits(self):
        return bits(self.all)[self.guard:self.guard + self.n]

    def assert_guards(self, what=""):
        b = bits(self.all)
        lo, hi = b[:self.guard], b[self.guard + self.n:]
        bad_lo = (lo != self.fill).nonzero().flatten()
        bad_hi = (hi != self.fill).nonzero().flatten()
        assert bad_lo.numel() == 0, "%s: %d elements written IN FRONT of the buffer, nearest at -%d" % (what, bad_lo.numel(), self.guard - int(bad_lo.max()))
        assert bad_hi.numel() == 0, "%s: %d elements written BEHIND the buffer (%d elements), first at +%d" % (what, bad_hi.numel(), self.n, int(bad_hi.min()))


def slice_view(dev, B, H, W, C, coff, extra, prefill=None):
    """-> (Guarded g, ops.View v): v = channels [coff, coff + C) of rows of ld = coff + C + extra floats inside g's payload [B,H,W,ld].
    prefill: None = the whole payload keeps the NaN sentinel; a [B,H,W,C] tensor = the slice starts from these values (accumulating calls)."""
    ld = coff + C + extra
    g = Guarded(B * H * W * ld, torch.float32, dev)
    buf = g.t.view(B, H, W, ld)
    if prefill is not None:
        buf[..., coff:coff + C] = prefill.to(dev)
    return g, ops.View(buf, B, H, W, C, ld, coff=coff)


def slice_of(g, v, coff):
    """the slice's values as a CPU tensor [B,H,W,C]"""
    return g.t.view(v.B, v.H, v.W, v.ld)[..., coff:coff + v.C].cpu()


def assert_only_slice_written(g, v, coff, before, what="", zero_cols=0, free_cols=0):
    """g: Guarded behind the View v (slice_view); before: g.snapshot() taken in front of the launch.  Both guards intact, every element outside
    [coff, coff + C + zero_cols) bit-identical to `before`, every element of the slice finite, the zero_cols columns behind the slice hold +0.0 (free_cols: that many columns behind the slice may hold anything)."""
    g.assert_guards(what)
    now = bits(g.all)[g.guard:g.guard + g.n].view(v.B, v.H, v.W, v.ld)
    old = before[g.guard:g.guard + g.n].view(v.B, v.H, v.W, v.ld)
    c1 = coff + v.C + max(zero_cols, free_cols)
    for name, a, b in (("in front of", now[..., :coff], old[..., :coff]), ("behind", now[..., c1:], old[..., c1:])):
        diff = (a != b)
        assert not diff.any(), "%s: %d elements %s the slice [%d, %d) of rows of %d were written (first at %s)" % (
            what, int(diff.sum()), name, coff, c1, v.ld, diff.nonzero()[0].tolist())
    vals = g.t.view(v.B, v.H, v.W, v.ld)[..., coff:coff + v.C].cpu()
    assert torch.isfinite(vals).all(), "%s: %d elements of the slice were not written" % (what, int((~torch.isfinite(vals)).sum()))
    if zero_cols:
        z = now[..., coff + v.C:coff + v.C + zero_cols]
        assert (z == 0).all(), "%s: the %d padding columns behind the slice must hold +0.0" % (what, zero_cols)


def assert_untouched(g, before, what=""):
    """nothing of the allocation (guards and payload) changed a bit"""
    assert torch.equal(bits(g.all), before), "%s: %d elements were written" % (what, int((bits(g.all) != before).sum()))


def assert_fully_written(g, n=None, what=""):
    """guards intact and the first n payload elements (default: all) no longer hold the sentinel -- for workspaces documented as fully overwritten"""
    g.assert_guards(what)
    n = g.n if n is None else n
    left = (g.payload_bits()[:n] == g.fill)
    assert not left.any(), "%s: %d of %d elements were never written (first at %d)" % (what, int(left.sum()), n, int(left.nonzero()[0]))
    if n < g.n:
        tail = g.payload_bits()[n:]
        assert (tail == g.fill).all(), "%s: %d elements behind the %d documented ones were written" % (what, int((tail != g.fill).sum()), n)
