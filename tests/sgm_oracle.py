"""A plain numpy restatement of the on-device SGM proxy matcher (mh_sgm_proxy, include/madnet_hip.h): gray, 9x7 census, Hamming cost, four aggregation
paths, winner + uniqueness, left-right check from the same volume, parabola sub-pixel.  No library: loops over W and H for the paths, vectorised over the rest.
Everything up to the sub-pixel step is integer arithmetic; the sub-pixel step is one float32 division and one float32 add."""
import numpy as np

BIG = 1 << 20


def gray(img):
    """[H,W,3] uint8, or float32 holding 0..255 -> int32 [H,W]"""
    x = np.asarray(img)
    if x.dtype != np.uint8:
        x = np.clip(np.floor(x.astype(np.float32) + np.float32(0.5)), 0, 255)
    x = x.astype(np.int32)
    return (77 * x[..., 0] + 150 * x[..., 1] + 29 * x[..., 2] + 128) >> 8


def census(g):
    """62 neighbours (dy in -3..3, dx in -4..4, centre excluded), bit = g(neighbour) < g(centre), coordinates clamped: uint64 [H,W]"""
    H, W = g.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros((H, W), np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            n = g[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)]
            out = (out << np.uint64(1)) | (n < g).astype(np.uint64)
    return out


def _popcount(v):
    b = np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.int32)


def cost_volume(cl, cr, D):
    H, W = cl.shape
    C = np.full((H, W, D), 64, np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = _popcount(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(Lq, Cp, p1, p2):
    """one step of a path: Lq = L_r at the previous pixel [..., D], Cp = the cost at this one"""
    m = Lq.min(-1, keepdims=True)
    lo = np.full_like(Lq, BIG); lo[..., 1:] = Lq[..., :-1] + p1
    hi = np.full_like(Lq, BIG); hi[..., :-1] = Lq[..., 1:] + p1
    return Cp + np.minimum(np.minimum(Lq, lo), np.minimum(hi, m + p2)) - m


def aggregate(C, p1, p2):
    H, W, D = C.shape
    S = np.zeros_like(C)
    for rev in (False, True):
        L = np.empty_like(C)
        xs = range(W - 1, -1, -1) if rev else range(W)
        prev = None
        for x in xs:
            L[:, x] = C[:, x] if prev is None else _step(L[:, prev], C[:, x], p1, p2)
            prev = x
        S += L
        L = np.empty_like(C)
        ys = range(H - 1, -1, -1) if rev else range(H)
        prev = None
        for y in ys:
            L[y] = C[y] if prev is None else _step(L[prev], C[y], p1, p2)
            prev = y
        S += L
    return S


def select(S, uniq, lr_tol):
    H, W, D = S.shape
    d1 = S.argmin(-1)                                   # lowest d on ties
    s1 = np.take_along_axis(S, d1[..., None], -1)[..., 0]
    ds = np.arange(D)[None, None, :]
    far = np.abs(ds - d1[..., None]) > 1
    s2 = np.where(far, S, BIG).min(-1)
    ok = ~(far.any(-1) & (uniq * s2 < 100 * s1))
    # the right view's winner from the same volume: dR(y, x') = argmin over d with x' + d < W of S(y, x' + d, d)
    diag = np.full((H, W, D), BIG, np.int64)
    for d in range(min(D, W)):
        diag[:, :W - d, d] = S[:, d:, d]
    dR = diag.argmin(-1)
    xs = np.arange(W)[None, :] - d1
    inside = xs >= 0
    back = np.take_along_axis(dR, np.clip(xs, 0, W - 1), 1)
    ok &= inside & (np.abs(back - d1) <= lr_tol) & (d1 != 0)
    sm = np.take_along_axis(S, np.clip(d1 - 1, 0, D - 1)[..., None], -1)[..., 0]
    sp = np.take_along_axis(S, np.clip(d1 + 1, 0, D - 1)[..., None], -1)[..., 0]
    den = 2 * (sm + sp - 2 * s1)
    sub = (d1 >= 1) & (d1 <= D - 2) & (den > 0)
    frac = (sm - sp).astype(np.float32) / np.where(sub, den, 1).astype(np.float32)
    out = d1.astype(np.float32) + np.where(sub, frac, np.float32(0)).astype(np.float32)
    return np.where(ok, out, np.float32(0)).astype(np.float32)


def sgm_proxy(left, right, D=128, p1=10, p2=120, uniq=95, lr_tol=1):
    """left, right [B,H,W,3] -> float32 [B,H,W]; 0 = rejected"""
    out = []
    for l, r in zip(left, right):
        C = cost_volume(census(gray(l)), census(gray(r)), D)
        out.append(select(aggregate(C, p1, p2), uniq, lr_tol))
    return np.stack(out)
