"""The numpy restatement of mh_sgm_proxy_ex (include/madnet_hip.h) on top of tests/sgm_oracle.py: the four diagonal aggregation paths and the 3x3 median of the
finished label map.  No library.  A diagonal path is walked row by row: row y of a path with step (dy, dx) takes its predecessor from row y - dy, column
x - dx; where that lies outside the frame a line starts and L = C."""
import numpy as np

import sgm_oracle
from sgm_oracle import _step

DIAGONALS = ((1, 1), (1, -1), (-1, 1), (-1, -1))          # paths 4 .. 7, (dy, dx)


def diagonal(C, dy, dx, p1, p2):
    """L_r of one diagonal direction: int32 [H,W,D]"""
    H, W, D = C.shape
    L = np.empty_like(C)
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    first = True
    for y in ys:
        L[y] = C[y]                                        # line starts: the whole first row, and one end of every later row
        if not first:
            if dx > 0:
                L[y, 1:] = _step(L[y - dy, :-1], C[y, 1:], p1, p2)
            else:
                L[y, :-1] = _step(L[y - dy, 1:], C[y, :-1], p1, p2)
        first = False
    return L


def aggregate8(C, p1, p2):
    S = sgm_oracle.aggregate(C, p1, p2)
    for dy, dx in DIAGONALS:
        S = S + diagonal(C, dy, dx, p1, p2)
    return S


def median3(out):
    """[H,W] labels, 0 = rejected -> a rejected pixel stays 0; a valid one becomes the lower median (index (n - 1) // 2 of the n valid values sorted ascending) of
    the valid labels among its 3x3 neighbours inside the frame"""
    H, W = out.shape
    p = np.zeros((H + 2, W + 2), out.dtype)                # outside the frame: no label
    p[1:-1, 1:-1] = out
    win = np.stack([p[i:i + H, j:j + W] for i in range(3) for j in range(3)], -1)
    n = (win > 0).sum(-1)
    srt = np.sort(np.where(win > 0, win, np.inf), -1)      # the valid values first, ascending
    med = np.take_along_axis(srt, (np.maximum(n, 1) - 1)[..., None] // 2, -1)[..., 0]
    return np.where(out > 0, med, 0).astype(out.dtype)


def window_max(out):
    """the largest label of every pixel's 3x3 window inside the frame (the scale of the median's tolerance)"""
    H, W = out.shape
    p = np.zeros((H + 2, W + 2), out.dtype)
    p[1:-1, 1:-1] = out
    return np.max([p[i:i + H, j:j + W] for i in range(3) for j in range(3)], axis=0)


def sgm_proxy(left, right, D=128, p1=10, p2=120, uniq=95, lr_tol=1, paths=4, median=0):
    """left, right [B,H,W,3] -> float32 [B,H,W]; 0 = rejected"""
    assert paths in (4, 8) and median in (0, 1, False, True)
    out = []
    for l, r in zip(left, right):
        C = sgm_oracle.cost_volume(sgm_oracle.census(sgm_oracle.gray(l)), sgm_oracle.census(sgm_oracle.gray(r)), D)
        S = aggregate8(C, p1, p2) if paths == 8 else sgm_oracle.aggregate(C, p1, p2)
        o = sgm_oracle.select(S, uniq, lr_tol)
        out.append(median3(o) if median else o)
    return np.stack(out)
