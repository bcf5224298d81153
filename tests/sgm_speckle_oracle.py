"""numpy restatement of mh_sgm_speckle as include/madnet_hip.h defines it (no tests here): a flood fill per frame over the 4-neighbour relation.
A pixel is valid when label > 0 (NaN, 0 and negative are not); two 4-neighbours of one frame are connected when both are valid and
|a - b| <= max_diff with the difference rounded once to float32; a component is the transitive closure; a valid pixel keeps its label, bit for bit,
when its component holds more than max_size pixels, everything else becomes 0."""
import numpy as np


def components(frame, max_diff=1.0):
    """frame [H,W] float32 -> list of int64 arrays, the flat pixel indices of every component (each in visiting order)"""
    v = np.ascontiguousarray(frame, dtype=np.float32)
    H, W = v.shape
    md = np.float32(max_diff)
    with np.errstate(invalid="ignore"):
        valid = v > 0
        right = np.zeros((H, W), bool)
        down = np.zeros((H, W), bool)
        right[:, :-1] = valid[:, :-1] & valid[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= md)      # float32 - float32: one rounding
        down[:-1, :] = valid[:-1, :] & valid[1:, :] & (np.abs(v[:-1, :] - v[1:, :]) <= md)
    right, down = right.ravel().tolist(), down.ravel().tolist()
    seen = (~valid).ravel().tolist()
    comps = []
    for start in np.flatnonzero(valid).tolist():
        if seen[start]:
            continue
        seen[start] = True
        stack, members = [start], []
        while stack:
            p = stack.pop()
            members.append(p)
            x = p % W
            if right[p] and not seen[p + 1]:
                seen[p + 1] = True; stack.append(p + 1)
            if x > 0 and right[p - 1] and not seen[p - 1]:
                seen[p - 1] = True; stack.append(p - 1)
            if down[p] and not seen[p + W]:
                seen[p + W] = True; stack.append(p + W)
            if p >= W and down[p - W] and not seen[p - W]:
                seen[p - W] = True; stack.append(p - W)
        comps.append(np.asarray(members, np.int64))
    return comps


def speckle(labels, max_size, max_diff=1.0):
    """labels [B,H,W] float32 -> the filtered map (a new array)"""
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    assert labels.ndim == 3
    out = np.zeros_like(labels)
    for b in range(labels.shape[0]):
        src, dst = labels[b].ravel(), out[b].ravel()           # views
        for members in components(labels[b], max_diff):
            if members.size > max_size:
                dst[members] = src[members]
    return out
