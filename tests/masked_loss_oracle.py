"""The definition of mh_reprojection_loss_masked (include/madnet_hip.h) in torch with autograd, in the dtype of the disparity (float64 or float32), built on
oracle.tf_ops.warp_image and the un-averaged ssim_map.  A helper of test_masked_loss.py, test_masked_loss_step.py and test_rectify_masks.py: no tests here.

Validity selects: what lies under an invalid pixel is replaced by zeros BEFORE any arithmetic (a NaN that only meets a zero weight or the unselected branch of a
where() would still poison autograd's products), which is legitimate because a valid pixel never reads an invalid one: both taps of its warp are valid by
definition, and a window counts only when all nine of its pixels do."""
import torch

from oracle import tf_ops as T


def validity(disp, valid_l, valid_r):
    """v [B,H,W] bool: valid_l[p] && valid_r at both clamped taps of the warp && isfinite(disp[p])"""
    B, H, W = disp.shape
    fin = torch.isfinite(disp)
    d = torch.where(fin, disp, torch.zeros_like(disp))
    x0 = torch.floor(torch.arange(W, dtype=disp.dtype).view(1, 1, W) - d)
    i0 = torch.clamp(x0, 0.0, float(W - 1)).to(torch.int64)
    i1 = torch.clamp(x0 + 1, 0.0, float(W - 1)).to(torch.int64)
    vr = valid_r != 0
    return (valid_l != 0) & fin & torch.gather(vr, 2, i0) & torch.gather(vr, 2, i1)


def windows(v):
    """[B,H-2,W-2] bool: the VALID 3x3 windows whose nine pixels are valid"""
    H, W = v.shape[1], v.shape[2]
    w = torch.ones_like(v[:, :H - 2, :W - 2])
    for dy in range(3):
        for dx in range(3):
            w = w & v[:, dy:dy + H - 2, dx:dx + W - 2]
    return w


def masked_loss(disp, left, right, valid_l, valid_r):
    """disp [B,H,W] (its dtype is the dtype of the evaluation; may require grad), left / right [B,H,W,3] in 0..255, masks [B,H,W] (non-zero = valid)
    -> (loss, SS, L1, v, N1, N2); v is held constant"""
    dt = disp.dtype
    v = validity(disp.detach(), valid_l, valid_r)
    wv = windows(v)
    n1, n2 = int(v.sum()), int(wv.sum())
    zero = torch.zeros((), dtype=dt)
    d = torch.where(v, disp, zero)
    l = torch.where((v & (valid_l != 0))[..., None], left.to(dt) / 256.0, zero)
    r = torch.where((valid_r != 0)[..., None], right.to(dt) / 256.0, zero)
    rep = torch.where(v[..., None], T.warp_image(r, d[..., None]), zero)
    l1 = torch.where(v[..., None], (rep - l).abs(), zero).sum() / (3.0 * n1) if n1 else disp.sum() * 0.0
    ss = torch.where(wv[..., None], T.ssim_map(rep, l), zero).sum() / (3.0 * n2) if n2 else disp.sum() * 0.0
    return 0.85 * ss + 0.15 * l1, ss, l1, v, n1, n2


def evaluate(disp, left, right, valid_l, valid_r, dtype):
    """-> dict(loss, ss, l1: floats; grad [B,H,W] in `dtype`; v; n1; n2)"""
    d = disp.to(dtype).requires_grad_(True)
    loss, ss, l1, v, n1, n2 = masked_loss(d, left, right, valid_l, valid_r)
    (g,) = torch.autograd.grad(loss, [d]) if (n1 or n2) else (torch.zeros_like(d),)
    return dict(loss=loss.item(), ss=ss.item(), l1=l1.item(), grad=g.detach(), v=v, n1=n1, n2=n2)


def step_loss(disp, left, right, valid_l, valid_r):
    """the signature of oracle.tf_ops.reprojection_loss (disp [B,H,W,1] at the frames' size) with the masks bound by the caller"""
    return masked_loss(disp[..., 0], left, right, valid_l, valid_r)[0]
