"""Hot image-space functions of the reference (Data_utils/preprocessing.py:7-29,121-230,269-277) on torch tensors (storage
only), backed by the HIP kernels: pad_image, bilinear_sampler (general form) / warp_image, rescale_image,
resize_to_prediction -- same names, argument meaning and autograd behaviour (gradients flow to the sampled coordinates / the
disparity and to the images; tf.floor contributes none).  random_crop / augment (preprocessing.py:31-89) take the decoded 8-bit
frames as device tensors and run on the kernel the training input runs on (mh_frame_prepare); their host statement, which
that kernel is checked against, lives in Data_utils/data_reader.py.  colorize_img (preprocessing.py:91-117) maps a disparity through matplotlib's `gray`
or `jet` table on the device (mh_colorize)."""
import numpy as np
import torch

from madnet_hip import _ffi, ops


def _lib():
    return _ffi.lib()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def pad_image(immy, down_factor=256, dynamic=False):
    """REFLECT-pad H,W up to a multiple of down_factor (before=(new-old)//2, after=(new-old+1)//2)  (preprocessing.py:7-29)."""
    B, H, W, Cc = immy.shape
    nh = H if H % down_factor == 0 else (H // down_factor + 1) * down_factor
    nw = W if W % down_factor == 0 else (W // down_factor + 1) * down_factor
    out = torch.empty(B, nh, nw, Cc, device=immy.device)
    ops.pad_reflect(_lib(), immy.contiguous().float(), out, (nh - H) // 2, (nw - W) // 2, stream=_stream(immy))
    return out


class _ResizeFn(torch.autograd.Function):
    """tf.image.resize_images(bilinear), TF1 legacy kernel, any channel count; gradient = ResizeBilinearGrad."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        B, H, W, Cc = x.shape
        xin = x.contiguous().float()
        out = torch.empty(B, oh, ow, Cc, device=x.device)
        _lib().resize_image_fwd(ops._p(xin), ops._p(out), B, H, W, Cc, oh, ow, ops._p(_stream(x)))
        ctx.shape = (B, H, W, Cc, oh, ow)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W, Cc, oh, ow = ctx.shape
        g = g.contiguous()
        dx = torch.empty(B, H, W, Cc, device=g.device)
        _lib().resize_image_bwd(ops._p(g), ops._p(dx), B, H, W, Cc, oh, ow, ops._p(_stream(g)))
        return dx, None, None


def rescale_image(img, out_shape):
    """preprocessing.rescale_image (preprocessing.py:269-273, FULLY_DIFFERENTIABLE = False): tf.image.resize_images(bilinear),
    the TF1 legacy kernel (no half-pixel centres).  Identity at equal size."""
    oh, ow = int(out_shape[0]), int(out_shape[1])
    if (img.shape[1], img.shape[2]) == (oh, ow):
        return img
    return _ResizeFn.apply(img, oh, ow)


def resize_to_prediction(x, pred):
    return rescale_image(x, pred.shape[1:3])


class _SamplerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, coords):
        imgs = imgs.contiguous().float(); coords = coords.contiguous().float()
        B, Hs, Ws, Cc = imgs.shape
        _, Ht, Wt, _ = coords.shape
        out = torch.empty(B, Ht, Wt, Cc, device=imgs.device)
        _lib().bilinear_sampler_fwd(ops._p(imgs), ops._p(coords), ops._p(out), B, Hs, Ws, Cc, Ht, Wt, ops._p(_stream(imgs)))
        ctx.save_for_backward(imgs, coords)
        return out

    @staticmethod
    def backward(ctx, g):
        imgs, coords = ctx.saved_tensors
        B, Hs, Ws, Cc = imgs.shape
        _, Ht, Wt, _ = coords.shape
        g = g.contiguous()
        dcoords = torch.empty_like(coords) if ctx.needs_input_grad[1] else None
        dimgs = torch.zeros_like(imgs) if ctx.needs_input_grad[0] else None
        if dcoords is None and dimgs is None:
            return None, None
        _lib().bilinear_sampler_bwd(ops._p(g), ops._p(imgs), ops._p(coords), ops._p(dcoords), ops._p(dimgs), B, Hs, Ws, Cc, Ht, Wt,
                                    ops._p(_stream(g)))
        return dimgs, dcoords


def bilinear_sampler(imgs, coords):
    """preprocessing.bilinear_sampler (preprocessing.py:121-199): imgs [B,Hs,Ws,C], coords [B,Ht,Wt,2] (x, y) -> [B,Ht,Wt,C].
    Indices are clamped to the border and the weights are NOT masked -- the code's behaviour, not its docstring ("points
    outside ... have value 0"): SURVEY App. D.7."""
    return _SamplerFn.apply(imgs, coords)


def warp_image(img, flow):
    """preprocessing.warp_image (preprocessing.py:201-230): coords = (x - flow, y), then bilinear_sampler.  img [B,H,W,C],
    flow [B,H,W,1] (for stereo: img = right image, flow = disparity aligned with the left one)."""
    B, H, W, _ = flow.shape
    xs = torch.arange(W, dtype=torch.float32, device=flow.device).view(1, 1, W, 1).expand(B, H, W, 1)
    ys = torch.arange(H, dtype=torch.float32, device=flow.device).view(1, H, 1, 1).expand(B, H, W, 1)
    coords = torch.cat([xs - flow, ys], dim=-1)
    return bilinear_sampler(img, coords)


def colorize_img(value, vmin=None, vmax=None, cmap=None):
    """preprocessing.colorize_img (preprocessing.py:91-117): value [B,H,W,1] -> float32 [B,H,W,3] on value's device, the 256-entry colour map read at
    round((value - vmin) / (vmax - vmin) * 255).  vmin / vmax default to the range of the whole tensor; cmap: None / 'gray' (the default) or 'jet', the two maps
    the kernel holds.  Where the reference is undefined (vmax == vmin, non-finite values, indices outside 0..255) the result is mh_colorize's: index 0, the colour
    (1, 0, 0), the clamped index."""
    name = "gray" if cmap is None else cmap
    if name not in ops.CMAPS:
        raise ValueError("colorize_img: unknown colour map %r; the maps that exist are 'gray' and 'jet'" % (cmap,))
    if (vmin is None) != (vmax is None):         # the reference takes the missing bound from the data
        fin = value[torch.isfinite(value)]
        vmin = float(fin.min()) if vmin is None else vmin
        vmax = float(fin.max()) if vmax is None else vmax
    B, H, W = value.shape[:3]
    assert value.dim() == 4 and value.shape[3] == 1, "colorize_img: value is [B,H,W,1]"
    v = value.reshape(B, H, W).contiguous().float()
    out = torch.empty(B, H, W, 3, dtype=torch.float32, device=value.device)
    lib = _lib()
    ops.colorize(lib, v, out, ops.colorize_ws(lib, B, H, W, value.device), name, 0, vmin, vmax, stream=_stream(value))
    return out


def _as_u8(img):
    """the decoded frame the kernel reads: uint8; a float tensor is taken if it holds 8-bit values exactly"""
    if img.dtype == torch.uint8:
        return img.contiguous()
    u8 = img.to(torch.uint8)
    if not torch.equal(u8.to(img.dtype), img):
        raise ValueError("random_crop / augment take decoded 8-bit frames (uint8, or floats holding 0..255 integers)")
    return u8.contiguous()


def _frame_prepare(lefts, rights, gts, crop, recipes):
    """samples of uint8 [Hs,Ws,3] views (+ [Hs,Ws] float32 / uint16 ground truth or None) -> float32 [B,h,w,3] x 2, [B,h,w,1]; recipes: per sample
    (r0, c0, active bits, delta, contrast, hue)"""
    lib, dev, B = _lib(), lefts[0].device, len(lefts)
    h, w = int(crop[0]), int(crop[1])
    table = ops.FrameTable(lib, dev, B, pinned=False)
    held = []
    for b in range(B):
        l, r = _as_u8(lefts[b]), _as_u8(rights[b])
        Hs, Ws = l.shape[:2]
        assert tuple(r.shape) == (Hs, Ws, 3) and l.shape[2] == 3, "views must be [H,W,3] of one size"
        g = gts[b]
        if g is None:
            g = torch.zeros(Hs, Ws, dtype=torch.float32, device=dev)
        g = g.reshape(g.shape[0], g.shape[1])
        kind = 1 if g.dtype == getattr(torch, "uint16", None) else 0
        g = (g if kind else g.float()).contiguous()
        assert tuple(g.shape) == (Hs, Ws), "the ground truth must have the size of the views"
        held += [l, r, g]
        table.set(b, l.data_ptr(), r.data_ptr(), g.data_ptr(), Hs, Ws, *recipes[b][:2], kind, *recipes[b][2:])
    out = [torch.empty(B, h, w, c, dtype=torch.float32, device=dev) for c in (3, 3, 1)]
    ws = ops.frame_prepare_ws(lib, B, h, w, dev) if table.any_contrast() else None
    ops.frame_prepare(lib, table, out[0], out[1], out[2], ws, _stream(out[0]))
    return out


_rng = np.random.default_rng()


def random_crop(crop_shape, tensor_list, rng=None):
    """preprocessing.random_crop (preprocessing.py:31-58) on [left, right, gt] device tensors of one sample -- the decoded uint8 [H,W,3] views and the [H,W,1]
    (or [H,W]) ground truth -- as float32 [h,w,C] windows (the cast the reference's reader has done before, data_reader.py:98).  The window is aligned
    over the list; start row / column are uniform in [0, H - h - 1) / [0, W - w - 1): the reference's upper bounds, which never pick the last admissible
    offset (Data_utils/data_reader.random_crop).  rng: a numpy Generator (default: the module's).
    Unlike the reference, which slices any list of tensors, the list is exactly [left, right, gt]: the kernel behind it prepares a stereo sample.  Pass the
    views as uint8: a float view is accepted if it holds 8-bit values exactly, which costs a comparison on the device and a synchronisation per call."""
    rng = _rng if rng is None else rng
    if len(tensor_list) != 3:
        raise ValueError("random_crop takes [left, right, gt], got %d tensors" % len(tensor_list))
    left, right, gt = tensor_list
    H, W = left.shape[:2]
    ch, cw = int(crop_shape[0]), int(crop_shape[1])
    if H < ch or W < cw:
        raise ValueError("random_crop: image %dx%d smaller than the crop %dx%d" % (H, W, ch, cw))
    max_row, max_col = H - ch - 1, W - cw - 1
    r0 = int(rng.integers(0, max_row if max_row > 0 else 1))
    c0 = int(rng.integers(0, max_col if max_col > 0 else 1))
    l, r, g = _frame_prepare([left], [right], [gt], (ch, cw), [(r0, c0, 0, 0.0, 1.0, 1.0)])
    return [l[0], r[0], g[0]]


def augment(left_img, right_img, rng=None):
    """preprocessing.augment (preprocessing.py:61-89) on the decoded uint8 views, [H,W,3] or [B,H,W,3]: with probability 1/2 each, the SAME brightness delta,
    contrast factor and hue rotation on both views, then clip to [0, 255]; float32 out.  Draws as Data_utils/data_reader.augment: four `active` values,
    delta, contrast, hue."""
    rng = _rng if rng is None else rng
    active = rng.uniform(0.0, 1.0, size=4)
    delta, contrast, hue = rng.uniform(-0.05, 0.05), rng.uniform(0.8, 1.2), rng.uniform(0.8, 1.2)
    bits = sum(1 << k for k in range(3) if active[k + 1] <= 0.5)
    batched = left_img.dim() == 4
    lefts = list(left_img) if batched else [left_img]
    rights = list(right_img) if batched else [right_img]
    H, W = lefts[0].shape[:2]
    l, r, _ = _frame_prepare(lefts, rights, [None] * len(lefts), (H, W), [(0, 0, bits, delta, contrast, hue)] * len(lefts))
    return (l, r) if batched else (l[0], r[0])
