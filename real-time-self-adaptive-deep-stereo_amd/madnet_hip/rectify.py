"""Rectification of raw camera pairs on the device from a calibration.  The reference leaves "all the op necessary to read/decode and rectify stereo frames" to
each Demo/grabber.py subclass (README.MD:97) and its one grabber lets the camera SDK do it; MADNet assumes that epipolar lines are image rows, so two plain cameras
(or a recording of them) need this step in front of the network.  Two device calls: mh_rectify_map builds, once, the position in the raw view of every rectified
pixel (OpenCV's initUndistortRectifyMap formula: pinhole model, k1 k2 p1 p2 k3), mh_remap samples every frame pair there (exact bilinear, zero outside the source).
Runs outside the captured step, like mh_frame_prepare.

Calibration: a dict, or the path of a JSON file holding one:
    {"size": [h, w],               raw frame size
     "out_size": [Ho, Wo],         rectified frame size; optional, default = size
     "left":  {"K": 3x3, "D": [k1, k2, p1, p2, k3], "R": 3x3, "P": 3x4 or 3x3},
     "right": {...}}
K and D are the view's camera matrix and distortion (D may be shorter than 5, missing terms are 0), R and P are what OpenCV's stereoRectify returns for it (R1 / P1,
R2 / P2; of P only the camera matrix P[:, :3] is read).  A view may give {"map": "file.npy"} instead: a float32 [Ho, Wo, 2] array of (x, y) positions in the raw
view, which serves any other lens model (fisheye, rational); a relative path is taken from the JSON file's folder.  Who has only the extrinsics of the pair gets R
and P from stereo_calibration / Rectifier.from_stereo."""
import json
import os

import numpy as np
import torch

from . import ops


def stereo_calibration(K1, D1, K2, D2, R, T, size, out_size=None):
    """The calibration dict of a camera pair from its intrinsics and extrinsics; host side, float64 numpy.

    Conventions.  K1, K2: 3x3 camera matrices of the left and the right camera, D1, D2 their distortion terms.  R (3x3), T (3): a point with coordinates X1 in the
    left camera's frame has X2 = R X1 + T in the right camera's (OpenCV's stereoCalibrate convention), so the right camera's centre is c2 = -R^T T in the left frame
    and the baseline is |T|.  size: (h, w) of the raw frames.

    Rectification after Fusiello, Trucco and Verri (2000): both cameras are rotated about their centres onto one orientation whose
      x axis  e1 = c2 / |c2|            runs along the baseline, from the left centre to the right one (from the right to the left one if c2 has a negative x, so that
                                        the image is not turned upside down for a pair given in the other order),
      y axis  e2 = z_left x e1, normalised, with z_left = (0, 0, 1) the left camera's old optical axis,
      z axis  e3 = e1 x e2.
    With Q = [e1; e2; e3] (rows) the rectifying rotations are R1 = Q for the left view and R2 = Q R^T for the right one (x_rect = R_i x_cam), and both views share
    one camera matrix Kn = (K1 + K2) / 2 with its skew set to 0.  P1 = [Kn | 0], P2 = [Kn | (-+ fxn |T|, 0, 0)] as stereoRectify writes them.  A point at depth Z in the
    rectified frame then lies on the same row in both views and u_left - u_right = fxn |T| / Z."""
    K1, K2, R = (np.asarray(m, np.float64).reshape(3, 3) for m in (K1, K2, R))
    T = np.asarray(T, np.float64).reshape(3)
    c2 = -R.T @ T
    norm = np.linalg.norm(c2)
    if not norm > 0:
        raise ValueError('stereo_calibration: the two cameras share one centre (T = 0)')
    e1 = c2 / norm
    if e1[0] < 0:
        e1 = -e1
    e2 = np.cross(np.array([0.0, 0.0, 1.0]), e1)
    if not np.linalg.norm(e2) > 0:
        raise ValueError('stereo_calibration: the baseline runs along the left optical axis')
    e2 = e2 / np.linalg.norm(e2)
    e3 = np.cross(e1, e2)
    Q = np.stack([e1, e2, e3])
    Kn = 0.5 * (K1 + K2)
    Kn[0, 1] = 0.0
    Kn[1, 0] = Kn[2, 0] = Kn[2, 1] = 0.0
    Kn[2, 2] = 1.0
    shift = (Q @ c2)[0]                                         # +-|T|: the right centre on the new x axis
    P1 = np.concatenate([Kn, np.zeros((3, 1))], axis=1)
    P2 = np.concatenate([Kn, np.array([[-Kn[0, 0] * shift], [0.0], [0.0]])], axis=1)
    cal = {'size': [int(size[0]), int(size[1])],
           'left': {'K': K1, 'D': np.asarray(D1 if D1 is not None else [], np.float64).reshape(-1), 'R': Q, 'P': P1},
           'right': {'K': K2, 'D': np.asarray(D2 if D2 is not None else [], np.float64).reshape(-1), 'R': Q @ R.T, 'P': P2}}
    if out_size is not None:
        cal['out_size'] = [int(out_size[0]), int(out_size[1])]
    return cal


def load_calibration(calibration):
    """dict or JSON path -> (dict, folder relative map paths are taken from)"""
    if isinstance(calibration, dict):
        return calibration, os.getcwd()
    with open(calibration) as f_in:
        return json.load(f_in), os.path.dirname(os.path.abspath(calibration))


def crop_or_pad(x, th, tw):
    """tf.image.resize_image_with_crop_or_pad on a [B,h,w,c] device tensor (Demo/demo_model.py:84-86): centre crop with offset
    (in - target)//2, centre zero pad with (target - in)//2 in front."""
    h, w = x.shape[1], x.shape[2]
    if h > th:
        o = (h - th) // 2
        x = x[:, o:o + th]
    if w > tw:
        o = (w - tw) // 2
        x = x[:, :, o:o + tw]
    h, w = x.shape[1], x.shape[2]
    if h < th or w < tw:
        out = x.new_zeros(x.shape[0], th, tw, x.shape[3])
        pt, pl = (th - h) // 2, (tw - w) // 2
        out[:, pt:pt + h, pl:pl + w] = x
        x = out
    return x


class Rectifier(object):
    """Builds the sampling map of both views once, at construction (on the current stream), and owns it.  apply(frames): [2,h,w,c] uint8 or float32 device
    tensor of raw frames (left first; c = 1, 3 or 4) -> [2,Ho,Wo,3] float32 on the frames' scale, zero where a rectified pixel has no source."""

    def __init__(self, lib, calibration, device='cuda'):
        cal, base = load_calibration(calibration)
        for key in ('size', 'left', 'right'):
            if key not in cal:
                raise ValueError("calibration lacks '%s'" % key)
        self.lib, self.device = lib, torch.device(device)
        self.size = (int(cal['size'][0]), int(cal['size'][1]))
        out = cal.get('out_size') or self.size
        self.out_size = (int(out[0]), int(out[1]))
        Ho, Wo = self.out_size
        self.map = torch.empty(2, Ho, Wo, 2, dtype=torch.float32, device=self.device)
        for i, side in enumerate(('left', 'right')):
            view = cal[side]
            if 'map' in view:
                m = view['map']
                if isinstance(m, str):
                    m = np.load(m if os.path.isabs(m) else os.path.join(base, m))
                m = np.ascontiguousarray(m, dtype=np.float32)
                if m.shape != (Ho, Wo, 2):
                    raise ValueError('%s map of shape %s, the rectified frame is %d x %d' % (side, m.shape, Ho, Wo))
                self.map[i].copy_(torch.from_numpy(m))
            else:
                for key in ('K', 'R', 'P'):
                    if key not in view:
                        raise ValueError("calibration of the %s view lacks '%s' (or a 'map')" % (side, key))
                cam = ops.camera_model(np.asarray(view['K']).tolist(), np.asarray(view.get('D', [])).reshape(-1).tolist(), np.asarray(view['R']).tolist(),
                                       np.asarray(view['P']).tolist())
                ops.rectify_map(lib, [cam], self.map[i:i + 1], stream=self._stream())

    @classmethod
    def from_stereo(cls, K1, D1, K2, D2, R, T, size, lib=None, device='cuda', out_size=None):
        """Rectifier of a pair of which only intrinsics and extrinsics are known: X2 = R X1 + T, Fusiello's rectification (stereo_calibration states the
        conventions).  lib: the loaded library (default: the product library)."""
        if lib is None:
            from . import _ffi
            lib = _ffi.lib()
        return cls(lib, stereo_calibration(K1, D1, K2, D2, R, T, size, out_size), device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == 'cuda' else None

    def new_output(self):
        return torch.empty(2, self.out_size[0], self.out_size[1], 3, dtype=torch.float32, device=self.device)

    def apply(self, frames, out=None):
        """one launch on the current stream"""
        if frames.dim() != 4 or frames.shape[0] != 2 or tuple(frames.shape[1:3]) != self.size:
            raise ValueError('frames of shape {}, the calibration is for [2, {}, {}, c]'.format(tuple(frames.shape), *self.size))
        if frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError('frames must be uint8 or float32')
        if out is None:
            out = self.new_output()
        ops.remap(self.lib, frames.contiguous(), self.map, out, stream=self._stream())
        return out

    def valid_masks(self, image_shape=None, crop_shape=None):
        """(valid_l, valid_r), uint8 [1,H,W] on the device: which pixels of the frames the network sees show something -- for Adapter(valid_masks=).  Set-up
        time, in torch.  A rectified pixel is valid when its map position lies inside the raw view, 0 <= mx <= Ws - 1 and 0 <= my <= Hs - 1 (there mh_remap
        reads four taps of the source; outside it blends in zeros).  That 0/1 image then goes the frames' way -- rescale_image to image_shape, crop_or_pad to
        crop_shape (None: the step is skipped, as in the demo) -- and a pixel stays valid when the result is >= 1 - 1e-5: the zeros of the pad are invalid, and so
        is every pixel an invalid one contributes to with noticeable weight."""
        Hs, Ws = self.size
        mx, my = self.map[..., 0], self.map[..., 1]
        x = ((mx >= 0) & (mx <= Ws - 1) & (my >= 0) & (my <= Hs - 1)).to(torch.float32)[..., None]          # [2,Ho,Wo,1]
        if image_shape is not None and (x.shape[1], x.shape[2]) != (int(image_shape[0]), int(image_shape[1])):
            from Data_utils import preprocessing
            x = preprocessing.rescale_image(x, image_shape)
        if crop_shape is not None:
            x = crop_or_pad(x, int(crop_shape[0]), int(crop_shape[1]))
        v = (x[..., 0] >= 1.0 - 1e-5).to(torch.uint8).contiguous()
        return v[:1], v[1:]
