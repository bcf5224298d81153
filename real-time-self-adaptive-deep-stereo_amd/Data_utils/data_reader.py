"""Input list reader for the online-adaptation driver and the offline trainer: same list format and centre crop/pad
semantics as the reference's tf.data pipeline (Data_utils/data_reader.py:55-197), as a plain Python
iterator (host IO is outside the hot path).

List file: one sample per row `left,right,gt` (Data_utils/data_reader.py:55-78).  Images: PNG/JPG
via Pillow; ground truth: 16-bit PNG (value/256, KITTI convention, :88-92), .pfm (:11-53) or .npy.
Every frame is centre-cropped / zero-padded to crop_shape like tf.image.resize_image_with_crop_or_pad
(:150) and yielded as float32 [1,H,W,C] holding the raw 0..255 values (:98).
Training (is_training=True) adds the aligned random crop and the colour augmentation of Data_utils/preprocessing.py:31-89: on the
host (random_crop / augment below: the statement the device kernel is checked against) or, with prepare='device', on the GPU behind
the upload of the decoded frames (mh_frame_prepare through device_prefetcher)."""
import os
import re

import time
import numpy as np


def read_list_file(path_file):
    """Returns (left_files, right_files, gt_files); rows must have >= 3 comma separated fields."""
    with open(path_file, 'r') as f_in:
        rows = [x.strip().split(',') for x in f_in.readlines() if x.strip()]
    if any(len(r) < 3 for r in rows):
        raise Exception('Expected lines with at least 3 comma separated fields: left,right,gt')
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def readPFM(file):
    """Portable float map reader (header: PF|Pf, 'w h', scale; rows bottom-to-top)."""
    with open(file, 'rb') as f:
        header = f.readline().rstrip().decode('ascii')
        if header not in ('PF', 'Pf'):
            raise Exception('Not a PFM file.')
        color = header == 'PF'
        m = re.match(r'^(\d+)\s(\d+)\s$', f.readline().decode('ascii'))
        if not m:
            raise Exception('Malformed PFM header.')
        width, height = int(m.group(1)), int(m.group(2))
        scale = float(f.readline().rstrip().decode('ascii'))
        data = np.fromfile(f, ('<' if scale < 0 else '>') + 'f')
    shape = (height, width, 3) if color else (height, width, 1)
    return np.flipud(np.reshape(data, shape)).astype(np.float32), abs(scale)


def _read_image(path, is_gt=False, keep_uint8=False):
    """keep_uint8: 8-bit images stay uint8 [H,W,3] (the float cast then happens on the GPU, device_prefetcher)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.npy':
        a = np.load(path).astype(np.float32)
        return a if a.ndim == 3 else a[..., None]
    if ext == '.pfm':
        return readPFM(path)[0]
    from PIL import Image
    im = Image.open(path)
    a = np.asarray(im)
    if is_gt:
        a = a.astype(np.float32)
        if a.ndim == 3:
            a = a[..., 0]
        if np.asarray(im).dtype != np.uint8:
            a = a / 256.0                       # 16-bit KITTI disparity PNG
        return a[..., None]
    if not (keep_uint8 and a.dtype == np.uint8):
        a = a.astype(np.float32)
    if a.ndim == 2:
        a = np.stack([a, a, a], -1)
    return a[..., :3]


def image_size(path):
    """(height, width) of an image / .npy / .pfm file from its header, without decoding it (the crop is drawn before the decode)"""
    ext = os.path.splitext(path)[1].lower()
    if ext == '.npy':
        shape = np.load(path, mmap_mode='r').shape            # maps the file: reads the header (any format version), not the data
        return int(shape[0]), int(shape[1])
    if ext == '.pfm':
        with open(path, 'rb') as f:
            f.readline()
            m = re.match(r'^(\d+)\s(\d+)\s$', f.readline().decode('ascii'))
        if not m:
            raise Exception('Malformed PFM header.')
        return int(m.group(2)), int(m.group(1))
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return int(h), int(w)


def _read_raw(path, is_gt=False):
    """What prepare='device' puts on the wire: 8-bit images as uint8 [H,W,3]; ground truth as [H,W], uint16 where the file is a 16-bit PNG (the
    division by 256 happens on the device), float32 otherwise."""
    if is_gt:
        ext = os.path.splitext(path)[1].lower()
        if ext in ('.npy', '.pfm'):
            return np.ascontiguousarray(_read_image(path, True)[..., 0], dtype=np.float32)
        from PIL import Image
        a = np.asarray(Image.open(path))
        if a.ndim == 3:
            a = a[..., 0]
        return a if a.dtype == np.uint16 else a.astype(np.float32) / (1.0 if a.dtype == np.uint8 else 256.0)
    a = _read_image(path, keep_uint8=True)
    if a.dtype != np.uint8:
        raise ValueError("prepare='device' takes 8-bit images; %s decodes to %s" % (path, a.dtype))
    return a


class raw_batch(object):
    """One batch of dataset(prepare='device'): the decoded frames as they are -- left / right: lists of uint8 [Hs,Ws,3], gt: list of uint16 or float32 [Hs,Ws] --
    and the per-sample recipe the device applies (mh_frame_prepare): window origin r0 / c0 in the source (negative: centre pad), active (bit 0 brightness, 1
    contrast, 2 hue), delta, contrast, hue; crop = (H, W) of the window."""
    __slots__ = ('left', 'right', 'gt', 'r0', 'c0', 'active', 'delta', 'contrast', 'hue', 'crop')

    def __init__(self, samples, crop):
        self.crop = (int(crop[0]), int(crop[1]))
        self.left, self.right, self.gt = [x[0] for x in samples], [x[1] for x in samples], [x[2] for x in samples]
        for k, name in enumerate(('r0', 'c0', 'active', 'delta', 'contrast', 'hue')):
            setattr(self, name, [x[3][k] for x in samples])

    def __len__(self):
        return len(self.left)


class _Replay(object):
    """hands draws made earlier (in the generating thread) to random_crop / augment on a worker thread"""

    def __init__(self, seq):
        self.seq = list(seq)

    def integers(self, lo, hi):
        return self.seq.pop(0)

    def uniform(self, lo, hi, size=None):
        return self.seq.pop(0)


def center_crop_or_pad(img, th, tw):
    """tf.image.resize_image_with_crop_or_pad: centre crop (offset (in-target)//2) / zero pad."""
    h, w = img.shape[:2]
    if h > th:
        o = (h - th) // 2
        img = img[o:o + th]
    if w > tw:
        o = (w - tw) // 2
        img = img[:, o:o + tw]
    h, w = img.shape[:2]
    if h < th or w < tw:
        pt, pl = (th - h) // 2, (tw - w) // 2
        out = np.zeros((th, tw) + img.shape[2:], img.dtype)
        out[pt:pt + h, pl:pl + w] = img
        img = out
    return img


def random_crop(crop_shape, arrays, rng):
    """Aligned random crop of [H,W,C] arrays (preprocessing.random_crop, Data_utils/preprocessing.py:31-58): the start row /
    column are uniform in [0, H - crop_h - 1) / [0, W - crop_w - 1) -- the reference's own upper bounds, which never pick the
    last admissible offset -- and [0, 1) = 0 when the image is not larger than the crop (short images are NOT padded there:
    the slice is simply shorter and tf.set_shape fails; here that case raises)."""
    h, w = arrays[0].shape[:2]
    ch, cw = int(crop_shape[0]), int(crop_shape[1])
    if h < ch or w < cw:
        raise ValueError("random_crop: image %dx%d smaller than the crop %dx%d" % (h, w, ch, cw))
    max_row, max_col = h - ch - 1, w - cw - 1
    r0 = int(rng.integers(0, max_row if max_row > 0 else 1))
    c0 = int(rng.integers(0, max_col if max_col > 0 else 1))
    return [x[r0:r0 + ch, c0:c0 + cw] for x in arrays]


def _rgb_to_hsv(x):
    mx, mn = x.max(-1), x.min(-1)
    d = mx - mn
    s = np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0)
    dd = np.where(d > 0, d, 1)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    h = np.where(mx == r, (g - b) / dd, np.where(mx == g, 2.0 + (b - r) / dd, 4.0 + (r - g) / dd))
    h = np.where(d > 0, (h / 6.0) % 1.0, 0.0)
    return h, s, mx


def _hsv_to_rgb(h, s, v):
    k = (np.stack([h * 6.0 + 5.0, h * 6.0 + 3.0, h * 6.0 + 1.0], -1)) % 6.0
    return v[..., None] - (v * s)[..., None] * np.clip(np.minimum(k, 4.0 - k), 0.0, 1.0)


def augment(left_img, right_img, rng):
    """preprocessing.augment (Data_utils/preprocessing.py:63-89) on float32 [H,W,3] images holding 0..255: with probability 1/2
    each (applied when the uniform draw is <= 0.5, like the tf.where there) the SAME brightness delta in +-0.05, contrast
    factor in [0.8, 1.2] and hue rotation in [0.8, 1.2] turns (i.e. +-0.2 of the colour circle) go on both views; then
    clip to [0, 255].  (The gamma branch is commented out in the reference.)"""
    active = rng.uniform(0.0, 1.0, size=4)
    delta = rng.uniform(-0.05, 0.05)
    contrast = rng.uniform(0.8, 1.2)
    hue = rng.uniform(0.8, 1.2)
    out = []
    for img in (left_img, right_img):
        x = np.asarray(img, np.float32)
        if active[1] <= 0.5:
            x = x + np.float32(delta)                                   # tf.image.adjust_brightness on a float image
        if active[2] <= 0.5:
            m = x.mean(axis=(0, 1), keepdims=True)                       # tf.image.adjust_contrast: per-channel mean
            x = (x - m) * np.float32(contrast) + m
        if active[3] <= 0.5:
            h, s, v = _rgb_to_hsv(x)
            x = _hsv_to_rgb((h + hue) % 1.0, s, v).astype(np.float32)
        out.append(np.clip(x, 0.0, 255.0).astype(np.float32))
    return out[0], out[1]


class dataset(object):
    """Iterator with the reference's constructor surface (Data_utils/data_reader.py:104-197).  Online adaptation reads the list
    in order, batch 1, centre crop / pad.  is_training=True is Train.py's pipeline: repeat(num_epochs) -> shuffle buffer of
    50 * batch_size samples -> aligned random crop -> optional augmentation -> batches of batch_size (remainder dropped)."""

    def __init__(self, path_file, batch_size=1, crop_shape=(320, 1216), num_epochs=1, augment=False,
                 is_training=False, shuffle=False, seed=0, keep_uint8=False, shard=(0, 1), prepare='host', workers=1):
        """keep_uint8 (no augmentation): 8-bit frames are yielded as uint8 [B,H,W,3] instead of float32 -- device_prefetcher then
        moves 1 byte per value over PCIe and casts on the GPU (mh_u8_to_f32); values are identical.
        prepare='device': nothing but the decode stays on the host -- the iterator yields raw_batch objects (whole decoded 8-bit frames, 16-bit ground truth as
        uint16, and per sample the crop origin and the augmentation parameters) and device_prefetcher crops, augments and casts them on the GPU
        (mh_frame_prepare).  The draws are made in the host path's order, so the same seed chooses the same samples, windows and parameters.
        One window origin serves all three arrays of a sample, so the ground truth must cover the image: after the column cut (and, in training, the row
        cut) it has to have the image's size, else ValueError -- the host path centre-crops / pads a ground truth of another height by its own size
        outside training; that case is not carried over.  Images must decode to 8 bits.
        workers=N: N threads decode ahead (PIL releases the GIL while it decodes); all draws stay in the iterating thread and the order is kept, so any N
        yields the batches of N=1.  Size it from the CPUs the job may use, not from os.cpu_count()."""
        if prepare not in ('host', 'device'):
            raise ValueError("prepare must be 'host' or 'device', got %r" % (prepare,))
        self._prepare, self._workers = prepare, max(1, int(workers))
        self._u8 = bool(keep_uint8) and not augment
        # shard = (rank, world): data-parallel training reads every world-th sample of each epoch (one pass over the list per
        # epoch in total, not one per rank)
        self._rank, self._world = int(shard[0]), max(1, int(shard[1]))
        self._left, self._right, self._gt = read_list_file(path_file)
        self._crop = tuple(crop_shape)
        self._epochs = num_epochs
        self._batch, self._augment, self._training, self._shuffle = int(batch_size), augment, is_training, shuffle
        self._rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self._left)

    def _per_rank(self):
        """samples of one epoch EVERY rank reads: the list is cut to a multiple of the world size, so that all ranks yield the same number of
        batches -- each training step issues collectives (madnet_hip/trainer.py), and a rank with one batch more would wait in an all-reduce
        its peers never enter"""
        return len(self._left) // self._world

    def get_max_steps(self):
        return (self._per_rank() * self._epochs) // self._batch

    def _samples(self):
        n = self._per_rank() * self._world
        order = [i for _ in range(self._epochs) for i in range(self._rank, n, self._world)]
        if not self._shuffle:
            for i in order:
                yield i
            return
        buf, cap = [], self._batch * 50                   # tf.data shuffle(buffer_size): draw uniformly from a sliding buffer
        for i in order:
            buf.append(i)
            if len(buf) > cap:
                yield buf.pop(int(self._rng.integers(0, len(buf))))
        while buf:
            yield buf.pop(int(self._rng.integers(0, len(buf))))

    def _load(self, i):
        th, tw = self._crop
        l, r, g = _read_image(self._left[i], keep_uint8=self._u8), _read_image(self._right[i], keep_uint8=self._u8), _read_image(self._gt[i], True)
        g = g[:, :l.shape[1]]                             # "crop gt to fit with image" (:146)
        if self._training:
            l, r, g = random_crop(self._crop, [l, r, g], self._rng)
        else:
            l, r, g = (center_crop_or_pad(x, th, tw) for x in (l, r, g))
        if self._augment:
            l, r = augment(l, r, self._rng)
        return l, r, g

    def _draw(self, i):
        """sample i's recipe, drawn in _load's order from the sizes in the file headers: (r0, c0, active bits, delta, contrast, hue) and the raw draws"""
        th, tw = self._crop
        h, w = image_size(self._left[i])
        if self._training:
            if h < th or w < tw:
                raise ValueError("random_crop: image %dx%d smaller than the crop %dx%d" % (h, w, th, tw))
            max_row, max_col = h - th - 1, w - tw - 1
            r0 = int(self._rng.integers(0, max_row if max_row > 0 else 1))
            c0 = int(self._rng.integers(0, max_col if max_col > 0 else 1))
        else:
            # center_crop_or_pad as a window origin, per axis: crop at (in - target)//2, pad by (target - in)//2 in front
            r0 = (h - th) // 2 if h >= th else -((th - h) // 2)
            c0 = (w - tw) // 2 if w >= tw else -((tw - w) // 2)
        if not self._augment:
            return (r0, c0, 0, 0.0, 1.0, 1.0), None
        active = self._rng.uniform(0.0, 1.0, size=4)
        delta, contrast, hue = self._rng.uniform(-0.05, 0.05), self._rng.uniform(0.8, 1.2), self._rng.uniform(0.8, 1.2)
        bits = sum(1 << k for k in range(3) if active[k + 1] <= 0.5)
        return (r0, c0, bits, delta, contrast, hue), [active, delta, contrast, hue]

    def _load_drawn(self, i, recipe, draws):
        """_load with the draws already made (worker threads): the host path's arrays, or the raw frames + recipe of prepare='device'"""
        if self._prepare == 'device':
            l, r, g = _read_raw(self._left[i]), _read_raw(self._right[i]), _read_raw(self._gt[i], True)
            if r.shape != l.shape:
                raise ValueError("prepare='device': left %s and right %s differ in size (%s)" % (l.shape, r.shape, self._left[i]))
            g = g[:, :l.shape[1]]                             # "crop gt to fit with image" (:146)
            if self._training:
                g = g[:l.shape[0]]                            # random_crop cuts the same rows / columns of all three
            if g.shape != l.shape[:2]:
                raise ValueError("prepare='device': ground truth %s does not cover the image %s (%s)" % (g.shape, l.shape[:2], self._gt[i]))
            return l, r, g, recipe
        th, tw = self._crop
        l, r, g = _read_image(self._left[i], keep_uint8=self._u8), _read_image(self._right[i], keep_uint8=self._u8), _read_image(self._gt[i], True)
        g = g[:, :l.shape[1]]
        if self._training:
            l, r, g = random_crop(self._crop, [l, r, g], _Replay(recipe[:2]))
        else:
            l, r, g = (center_crop_or_pad(x, th, tw) for x in (l, r, g))
        if self._augment:
            l, r = augment(l, r, _Replay(draws))
        return l, r, g

    def _loaded(self):
        """the samples in order.  The default (host, one worker) is the plain loop; otherwise the recipe is drawn here and the decode (+ the host's crop /
        augmentation) runs on the pool, at most 2 * workers samples ahead."""
        if self._prepare == 'host' and self._workers == 1:
            for i in self._samples():
                yield self._load(i)
            return
        if self._workers == 1:
            for i in self._samples():
                yield self._load_drawn(i, *self._draw(i))
            return
        import collections
        from concurrent.futures import ThreadPoolExecutor
        pending = collections.deque()
        with ThreadPoolExecutor(max_workers=self._workers) as pool:
            for i in self._samples():
                pending.append(pool.submit(self._load_drawn, i, *self._draw(i)))
                if len(pending) >= 2 * self._workers:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    def __iter__(self):
        batch = []
        for sample in self._loaded():
            batch.append(sample)
            if len(batch) == self._batch:
                if self._prepare == 'device':
                    yield raw_batch(batch, self._crop)
                else:
                    yield tuple((lambda a: a if (self._u8 and a.dtype == np.uint8) else a.astype(np.float32))(np.stack([b[k] for b in batch]))
                                for k in range(3))
                batch = []


def prepare_on_device(batch, device='cuda', lib=None):
    """One raw_batch -> (left, right [B,H,W,3], gt [B,H,W,1]) float32 tensors on `device`, on its current stream: the one-off form of what device_prefetcher
    does per ring slot (the validation batch of Train.py, Data_utils/preprocessing.random_crop / augment).  lib: the loaded library, default the product's."""
    import torch
    from madnet_hip import ops
    if lib is None:
        from madnet_hip import _ffi
        lib = _ffi.lib()
    dev = torch.device(device)
    B, (H, W) = len(batch), batch.crop
    table = ops.FrameTable(lib, dev, B, pinned=False)
    held = []
    for b in range(B):
        src = [torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).to(dev) for a in (batch.left[b], batch.right[b], batch.gt[b])]
        held += src
        Hs, Ws = batch.left[b].shape[:2]
        table.set(b, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), Hs, Ws, batch.r0[b], batch.c0[b], _gt_kind(batch.gt[b]),
                  batch.active[b], batch.delta[b], batch.contrast[b], batch.hue[b])
    out = [torch.empty(B, H, W, c, dtype=torch.float32, device=dev) for c in (3, 3, 1)]
    ws = ops.frame_prepare_ws(lib, B, H, W, dev) if table.any_contrast() else None
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else None
    ops.frame_prepare(lib, table, out[0], out[1], out[2], ws, stream)
    return tuple(out)


def _gt_kind(g):
    if g.dtype == np.uint16:
        return 1
    if g.dtype != np.float32:
        raise ValueError("prepare='device': ground truth must be uint16 or float32, got %s" % g.dtype)
    return 0


class _null_context(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class device_prefetcher(object):
    """Decode-ahead + host-to-device overlap for the online loop (replaces tf.data's prefetch,
    Data_utils/data_reader.py:171-175): a reader thread decodes frames `depth` ahead into a ring of PINNED host
    buffers, the copies are issued on a private copy stream and each yielded triple carries a HIP event the
    consumer stream waits on -- frame t+1 is decoded and uploaded while frame t adapts.

        for left, right, gt in device_prefetcher(dataset(...), 'cuda', consumer_stream=adapter.stream):
            adapter.step(left, right, gt)

    The hand-over keeps the consumer's thread out of the reader's way (round 6, scripts/exp/prefetch_phases*.py: a reader woken by the consumer between two steps
    cost the loop 30 us per step in GIL ping-pong, a cross-stream event wait in front of the step's graph 10 more): the consumer never wakes the reader -- it appends
    the slot it is done with (+ an event on its stream) to a deque the reader POLLS when it runs out of slots -- never synchronises its stream, and waits on a
    frame's upload event only if the upload is not complete yet.

    Batches of dataset(prepare='device') (raw_batch: decoded 8-bit frames + per-sample crop origin and augmentation parameters) are prepared on the device: the
    frames go up as bytes and mh_frame_prepare crops, augments and casts them on the copy stream into the slot's float32 tensors -- the consumer sees the same
    (left, right, gt) tensors through the same hand-over.
    """

    POLL = 2e-4            # seconds between two looks of a reader that is out of slots

    def __init__(self, data_set, device='cuda', depth=3, consumer_stream=None, lib=None, cast=True, proxy_matcher=None):
        """uint8 arrays from the data set are uploaded as uint8; cast=True: cast to float32 on the GPU (mh_u8_to_f32 on the copy stream; `lib` = the loaded
        library, default the product's) so that the consumer always sees float32 tensors; cast=False: yielded as uint8 device tensors (Adapter.step casts
        while it copies them into the engine's input buffers: one kernel and 5.6 MB of traffic less per image).
        proxy_matcher: a madnet_hip.proxy.ProxyMatcher for the frames' shape.  Every slot then carries a proxy disparity map [B,H,W] of its own, computed
        from the slot's left / right frames on the copy stream, behind their upload and in front of the slot's ready event (where mh_frame_prepare runs for
        the training input): it overlaps the previous step and the consumer needs no further synchronisation.  The iterator yields it in the proxy
        position, (left, right, gt, proxy, *rest)."""
        self._matcher = proxy_matcher
        self._proxy = None                       # per slot: the matcher's output
        self._lib = lib
        import collections
        import queue
        import threading
        import torch
        self._torch = torch
        self._ds, self._depth = data_set, max(2, depth)
        self._dev = torch.device(device)
        self._cuda = self._dev.type == 'cuda'
        self._cast = cast
        self._q = queue.Queue()                  # unbounded: the ring bounds what is in flight, and a put that never blocks is never woken by the consumer
        self._free = []                          # the reader's own list of free slots
        self._returned = collections.deque()     # (slot, event on the consumer's stream): appended by the consumer, popped by the reader
        self._ring = None
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._reader, daemon=True)
        self._copy_stream = torch.cuda.Stream(device=self._dev) if self._cuda else None
        self._consumer = consumer_stream         # stream the frames are consumed on (default: the current stream)
        self._raw = None                         # per slot, for raw_batch input: staging bytes (host + device), the mh_frame_seg table, the partial-sum workspace

    def _raw_ring(self, rb):
        """the ring for dataset(prepare='device'): per slot the three float32 tensors the consumer sees and a byte staging area (page-locked host + device) that
        grows to the largest batch of frames seen; the slot's mh_frame_seg table travels at its end"""
        t = self._torch
        from madnet_hip import ops
        if self._lib is None:
            from madnet_hip import _ffi
            self._lib = _ffi.lib()
        B, (H, W) = len(rb), rb.crop
        self._ring, self._raw = [], []
        for _ in range(self._depth + 1):
            devb = [t.empty((B, H, W, c), dtype=t.float32, device=self._dev) for c in (3, 3, 1)]
            self._ring.append((None, devb, t.cuda.Event() if self._cuda else None, None, t.cuda.Event() if self._cuda else None))
            self._raw.append({'host': None, 'stage': None, 'ws': None})
        self._free = list(range(len(self._ring)))[::-1]

    def _upload_raw(self, rb):
        """raw frames + the slot's mh_frame_seg table -> the slot's staging bytes (one copy over PCIe, 1 byte per image value, 2 per 16-bit disparity; the
        kernel reads frames and table from device memory) -> mh_frame_prepare on the copy stream"""
        t = self._torch
        from madnet_hip import _ffi, ops
        import ctypes
        i = self._slot(rb)
        if i is None:
            return None
        _, devb, ev, _, _ = self._ring[i]
        raw = self._raw[i]
        B, (H, W) = len(rb), rb.crop
        offs, need = [], 0
        for b in range(B):
            o = []
            for a in (rb.left[b], rb.right[b], rb.gt[b]):
                o.append(need)
                need += (a.nbytes + 15) // 16 * 16
            offs.append(o)
        tab_off = need
        need += (ctypes.sizeof(_ffi.FrameSeg) * B + 15) // 16 * 16
        contrast = any(a & 2 for a in rb.active)
        if raw['host'] is None or raw['host'].numel() < need or (contrast and raw['ws'] is None):
            # allocated with the copy stream current: the only stream these buffers are ever used on, so a block the caching allocator hands back is
            # ordered behind whatever was queued on it before.  A quarter of headroom: a set of mixed sizes re-pins host memory a few times, not per batch
            with (t.cuda.stream(self._copy_stream) if self._cuda else _null_context()):
                if raw['host'] is None or raw['host'].numel() < need:
                    cap = need + need // 4
                    raw['host'] = t.empty(cap, dtype=t.uint8, pin_memory=self._cuda)
                    raw['stage'] = t.empty(cap, dtype=t.uint8, device=self._dev) if self._cuda else raw['host']
                if contrast and raw['ws'] is None:
                    raw['ws'] = ops.frame_prepare_ws(self._lib, B, H, W, self._dev)
        hnp, base = raw['host'].numpy(), raw['stage'].data_ptr()
        table = ops.FrameTable.at(raw['host'].data_ptr() + tab_off, base + tab_off, B)
        for b in range(B):
            for a, o in zip((rb.left[b], rb.right[b], rb.gt[b]), offs[b]):
                np.copyto(hnp[o:o + a.nbytes].view(a.dtype).reshape(a.shape), a)
            Hs, Ws = rb.left[b].shape[:2]
            table.set(b, base + offs[b][0], base + offs[b][1], base + offs[b][2], Hs, Ws, rb.r0[b], rb.c0[b], _gt_kind(rb.gt[b]),
                      rb.active[b], rb.delta[b], rb.contrast[b], rb.hue[b])
        if self._cuda:
            with t.cuda.stream(self._copy_stream):
                raw['stage'][:need].copy_(raw['host'][:need], non_blocking=True)
                ops.frame_prepare(self._lib, table, devb[0], devb[1], devb[2], raw['ws'], self._copy_stream.cuda_stream)
                ev.record(self._copy_stream)
        else:
            ops.frame_prepare(self._lib, table, devb[0], devb[1], devb[2], raw['ws'], None)
        return i

    def _slot(self, arrays):
        t = self._torch
        if self._ring is None and isinstance(arrays, raw_batch):
            self._raw_ring(arrays)
        if self._ring is None:                   # allocate the ring on first use (shapes known now)
            self._ring = []
            u8 = [np.asarray(a).dtype == np.uint8 for a in arrays]
            if any(u8) and self._cast and self._lib is None:
                from madnet_hip import _ffi
                self._lib = _ffi.lib()
            for _ in range(self._depth + 1):
                host = [t.empty(np.shape(a), dtype=(t.uint8 if q else t.float32), pin_memory=self._cuda) for a, q in zip(arrays, u8)]
                stage = [t.empty(np.shape(a), dtype=t.uint8, device=self._dev) if q else None for a, q in zip(arrays, u8)]
                devb = [(s8 if (q and not self._cast) else t.empty(np.shape(a), dtype=t.float32, device=self._dev)) for a, q, s8 in zip(arrays, u8, stage)]
                self._ring.append((host, devb, t.cuda.Event() if self._cuda else None, stage, t.cuda.Event() if self._cuda else None))
            if self._matcher is not None:
                if len(arrays) < 3 or tuple(np.shape(arrays[0])) != tuple(self._matcher.shape) + (3,) or np.shape(arrays[1]) != np.shape(arrays[0]):
                    raise ValueError("proxy_matcher: built for frames %s, the data set yields %s" % (self._matcher.shape, np.shape(arrays[0])))
                self._proxy = [self._matcher.new_output() for _ in self._ring]
            self._free = list(range(len(self._ring)))[::-1]
        while not self._free:
            try:
                i, done = self._returned.popleft()
            except IndexError:
                if self._stop.is_set():
                    return None
                time.sleep(self.POLL)
                continue
            if done is not None:
                done.synchronize()               # what the consumer enqueued on this slot's buffers has run (the GIL is released while waiting)
            self._free.append(i)
        return self._free.pop()

    def _reader(self):
        t = self._torch
        try:
            for arrays in self._ds:
                if self._stop.is_set():
                    return
                if isinstance(arrays, raw_batch):        # dataset(prepare='device'): crop, augment and cast on the device
                    if self._matcher is not None:
                        raise ValueError("proxy_matcher works on uploaded frames, not on dataset(prepare='device') batches")
                    i = self._upload_raw(arrays)
                    if i is None:
                        return
                    self._q.put(i)
                    continue
                i = self._slot(arrays)
                if i is None:
                    return
                host, devb, ev, stage, _ = self._ring[i]
                for h, a in zip(host, arrays):
                    np.copyto(h.numpy(), np.asarray(a).reshape(tuple(h.shape)), casting='unsafe')     # straight into the pinned slot
                if self._cuda:
                    with t.cuda.stream(self._copy_stream):
                        for h, d, s8 in zip(host, devb, stage):
                            if s8 is None:
                                d.copy_(h, non_blocking=True)
                            else:
                                s8.copy_(h, non_blocking=True)
                                if self._cast:
                                    self._lib.u8_to_f32(s8.data_ptr(), d.data_ptr(), s8.numel(), self._copy_stream.cuda_stream)
                        if self._matcher is not None:
                            self._matcher.compute(devb[0], devb[1], out=self._proxy[i], stream=self._copy_stream.cuda_stream)
                        ev.record(self._copy_stream)
                else:
                    for h, d, s8 in zip(host, devb, stage):
                        if s8 is None:
                            d.copy_(h)
                        else:
                            s8.copy_(h)
                            if self._cast and self._lib is not None:
                                self._lib.u8_to_f32(s8.data_ptr(), d.data_ptr(), s8.numel(), None)
                    if self._matcher is not None:
                        self._matcher.compute(devb[0], devb[1], out=self._proxy[i])
                self._q.put(i)
            self._q.put(None)
        except Exception as e:                   # surface reader errors in the consumer
            self._q.put(e)

    def __iter__(self):
        self._thread.start()
        prev = None
        while True:
            i = self._q.get()
            if prev is not None:
                # the slot handed out last time: whatever the consumer enqueued on its buffers is in its stream by now -- an event behind it frees the slot for the reader
                done = None
                if self._cuda:
                    done = self._ring[prev][4]
                    done.record(self._consumer or self._torch.cuda.current_stream(self._dev))
                self._returned.append((prev, done))
            if i is None:
                return
            if isinstance(i, Exception):
                raise i
            host, devb, ev, _, _ = self._ring[i]
            if self._cuda and not ev.query():        # (uploads run a step ahead: usually complete -- no cross-stream edge in front of the step then)
                (self._consumer or self._torch.cuda.current_stream(self._dev)).wait_event(ev)
            prev = i
            if self._proxy is not None:
                yield tuple(devb[:3]) + (self._proxy[i],) + tuple(devb[3:])
                continue
            yield tuple(devb)

    def close(self):
        self._stop.set()
