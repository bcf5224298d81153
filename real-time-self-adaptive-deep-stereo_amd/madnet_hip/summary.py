"""TensorBoard event files: what tf.summary.FileWriter + merge_all write in the reference (Stereo_Online_Adaptation.py:131-140, 196-198, 235-236), without
TensorFlow.  Host side only: scalars are plain floats, images are uint8 [H,W,3] arrays (mh_colorize with out_kind 1 makes them on the device: ops.colorize)
encoded as PNG with PIL.  The driver scripts do not call it yet: their --summary flags are still accepted and ignored.

File: events.out.tfevents.<10-digit seconds>.<hostname>, a sequence of TFRecords
    uint64 length | masked crc32c of those 8 bytes | payload | masked crc32c of the payload        (little endian)
whose payloads are Event messages: the first {1: wall_time, 3: file_version = "brain.Event:2"}, every later one {1: wall_time (double), 2: step (varint),
5: Summary{1: repeated Value{1: tag, 2: simple_value (float32) | 4: Image{1: height, 2: width, 3: colorspace = 3, 4: encoded_image_string}}}}.
The crc and the protobuf helpers are those of Data_utils/tf_checkpoint.py."""
import io
import os
import socket
import struct
import time

import numpy as np

from Data_utils.tf_checkpoint import _field, _put_varint, crc32c, mask_crc


def _bytes_field(tag, payload):
    return _field(tag, 2, _put_varint(len(payload)) + payload)


def _png(image):
    """uint8 [H,W,3] (numpy array or tensor, any device) -> (H, W, PNG bytes)"""
    from PIL import Image
    if hasattr(image, "detach"):
        image = image.detach().cpu().numpy()
    a = np.ascontiguousarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("summary image must be uint8 [H,W,3], got %s %s" % (a.dtype, a.shape))
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").save(buf, format="PNG")
    return a.shape[0], a.shape[1], buf.getvalue()


class SummaryWriter(object):
    """with SummaryWriter(logdir) as w: w.add(step, scalars={tag: float}, images={tag: uint8 [H,W,3]}).  One add = one event (as one run of merge_all), flushed at
    once, so a run that is killed leaves whole records only."""

    def __init__(self, logdir, wall_time=time.time, hostname=None):
        self._now = wall_time
        os.makedirs(logdir, exist_ok=True)
        t0 = self._now()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(t0), hostname or socket.gethostname()))
        self._f = open(self.path, "wb")
        self._record(_field(1, 1, struct.pack("<d", t0)) + _bytes_field(3, b"brain.Event:2"))

    def _record(self, payload):
        head = struct.pack("<Q", len(payload))
        self._f.write(head + struct.pack("<I", mask_crc(crc32c(head))) + payload + struct.pack("<I", mask_crc(crc32c(payload))))
        self._f.flush()

    def add(self, step, scalars=None, images=None):
        """one event at `step`: the scalars first, in the order given, then the images"""
        values = b""
        for tag, v in (scalars or {}).items():
            values += _bytes_field(1, _bytes_field(1, tag.encode()) + _field(2, 5, struct.pack("<f", float(v))))
        for tag, img in (images or {}).items():
            h, w, png = _png(img)
            image = _field(1, 0, _put_varint(h)) + _field(2, 0, _put_varint(w)) + _field(3, 0, _put_varint(3)) + _bytes_field(4, png)
            values += _bytes_field(1, _bytes_field(1, tag.encode()) + _bytes_field(4, image))
        self._record(_field(1, 1, struct.pack("<d", self._now())) + _field(2, 0, _put_varint(int(step))) + _bytes_field(5, values))

    def flush(self):
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

