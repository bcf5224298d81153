"""madnet_hip.summary.SummaryWriter against a reader of its own: TFRecord framing plus the five messages (Event, Summary, Value, Image, and the version
event), with a bitwise crc32c that shares nothing with the writer's table-driven one."""
import io
import os
import re
import struct

import numpy as np
import pytest

from madnet_hip.summary import SummaryWriter


# ---- the reader -------------------------------------------------------------------------------------------------------------------------------
def crc32c_bitwise(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
    return c ^ 0xFFFFFFFF


def masked(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def records(blob):
    """the payloads of a TFRecord stream; both CRCs of every record checked; raises on a torn record"""
    out, pos = [], 0
    while pos < len(blob):
        assert pos + 12 <= len(blob), "torn record header at %d" % pos
        (n,) = struct.unpack_from("<Q", blob, pos)
        assert struct.unpack_from("<I", blob, pos + 8)[0] == masked(crc32c_bitwise(blob[pos:pos + 8])), "length crc of record %d" % len(out)
        assert pos + 12 + n + 4 <= len(blob), "torn record payload at %d" % pos
        payload = blob[pos + 12:pos + 12 + n]
        assert struct.unpack_from("<I", blob, pos + 12 + n)[0] == masked(crc32c_bitwise(payload)), "payload crc of record %d" % len(out)
        out.append(payload)
        pos += 12 + n + 4
    return out


def fields(buf):
    """protobuf -> [(field, wire type, value)]: varint -> int, 64-bit / 32-bit -> raw bytes, length-delimited -> bytes"""
    out, pos = [], 0
    while pos < len(buf):
        key, shift = 0, 0
        while True:
            b = buf[pos]; pos += 1
            key |= (b & 0x7F) << shift; shift += 7
            if not b & 0x80:
                break
        f, w = key >> 3, key & 7
        if w == 0:
            v, shift = 0, 0
            while True:
                b = buf[pos]; pos += 1
                v |= (b & 0x7F) << shift; shift += 7
                if not b & 0x80:
                    break
        elif w == 1:
            v = buf[pos:pos + 8]; pos += 8
        elif w == 5:
            v = buf[pos:pos + 4]; pos += 4
        else:
            assert w == 2, "wire type %d" % w
            n, shift = 0, 0
            while True:
                b = buf[pos]; pos += 1
                n |= (b & 0x7F) << shift; shift += 7
                if not b & 0x80:
                    break
            v = buf[pos:pos + n]; pos += n
        out.append((f, w, v))
    assert pos == len(buf)
    return out


def event(payload):
    """-> dict(wall_time, step, file_version, values=[(tag, float32 bits | None, (h, w, colorspace, png) | None)])"""
    ev = {"step": 0, "file_version": None, "values": [], "wall_time": None}
    for f, w, v in fields(payload):
        if (f, w) == (1, 1):
            ev["wall_time"] = struct.unpack("<d", v)[0]
        elif (f, w) == (2, 0):
            ev["step"] = v
        elif (f, w) == (3, 2):
            ev["file_version"] = v.decode()
        elif (f, w) == (5, 2):
            for sf, sw, sv in fields(v):
                assert (sf, sw) == (1, 2)
                tag, simple, image = None, None, None
                for vf, vw, vv in fields(sv):
                    if (vf, vw) == (1, 2):
                        tag = vv.decode()
                    elif (vf, vw) == (2, 5):
                        simple = struct.unpack("<I", vv)[0]
                    elif (vf, vw) == (4, 2):
                        im = {k: x for k, _, x in fields(vv)}
                        image = (im[1], im[2], im[3], im[4])
                    else:
                        raise AssertionError("unexpected Value field %d / %d" % (vf, vw))
                ev["values"].append((tag, simple, image))
        else:
            raise AssertionError("unexpected Event field %d / %d" % (f, w))
    return ev


def read_events(path):
    return [event(p) for p in records(open(path, "rb").read())]


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
def test_reader_crc_known_answers():
    assert crc32c_bitwise(b"123456789") == 0xE3069283
    assert crc32c_bitwise(bytes(32)) == 0x8A9136AA


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _images(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(13, 17, 3), dtype=np.uint8)


def test_event_file_holds_what_was_added(tmp_path):
    from PIL import Image
    clock = iter([1700000123.75, 1700000124.5, 1700000125.25, 1700000126.0])
    a, b = _images(1), _images(2)
    with SummaryWriter(str(tmp_path), wall_time=lambda: next(clock), hostname="box7") as w:
        w.add(0, scalars={"EPE": 1.25, "bad3": 0.1}, images={"full_res_disp/image": a, "gt_disp/image": b})
        w.add(100, scalars={"bad3": 3.0e-8, "EPE": 2.0 ** 24 + 1})            # order as given, not sorted; a value float32 has to round
        w.add(300000, images={"gt_disp/image": b})
        path = w.path
    assert os.listdir(str(tmp_path)) == ["events.out.tfevents.1700000123.box7"] and os.path.basename(path) == "events.out.tfevents.1700000123.box7"
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\.box7", os.path.basename(path))
    evs = read_events(path)
    assert len(evs) == 4
    assert evs[0]["file_version"] == "brain.Event:2" and evs[0]["wall_time"] == 1700000123.75 and evs[0]["values"] == [] and evs[0]["step"] == 0
    assert [e["step"] for e in evs[1:]] == [0, 100, 300000] and [e["wall_time"] for e in evs[1:]] == [1700000124.5, 1700000125.25, 1700000126.0]
    assert all(e["file_version"] is None for e in evs[1:])
    assert [v[0] for v in evs[1]["values"]] == ["EPE", "bad3", "full_res_disp/image", "gt_disp/image"]
    assert [v[1] for v in evs[1]["values"][:2]] == [_bits(1.25), _bits(0.1)] and all(v[2] is None for v in evs[1]["values"][:2])
    for (tag, simple, image), want in zip(evs[1]["values"][2:], (a, b)):
        assert simple is None and image[:3] == (13, 17, 3)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(image[3])).convert("RGB")), want), tag
        assert image[3][:8] == b"\x89PNG\r\n\x1a\n"
    assert [(v[0], v[1]) for v in evs[2]["values"]] == [("bad3", _bits(3.0e-8)), ("EPE", _bits(2.0 ** 24))]
    assert [v[0] for v in evs[3]["values"]] == ["gt_disp/image"]


def test_default_name_and_tensor_images(tmp_path):
    import socket
    import torch
    img = _images(3)
    w = SummaryWriter(str(tmp_path / "sub" / "dir"))                          # the folder is made
    w.add(7, images={"x/image": torch.from_numpy(img)})
    w.close(); w.close()
    name = os.path.basename(w.path)
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\." + re.escape(socket.gethostname()), name)
    from PIL import Image
    (tag, _, image), = read_events(w.path)[1]["values"]
    assert tag == "x/image" and np.array_equal(np.asarray(Image.open(io.BytesIO(image[3]))), img)
    with pytest.raises(ValueError):
        SummaryWriter(str(tmp_path / "bad")).add(0, images={"y": img[..., 0]})


def test_a_file_read_mid_run_holds_whole_records_only(tmp_path):
    """every event is flushed when add returns: a copy taken between two adds (a killed run) parses, with both CRCs, to exactly the events added so far"""
    w = SummaryWriter(str(tmp_path), hostname="h")
    for k in range(3):
        w.add(k * 100, scalars={"EPE": float(k)}, images={"full_res_disp/image": _images(k)})
        evs = read_events(w.path)                                             # the writer is still open
        assert [e["step"] for e in evs[1:]] == [100 * j for j in range(k + 1)]
    w.close()
    assert len(read_events(w.path)) == 4
