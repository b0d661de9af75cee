"""What the lossless-DNG tests share (tests/test_lossless_dng.py on the CPU, tests/test_gpu_lossless_dng.py on the GPU): the
synthetic clips' frames, the stream geometry, a TIFF walk and a look into a stream's DHT segment."""
import struct

import numpy as np

from mlvfs_amd import synth

W, H = 416, 264                     # the clips of tests/test_gpu_ref_host.py / tests/test_gpu_mount.py
BIG_W, BIG_H, BIG_N = 3584, 1320, 8


def clip_frames(kind, n=5):
    """The frames make_clip (test_gpu_ref_host.py) and dual_clip (test_gpu_mount.py) put into their clips."""
    if kind == "dual":
        return [synth.dual_iso_frame(W, H, frame=k) for k in range(n)]
    return [synth.normal_frame(W, H, seed=9, frame=k, hot=60, cold=60) for k in range(n)]


def fallback_frames(n=5, at=2):
    """A clip in which frame `at` cannot be served compressed: its first pixel is 0, the first difference -32768 (class 16)."""
    frames = clip_frames("plain", n)
    frames[at] = frames[at].copy()
    frames[at][0, 0] = 0
    return frames


LONG_K = 10                         # classes 1 .. 10 in long_stream_frames' staircase: class 0's code is ten one-bits or more


def long_stream_frames(n=5, at=2):
    """A clip in which frame `at` cannot be served compressed although every difference class is below 16: its rows alternate the two
    halves of one staircase of 2W values, so every row of the 2W x H/2 view is that staircase and every difference below the first row
    is zero.  The staircase uses class j Fibonacci(j) times (1, 1, 2, 3, 5 ...), j = 1 .. LONG_K, which gives class 0 -- the all-ones
    code of the reference's table, the longest -- LONG_K bits or more: a stream of 0xFF bytes, each stuffed, longer than the pixels."""
    frames = clip_frames("plain", n)
    steps, a, b = [], 1, 1
    for j in range(1, LONG_K + 1):
        steps += [1 << (j - 1)] * a
        a, b = b, a + b
    row = [8192]
    for k in range(2 * W - 1):
        d = steps[k] if k < len(steps) else 0
        row.append(row[-1] + d if row[-1] + d < 16384 else row[-1] - d)
    pair = np.array(row, np.uint16).reshape(2, W)
    frames[at] = np.ascontiguousarray(np.tile(pair, (H // 2, 1)))
    return frames


def mount_stream_room(w, h):
    """(cap, stride) of csrc/mount.cpp for a w x h frame: a stream longer than the pixels (cap) is not served; the room a stream has
    on the device is the frames' own stride there, the pixels' size rounded up to 256 bytes"""
    img = w * h * 2
    return img // 4 * 4, (img + 255) // 256 * 256


def big_frames():
    return [synth.normal_frame(BIG_W, BIG_H, seed=1, frame=k) for k in range(BIG_N)]


def jpeg_view(img):
    """The component a w x h Bayer frame is encoded as: 2w x h/2 (the row above is then the same colour), w x h for an odd h."""
    h, w = img.shape
    return np.ascontiguousarray(img).reshape(h // 2, 2 * w) if h % 2 == 0 else np.ascontiguousarray(img)


def max_class(stream):
    """Highest SSSS a stream of the reference's encoder can use: SOI, SOF3 (13 bytes), then DHT = marker, length, Tc/Th, 16 counts,
    the values."""
    assert stream[:2] == b"\xff\xd8" and stream[2:4] == b"\xff\xc3" and stream[15:17] == b"\xff\xc4"
    n = sum(stream[20:36])
    return max(stream[36:36 + n])


def ifd0(buf):
    """{tag: (type, count, value, offset of the value field)} of IFD0"""
    assert struct.unpack_from("<HHI", buf, 0) == (0x4949, 42, 8)
    (count,) = struct.unpack_from("<H", buf, 8)
    out = {}
    for i in range(count):
        at = 10 + 12 * i
        tag, typ, cnt, val = struct.unpack_from("<HHII", buf, at)
        out[tag] = (typ, cnt, val, at + 8)
    return out


def assert_lossless_header(got, plain, length):
    """got = plain everywhere but in the value fields of Compression (259) = 7 and StripByteCounts (279) = length"""
    got, plain = bytes(got), bytes(plain)
    assert len(got) == len(plain) == 65536
    a, b = ifd0(got), ifd0(plain)
    assert a.keys() == b.keys()
    assert a[259][:3] == (3, 1, 7) and b[259][:3] == (3, 1, 1)
    assert a[279][:3] == (4, 1, length)
    assert a[258][2] == 16 and a[273][2] == 65536 and a[278][2] == b[257][2]
    masked = bytearray(got)
    for tag in (259, 279):
        at = a[tag][3]
        assert at == b[tag][3]
        masked[at:at + 4] = plain[at:at + 4]
    assert bytes(masked) == plain
