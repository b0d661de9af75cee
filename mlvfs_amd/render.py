"""Rendered half-size sRGB frames: the definition of include/mlvfs_amd.h ("rendered half-size sRGB frames") restated
in Python integers and numpy.  The tests and the tools share it as the yardstick; nothing here runs on a GPU and no floating point takes
part but for srgb_lut12(), which the library never calls (it carries the table as a constant, csrc/srgb_lut12.h).

    p = params_from_header(dng_header_bytes, gain_q8=256)      # black, A[3], K[9] from tags 50714, 50717, 50728, 50965
    rgb = render(frame_u16, p)                                 # (H // 2, W // 2, 3) uint8
    file = tiff_header(W // 2, H // 2) + rgb.tobytes()
"""
from __future__ import annotations

import struct

import numpy as np

HEADER_BYTES = 256                       # mlvfs_amd_rgb_header_size()
A_MAX = (1 << 31) - 1

# D50 XYZ -> linear sRGB (Bradford-adapted), integers over 10^7
S = ((31338561, -16168667, -4906146),
     (-9787684, 19161415, 334540),
     (719453, -2289914, 14052427))


def geom(w: int, h: int) -> tuple[int, int]:
    return w // 2, h // 2


def srgb_lut12() -> np.ndarray:
    """LUT[t] = round(255 * oetf(t / 4095)): the bytes of tests/golden/srgb_lut12.bin and csrc/srgb_lut12.h"""
    return np.floor(srgb_curve12() + 0.5).astype(np.uint8)


def srgb_curve12() -> np.ndarray:
    """255 * oetf(t / 4095) before rounding, float64"""
    x = np.arange(4096, dtype=np.float64) / 4095.0
    return 255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def params(black: int, white: int, neutral, fm, gain_q8: int = 256) -> list[int]:
    """black, A[3], K[9] as Python integers.  neutral: num0, den0, num1, den1, num2, den2 (AsShotNeutral, tag 50728);
    fm: ForwardMatrix2's nine numerators over 10000 (tag 50965)."""
    if not 1 <= gain_q8 <= 65535:
        raise ValueError("gain_q8 must be 1 .. 65535")
    rng = max(white - black, 1)
    num, den = [int(v) for v in neutral[0::2]], [int(v) for v in neutral[1::2]]
    if any(v <= 0 for v in num + den):
        num, den = [1, 1, 1], [1, 1, 1]
    A = []
    for j in range(3):
        D = 256 * num[j] * rng
        A.append(min((2 * 65535 * 4096 * gain_q8 * den[j] + D) // (2 * D), A_MAX))
    K = []
    for i in range(3):
        for j in range(3):
            P = sum(S[i][k] * int(fm[3 * k + j]) for k in range(3))
            K.append((2 * 4096 * P + 10 ** 11) // (2 * 10 ** 11))          # Python's // floors towards -inf
    return [int(black)] + A + K


def _ifd(buf: bytes, at: int) -> dict:
    (count,) = struct.unpack_from("<H", buf, at)
    return {tag: (typ, cnt, val) for tag, typ, cnt, val in (struct.unpack_from("<HHII", buf, at + 2 + 12 * i) for i in range(count))}


def header_colour(header) -> tuple[int, int, list[int], list[int]]:
    """black, white, the six AsShotNeutral integers and ForwardMatrix2's nine numerators from a .dng header of this library"""
    buf = bytes(header)
    assert struct.unpack_from("<HHI", buf, 0) == (0x4949, 42, 8)
    t = _ifd(buf, 8)
    assert t[50728][:2] == (5, 3) and t[50965][:2] == (10, 9)
    black, white = struct.unpack("<i", struct.pack("<I", t[50714][2]))[0], struct.unpack("<i", struct.pack("<I", t[50717][2]))[0]
    neutral = list(struct.unpack_from("<6i", buf, t[50728][2]))
    fm = struct.unpack_from("<18i", buf, t[50965][2])
    assert all(d == 10000 for d in fm[1::2])
    return black, white, neutral, list(fm[0::2])


def params_from_header(header, gain_q8: int = 256) -> list[int]:
    return params(*header_colour(header), gain_q8)


def stages(frame, p) -> dict:
    """every intermediate of the definition as int64 arrays: c (3, H', W') after the clamp, n, acc, t -- for tests that look inside"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2 and f.shape[0] >= 2 and f.shape[1] >= 2
    h, w = f.shape
    pw, ph = geom(w, h)
    q = f[:2 * ph, :2 * pw].astype(np.int64)
    g = q[0::2, 1::2] + q[1::2, 0::2]
    c = np.stack([q[0::2, 0::2], (g + 1) >> 1, q[1::2, 1::2]])
    black, A, K = int(p[0]), p[1:4], p[4:13]
    c = np.maximum(c - black, 0)
    # c <= 65535 + 2^31 and A < 2^31: the product and the rounding term stay below 2^63
    n = np.stack([np.minimum((c[j] * np.int64(A[j]) + 2048) >> 12, 65535) for j in range(3)])
    acc = np.stack([sum(np.int64(K[3 * i + j]) * n[j] for j in range(3)) for i in range(3)])
    t = np.clip((acc + 32768) >> 16, 0, 4095)
    return dict(c=c, n=n, acc=acc, t=t, t16=index16(acc), green_sum=g)


def index16(acc) -> np.ndarray:
    """step 3d of the 16-bit routes: clamp((acc + 2048) >> 12, 0, 65535)"""
    return np.clip((np.asarray(acc, np.int64) + 2048) >> 12, 0, 65535)


def tone16(t16, look16) -> np.ndarray:
    """step 4 of the 16-bit routes on t16 (3, H, W) -> (H, W, 3) uint16; look16 = (S16, n, T) or a look.Look16"""
    from . import look as _look
    return np.ascontiguousarray(_look.apply16(t16, *_look.as_tuple16(look16)).transpose(1, 2, 0))


def develop(st: dict, lut=None, look=None, look16=None) -> np.ndarray:
    """steps 3d / 4 of a stages() result: the 8-bit rendering, or with look16 the 16-bit one"""
    if look16 is not None:
        if look is not None or lut is not None:
            raise ValueError("look16= excludes look= and lut=")
        return tone16(st["t16"], look16)
    return tone(st["t"], lut, look)


def tone(t, lut=None, look=None) -> np.ndarray:
    """step 4 on t (3, H, W) -> (H, W, 3) uint8: the table, or with look = (S, n, T) or a look.Look the definition of mlvfs_amd/look.py"""
    if look is not None:
        from . import look as _look
        return np.ascontiguousarray(_look.apply(t, *_look.as_tuple(look)).transpose(1, 2, 0))
    lut = srgb_lut12() if lut is None else np.asarray(lut, np.uint8)
    return np.ascontiguousarray(lut[t].transpose(1, 2, 0))


def render(frame, p, lut=None, look=None, look16=None) -> np.ndarray:
    """(H // 2, W // 2, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit
    rendering through a deep look, uint16"""
    return develop(stages(frame, p), lut, look, look16)


def tiff_header(pw: int, ph: int, bits: int = 8) -> bytes:
    """the file's first HEADER_BYTES bytes: a baseline little-endian TIFF, one strip of 8-bit (or 16-bit) RGB behind the header"""
    if bits not in (8, 16):
        raise ValueError(f"{bits} bits per sample (8 or 16)")
    entries = [(256, 4, 1, pw), (257, 4, 1, ph), (258, 3, 3, 158), (259, 3, 1, 1), (262, 3, 1, 2), (273, 4, 1, HEADER_BYTES), (274, 3, 1, 1),
               (277, 3, 1, 3), (278, 4, 1, ph), (279, 4, 1, 3 * (bits // 8) * pw * ph), (284, 3, 1, 1), (305, 2, 6, 164)]
    buf = struct.pack("<HHIH", 0x4949, 42, 8, len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + struct.pack("<I", 0)
    assert len(buf) == 158
    buf += struct.pack("<3H", bits, bits, bits) + b"MLVFS\0"
    return buf + bytes(HEADER_BYTES - len(buf))


def split_file16(file, pw: int, ph: int) -> np.ndarray:
    """the samples of one served 16-bit file"""
    b = bytes(file)
    assert len(b) == HEADER_BYTES + 6 * pw * ph
    return np.frombuffer(b, "<u2", offset=HEADER_BYTES).reshape(ph, pw, 3)


def split_file(file, pw: int, ph: int) -> np.ndarray:
    """the pixels of one served file"""
    b = bytes(file)
    assert len(b) == HEADER_BYTES + 3 * pw * ph
    return np.frombuffer(b, np.uint8, offset=HEADER_BYTES).reshape(ph, pw, 3)
