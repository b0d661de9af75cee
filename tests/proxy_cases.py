"""Half-size Bayer proxies (include/mlvfs_amd.h, "half-size Bayer proxies"): the definition restated in numpy, the
header rule, and the cases the CPU and GPU tests share.  tests/test_proxy_cases.py proves that the cases are not vacuous."""
import struct

import numpy as np

from mlvfs_amd import synth

# (width, height) for mlvfs_amd_bin2_dev: the smallest frame, sizes with 1 .. 3 dropped columns and rows, the smallest fast shapes
# (a width that is a multiple of 16), a width the fast form does not take, more than one block row, exactly one wave per row of
# 16-pixel groups (1024 / 16 = 64 lanes), one lane more, and the mount tests' size
BIN_SIZES = [(4, 4), (6, 6), (7, 5), (16, 4), (32, 8), (20, 8), (48, 12), (1024, 8), (1040, 8), (416, 264)]
BIG_W, BIG_H = 3584, 1320
DROP_W, DROP_H = 418, 266                       # a clip whose size drops two columns and two rows

# the tags whose value fields a proxy header changes (259 as well when the strip is a stream)
PROXY_TAGS = (256, 257, 278, 279, 50719, 50720, 50829, 41486, 41487)


def proxy_size(w, h):
    return 2 * (w // 4), 2 * (h // 4)


def bin2(frame):
    """out(Y, X) = (in(y0, x0) + in(y0, x0 + 2) + in(y0 + 2, x0) + in(y0 + 2, x0 + 2) + 2) >> 2 with y0 = 4 (Y >> 1) + (Y & 1),
    x0 = 4 (X >> 1) + (X & 1): the rounded mean of the four pixels of one CFA colour inside a 4x4 block"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    pw, ph = proxy_size(w, h)
    b = f[:2 * ph, :2 * pw].astype(np.uint32).reshape(ph // 2, 2, 2, pw // 2, 2, 2)     # block row, row pair, py, block, column pair, px
    s = b.sum(axis=(1, 4)) + 2                                                          # -> block row, py, block, px
    return (s >> 2).astype(np.uint16).reshape(ph, pw)


def sums(frame):
    """the four-pixel sums behind bin2's output, before rounding"""
    f = np.asarray(frame)
    h, w = f.shape
    pw, ph = proxy_size(w, h)
    b = f[:2 * ph, :2 * pw].astype(np.uint32).reshape(ph // 2, 2, 2, pw // 2, 2, 2)
    return b.sum(axis=(1, 4)).reshape(ph, pw)


# ---- content
def random_frame(w, h, seed=0):
    """the whole 16-bit range: sums of every residue mod 4, sums above 65535"""
    return np.random.default_rng(1000 + seed).integers(0, 65536, (h, w), dtype=np.uint16)


def ones_frame(w, h):
    return np.full((h, w), 0xFFFF, np.uint16)


PARITY_CONSTANTS = (1000, 23456, 65535, 7)


def parity_frame(w, h):
    """four constants by CFA parity: a binning that mixes parities cannot give the same four constants back"""
    f = np.zeros((h, w), np.uint16)
    for py in (0, 1):
        for px in (0, 1):
            f[py::2, px::2] = PARITY_CONSTANTS[2 * py + px]
    return f


def position_frame(w, h):
    """value = (y * W + x) & 0xFFFF: any swap of rows or columns shows"""
    y, x = np.mgrid[0:h, 0:w]
    return ((y * w + x) & 0xFFFF).astype(np.uint16)


def residue_frame(w, h):
    """zeros and ones: in block (by, bx), (by + bx) % 4 of the four pixels of every colour are 1, so the sums take every residue
    0 .. 3 with small values (no carry hides a wrong rounding)"""
    f = np.zeros((h, w), np.uint16)
    y, x = np.mgrid[0:h, 0:w]
    k = ((y // 4) + (x // 4)) % 4                       # how many of the block's four same-colour pixels are 1
    order = ((y >> 1) & 1) * 2 + ((x >> 1) & 1)         # which of the four this pixel is
    f[order < k] = 1
    return f


CONTENT = ("random", "ones", "parity", "position", "residue")


def content(kind, w, h, seed=0):
    return {"random": lambda: random_frame(w, h, seed), "ones": lambda: ones_frame(w, h), "parity": lambda: parity_frame(w, h),
            "position": lambda: position_frame(w, h), "residue": lambda: residue_frame(w, h)}[kind]()


def batch(w, h, n, first=0):
    """n frames of distinct content, cycling through CONTENT from `first` on"""
    return [content(CONTENT[(first + k) % len(CONTENT)], w, h, seed=k) for k in range(n)]


# ---- the header rule
def lo(v):
    return 2 * -(-v // 4)


def hi(v, lim):
    return min(2 * (v // 4), lim)


def _walk(buf, at):
    (count,) = struct.unpack_from("<H", buf, at)
    out = {}
    for i in range(count):
        e = at + 2 + 12 * i
        tag, typ, cnt, val = struct.unpack_from("<HHII", buf, e)
        out[tag] = (typ, cnt, val, e + 8)
    return out


def header_tags(header):
    """{tag: (type, count, value field, offset of the value field)} of IFD0 and of the EXIF IFD of a 65536-byte header"""
    buf = bytes(header)
    assert struct.unpack_from("<HHI", buf, 0) == (0x4949, 42, 8)
    tags = _walk(buf, 8)
    exif = _walk(buf, tags[34665][2])
    assert not (tags.keys() & exif.keys())
    tags.update(exif)
    return tags


def _shorts(v):
    return v & 0xFFFF, v >> 16


def proxy_tags(tags, header, fh, stream_bytes=0):
    """The proxy header's fields from the full-size header's: {tag: (offset, bytes)}.  tags = header_tags(header); fh: the frame's
    headers (xRes and yRes are read).  The active area is the one the full-size header wrote (tag 50829: top, left, bottom, right =
    y1, x1, y2, x2 after its overwrite rule); DefaultScale and the focal-plane numerators are not touched."""
    buf = bytes(header)
    w, h = int(fh.rawi_hdr.xRes), int(fh.rawi_hdr.yRes)
    pw, ph = proxy_size(w, h)
    assert tags[256][2] == w and tags[257][2] == h
    out = {256: (tags[256][3], struct.pack("<I", pw)), 257: (tags[257][3], struct.pack("<I", ph)), 278: (tags[278][3], struct.pack("<I", ph)),
           279: (tags[279][3], struct.pack("<I", stream_bytes or pw * ph * 2))}
    if stream_bytes:
        out[259] = (tags[259][3], struct.pack("<I", 7))
    ox, oy = _shorts(tags[50719][2])
    out[50719] = (tags[50719][3], struct.pack("<HH", lo(ox), lo(oy)))
    assert tags[50829][:2] == (4, 4)
    at = tags[50829][2]
    top, left, bottom, right = struct.unpack_from("<4i", buf, at)
    assert _shorts(tags[50720][2]) == ((right - left) & 0xFFFF, (bottom - top) & 0xFFFF)
    x1, y1, x2, y2 = lo(left), lo(top), hi(right, pw), hi(bottom, ph)
    out[50720] = (tags[50720][3], struct.pack("<HH", max(x2 - x1, 0), max(y2 - y1, 0)))
    out[50829] = (at, struct.pack("<4i", y1, x1, y2, x2))
    for tag in (41486, 41487):
        assert tags[tag][:2] == (5, 1)
        num, den = struct.unpack_from("<2i", buf, tags[tag][2])
        out[tag] = (tags[tag][2], struct.pack("<2i", num, den * 2))
    return out


def proxy_header(header, fh, stream_bytes=0):
    """the full-size header with the proxy's fields written over their value fields: what the proxy file's first 65536 bytes must be"""
    buf = bytearray(bytes(header))
    assert len(buf) == 65536
    for at, val in proxy_tags(header_tags(buf), buf, fh, stream_bytes).values():
        buf[at:at + len(val)] = val
    return bytes(buf)


def proxy_header_from_proxy(header, stream_bytes):
    """an uncompressed proxy header -> the same frame's header with its strip as one stream: Compression 7, StripByteCounts"""
    buf = bytearray(bytes(header))
    t = header_tags(buf)
    assert t[259][:3] == (3, 1, 1)
    struct.pack_into("<I", buf, t[259][3], 7)
    struct.pack_into("<I", buf, t[279][3], stream_bytes)
    return bytes(buf)


# ---- header cases: (synth.header_case index, overrides) -> frame_headers
def header_cases():
    """[(label, FrameHeaders, fps, basename)]: three camera rows and more; an active area inside the frame whose origin is no multiple
    of 4; one larger than the frame (the overwrite rule); odd crop origins; a 5:3 case (wider than 2:1, at most 720 rows); a case
    below 2000 columns; a frame whose size drops columns and rows"""
    out = []

    def case(label, k, size=None, area=None, crop=None):
        fh, fps, base = synth.header_case(k)
        ri = fh.rawi_hdr.raw_info
        if size:
            fh.rawi_hdr.xRes, fh.rawi_hdr.yRes = size
        if area:                                            # x1, y1, x2, y2
            ri.active_area[0], ri.active_area[1], ri.active_area[2], ri.active_area[3] = area[1], area[0], area[3], area[2]
        if crop:
            ri.crop[0], ri.crop[1] = crop
        out.append((label, fh, fps, base))

    for k in (0, 1, 2, 3, 9):                               # five camera rows, as the generator has them
        case(f"generator {k}", k)
    case("area inside the frame, origin 146 x 29", 14, size=(3584, 1320), area=(146, 29, 3583, 1319), crop=(7, 3))
    case("area inside the frame, origin 2 x 1", 15, size=(1920, 1080), area=(2, 1, 1917, 1079), crop=(1, 1))
    case("area larger than the frame", 16, size=(1920, 1080), area=(146, 28, 2066, 1108), crop=(5, 9))
    case("5:3", 17, size=(1920, 672), area=(0, 0, 1920, 672), crop=(3, 5))
    case("5:3, area inside", 18, size=(2080, 720), area=(72, 26, 2080, 702), crop=(0, 1))
    case("below 2000 columns", 19, size=(1728, 972), area=(0, 0, 1728, 972), crop=(11, 2))
    case("dropped columns and rows", 20, size=(1923, 1081), area=(5, 3, 1923, 1081), crop=(2, 2))
    case("small", 21, size=(418, 266), area=(0, 0, 418, 266), crop=(0, 0))
    return out


# offset / max_size windows of the header (within the header: defined in the reference too)
WINDOWS = [(0, 65536), (0, 0), (0, 1), (0, 700), (8, 512), (644, 900), (65000, 536), (100, 65436), (0, 100000)]
