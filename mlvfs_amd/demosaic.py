"""Rendered full-size sRGB frames: the definition of include/mlvfs_amd.h ("rendered full-size sRGB frames") restated
in numpy integers.  The tests and the tools share it as the yardstick; nothing here runs on a GPU.  The parameters, the tone table
and the file's header are the half-size rendering's (mlvfs_amd/render.py): only the geometry and the demosaic differ.

    p = render.params_from_header(dng_header_bytes, gain_q8=256)
    rgb = demosaic.render(frame_u16, p)                        # (H, W, 3) uint8
    file = render.tiff_header(W, H) + rgb.tobytes()
"""
from __future__ import annotations

import numpy as np

from . import render as _render

HEADER_BYTES = _render.HEADER_BYTES
MIN_SIDE = 4
MAX_PIXELS = 1 << 25                     # W * H stays below it

# np.pad's name for each rule that defines b outside the frame.  "reflect" is the definition's (about the edge pixel: -1 -> 1);
# the other two are the wrong forms the case tests hold the frames against: the edge pixel repeated, and the mirror that repeats
# the edge pixel (-1 -> 0), which breaks the CFA parity
BORDERS = {"reflect": "reflect", "clamp": "edge", "mirror": "symmetric"}


def geom(w: int, h: int) -> tuple[int, int]:
    if w < MIN_SIDE or h < MIN_SIDE or w * h >= MAX_PIXELS:
        raise ValueError(f"a full-size rendering takes frames of 4x4 up to 2^25 pixels, not {w}x{h}")
    return w, h


def reflect(i: int, n: int) -> int:
    """the index inside 0 .. n - 1 that stands for i in -2 .. n + 1"""
    return -i if i < 0 else 2 * (n - 1) - i if i >= n else i


def matrix_fits_32(p) -> bool:
    """whether step 3 of these parameters stays inside 32 bits signed: sum_j |K[i][j]| * 65535 + 32768 < 2^31 for every row"""
    K = [int(v) for v in p[4:13]]
    return all(sum(abs(k) for k in K[3 * i:3 * i + 3]) * 65535 + 32768 < (1 << 31) for i in range(3))


def site_colour(h: int, w: int) -> np.ndarray:
    """j(y, x) = (y & 1) + (x & 1): 0 R, 1 G, 2 B"""
    y, x = np.mgrid[0:h, 0:w]
    return (y & 1) + (x & 1)


# which of the four sums (0 sG, 1 sH, 2 sV, 3 sD; -1: the site's own sample) gives channel i at a site, [y & 1][x & 1][i]
SUM_OF = (((-1, 0, 3), (1, -1, 2)),
          ((2, -1, 1), (3, 0, -1)))
SUM_NAMES = ("sG", "sH", "sV", "sD")


def stages(frame, p, border: str = "reflect") -> dict:
    """every intermediate of the definition as int64 arrays: b (H, W) balanced samples; sums (4, H, W) = sG, sH, sV, sD at every
    pixel; which (3, H, W) the index into sums that channel i takes there, -1 where it is the site's own sample; s (3, H, W) the
    sum taken (16 b where the channel is the site's own, so that (s + 8) >> 4 is b); n (3, H, W) after step 2's clamp; t (3, H, W);
    below (H, W) bool: in < black"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    geom(w, h)
    black, A, K = int(p[0]), [int(v) for v in p[1:4]], [int(v) for v in p[4:13]]
    j = site_colour(h, w)
    q = f.astype(np.int64)
    c = np.maximum(q - black, 0)
    # c <= 65535 + 2^31 and A < 2^31: the product and the rounding term stay below 2^63
    b = np.minimum((c * np.array(A, np.int64)[j] + 2048) >> 12, 65535)
    e = np.pad(b, 2, mode=BORDERS[border])
    at = lambda dy, dx: e[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    h1, v1 = at(0, -1) + at(0, 1), at(-1, 0) + at(1, 0)
    d1 = at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1)
    h2, v2 = at(0, -2) + at(0, 2), at(-2, 0) + at(2, 0)
    sums = np.stack([8 * b + 4 * (h1 + v1) - 2 * (h2 + v2),
                     10 * b + 8 * h1 - 2 * d1 - 2 * h2 + v2,
                     10 * b + 8 * v1 - 2 * d1 - 2 * v2 + h2,
                     12 * b + 4 * d1 - 3 * (h2 + v2)])
    y, x = np.mgrid[0:h, 0:w]
    which = np.array(SUM_OF, np.int64)[y & 1, x & 1].transpose(2, 0, 1)                     # (3, H, W)
    s = np.where(which < 0, 16 * b, np.take_along_axis(sums, np.maximum(which, 0), 0))
    n = np.clip((s + 8) >> 4, 0, 65535)
    acc = np.stack([sum(np.int64(K[3 * i + k]) * n[k] for k in range(3)) for i in range(3)])
    t = np.clip((acc + 32768) >> 16, 0, 4095)
    return dict(b=b, sums=sums, which=which, s=s, n=n, acc=acc, t=t, t16=_render.index16(acc), below=q < black, site=j)


def render(frame, p, lut=None, border: str = "reflect", look=None, look16=None) -> np.ndarray:
    """(H, W, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit rendering through
    a deep look, uint16"""
    return _render.develop(stages(frame, p, border), lut, look, look16)


def split_file(file, w: int, h: int) -> np.ndarray:
    """the pixels of one served file"""
    return _render.split_file(file, w, h)
