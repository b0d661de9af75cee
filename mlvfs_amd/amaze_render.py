"""Rendered full-size frames demosaiced by AMaZE: the definition of include/mlvfs_amd.h ("rendered full-size frames demosaiced by
AMaZE") restated in numpy.  Integers but for AMaZE itself, which is amaze_demosaic_RT.c and is handed in as a callable:
raw float32 (H, W) -> (red, green, blue) float32 (H, W), output planes zero beforehand -- the tests and the tools pass the checker's.
Nothing here runs on a GPU.  The parameters, the tone forms and the file's header are the other renderings' (mlvfs_amd/render.py).

    p = render.params_from_header(dng_header_bytes, gain_q8=256)
    rgb = amaze_render.render(frame_u16, p, amaze)             # (H, W, 3) uint8
    file = render.tiff_header(W, H) + rgb.tobytes()
"""
from __future__ import annotations

import numpy as np

from . import demosaic as _demosaic
from . import render as _render

HEADER_BYTES = _render.HEADER_BYTES
MIN_SIDE = 36                            # what AMaZE takes, with a width that is a multiple of 4
MAX_PIXELS = _demosaic.MAX_PIXELS        # W * H stays below it


def geom(w: int, h: int) -> tuple[int, int]:
    if w % 4 or w < MIN_SIDE or h < MIN_SIDE or w * h >= MAX_PIXELS:
        raise ValueError(f"an AMaZE rendering takes frames of 36x36 up to 2^25 pixels, the width a multiple of 4, not {w}x{h}")
    return w, h


def sample16(v) -> np.ndarray:
    """step 3: n = int(floor(clampf(v) + 0.5f)) in float32; clampf(v) is 0 for NaN and v <= 0, 65535 for v >= 65535, v otherwise.
    (np.clip alone would hand NaN on; the comparison does not)"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > np.float32(0), np.minimum(v, np.float32(65535)), np.float32(0)).astype(np.float32)
    return np.floor(c + np.float32(0.5)).astype(np.int64)


def stages(frame, p, amaze) -> dict:
    """every intermediate of the definition: b (H, W) int64 balanced samples (the full-size definition's); raw float32 (H, W);
    planes (3, H, W) float32 as AMaZE gives them; n (3, H, W) after step 3; acc, t, t16 as in the other definitions; site (H, W)"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    geom(w, h)
    K = [int(v) for v in p[4:13]]
    b = _demosaic.stages(f, p)["b"]
    raw = b.astype(np.float32)                                     # b <= 65535: exact
    planes = np.stack([np.asarray(c, np.float32) for c in amaze(raw)])
    assert planes.shape == (3, h, w)
    n = sample16(planes)
    acc = np.stack([sum(np.int64(K[3 * i + k]) * n[k] for k in range(3)) for i in range(3)])
    t = np.clip((acc + 32768) >> 16, 0, 4095)
    return dict(b=b, raw=raw, planes=planes, n=n, acc=acc, t=t, t16=_render.index16(acc), site=_demosaic.site_colour(h, w))


def render(frame, p, amaze, lut=None, look=None, look16=None) -> np.ndarray:
    """(H, W, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit rendering through
    a deep look, uint16"""
    return _render.develop(stages(frame, p, amaze), lut, look, look16)


def split_file(file, w: int, h: int) -> np.ndarray:
    """the pixels of one served file"""
    return _render.split_file(file, w, h)
