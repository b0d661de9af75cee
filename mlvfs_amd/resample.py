"""Rendered frames resampled from the full-size rendering: the definition of include/mlvfs_amd.h ("rendered frames resampled from the
full-size rendering") restated in numpy integers.  The tests and the tools share it as the yardstick; nothing here
runs on a GPU.  The source is the full-size rendering's three demosaiced channels (mlvfs_amd/demosaic.py, stages()["n"]); the two
averaging passes are the scaled rendering's (mlvfs_amd/scale.py, average) with W and H in the place of W' and H'; the parameters,
the matrix, the tone step and the file's header are the half-size rendering's.

    p = render.params_from_header(dng_header_bytes, gain_q8=256)
    ow, oh = resample.fit(W, H, 1920, 1080)
    rgb = resample.render(frame_u16, p, ow, oh)                # (oh, ow, 3) uint8
    file = render.tiff_header(ow, oh) + rgb.tobytes()

This is not scale.render at the sizes both take: this averages interpolated samples, that averages superpixels.
"""
from __future__ import annotations

import numpy as np

from . import demosaic as _demosaic
from . import render as _render
from . import scale as _scale

HEADER_BYTES = _render.HEADER_BYTES
MIN_SIDE = _demosaic.MIN_SIDE
MAX_SIDE = 65535                         # of the W x H grid
MAX_PIXELS = _demosaic.MAX_PIXELS        # W * H stays below it


def geom(w: int, h: int, ow: int | None = None, oh: int | None = None) -> tuple[int, int]:
    """W, H of a frame the resampled rendering takes; with ow, oh: and that size is one it gives"""
    if w < MIN_SIDE or h < MIN_SIDE or w * h >= MAX_PIXELS or w > MAX_SIDE or h > MAX_SIDE:
        raise ValueError(f"a resampled rendering takes frames of 4x4 up to 2^25 pixels and {MAX_SIDE} a side, not {w}x{h}")
    if ow is not None and not (1 <= ow <= w and 1 <= oh <= h):
        raise ValueError(f"a resampled rendering of a {w}x{h} frame is 1x1 up to {w}x{h}, not {ow}x{oh}")
    return w, h


def fit(w: int, h: int, box_w: int, box_h: int) -> tuple[int, int]:
    """the largest size inside a box at the frame's aspect, on the W x H grid (mlvfs_amd_rgb_fit_full)"""
    geom(w, h)
    if box_w < 1 or box_h < 1:
        raise ValueError(f"a box of {box_w}x{box_h}")
    if box_w * h <= box_h * w:
        ow = min(box_w, w)
        return ow, max(1, (2 * ow * h + w) // (2 * w))
    oh = min(box_h, h)
    return max(1, (2 * oh * w + h) // (2 * h)), oh


def stages(frame, p, ow: int, oh: int, border: str = "reflect", source=None) -> dict:
    """every intermediate of the definition as int64 arrays: d (3, H, W) the demosaiced source, hd (3, H, ow), m (3, oh, ow), acc, t,
    t16.  source: d where the caller has it already (demosaic.stages(frame, p)["n"]) -- one frame at several sizes"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    geom(w, h, ow, oh)
    d = _demosaic.stages(f, p, border)["n"] if source is None else source
    hd = _scale.average(d, ow)
    m = _scale.average(hd.transpose(0, 2, 1), oh).transpose(0, 2, 1)
    K = p[4:13]
    acc = np.stack([sum(np.int64(K[3 * i + j]) * m[j] for j in range(3)) for i in range(3)])
    t = np.clip((acc + 32768) >> 16, 0, 4095)
    return dict(d=d, hd=hd, m=m, acc=acc, t=t, t16=_render.index16(acc))


def render(frame, p, ow: int, oh: int, lut=None, look=None, look16=None, source=None) -> np.ndarray:
    """(oh, ow, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit rendering
    through a deep look, uint16"""
    return _render.develop(stages(frame, p, ow, oh, source=source), lut, look, look16)


def split_file(file, ow: int, oh: int) -> np.ndarray:
    """the pixels of one served file"""
    return _render.split_file(file, ow, oh)
