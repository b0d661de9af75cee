"""Resampled rendered frames demosaiced by AMaZE: the definition of include/mlvfs_amd.h ("resampled rendered frames demosaiced by
AMaZE") restated in numpy.  It composes two definitions and adds no arithmetic of its own: the source is the AMaZE
rendering's three rounded channels (mlvfs_amd/amaze_render.py, stages()["n"]), the two averaging passes, the matrix and the tone step
are the resampled rendering's (mlvfs_amd/resample.py) on that source.  AMaZE itself is handed in as a callable, as amaze_render takes
it: raw float32 (H, W) -> (red, green, blue) float32 (H, W).  Nothing here runs on a GPU.

    p = render.params_from_header(dng_header_bytes, gain_q8=256)
    ow, oh = amaze_resample.fit(W, H, 1920, 1080)
    rgb = amaze_resample.render(frame_u16, p, amaze, ow, oh)   # (oh, ow, 3) uint8
    file = render.tiff_header(ow, oh) + rgb.tobytes()

ow = W, oh = H is amaze_render.render.
"""
from __future__ import annotations

import numpy as np

from . import amaze_render as _amaze_render
from . import render as _render
from . import resample as _resample

HEADER_BYTES = _render.HEADER_BYTES
MIN_SIDE = _amaze_render.MIN_SIDE        # what AMaZE takes, with a width that is a multiple of 4
MAX_SIDE = _resample.MAX_SIDE            # of the W x H grid
MAX_PIXELS = _amaze_render.MAX_PIXELS    # W * H stays below it


def geom(w: int, h: int, ow: int | None = None, oh: int | None = None) -> tuple[int, int]:
    """W, H of a frame the route takes -- both geometries: the AMaZE rendering's and the resampled rendering's; with ow, oh: and that
    size is one it gives"""
    _amaze_render.geom(w, h)
    _resample.geom(w, h, ow, oh)
    return w, h


def fit(w: int, h: int, box_w: int, box_h: int) -> tuple[int, int]:
    """the largest size inside a box at the frame's aspect (mlvfs_amd_rgb_fit_full)"""
    geom(w, h)
    return _resample.fit(w, h, box_w, box_h)


def stages(frame, p, amaze, ow: int, oh: int, source=None) -> dict:
    """every intermediate of the definition: resample.stages' d (here the AMaZE rendering's n), hd, m, acc, t, t16.  source: n where
    the caller has it already (amaze_render.stages(frame, p, amaze)["n"]) -- one frame at several sizes"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    geom(w, h, ow, oh)
    n = _amaze_render.stages(f, p, amaze)["n"] if source is None else source
    return _resample.stages(f, p, ow, oh, source=n)


def render(frame, p, amaze, ow: int, oh: int, lut=None, look=None, look16=None, source=None) -> np.ndarray:
    """(oh, ow, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit rendering
    through a deep look, uint16"""
    return _render.develop(stages(frame, p, amaze, ow, oh, source=source), lut, look, look16)


def split_file(file, ow: int, oh: int) -> np.ndarray:
    """the pixels of one served file"""
    return _render.split_file(file, ow, oh)
