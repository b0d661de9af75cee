"""Rendered frames at any smaller size: the definition of include/mlvfs_amd.h ("rendered frames at any smaller size")
restated in numpy integers.  The tests and the tools share it as the yardstick; nothing here runs on a GPU.  The source is the
half-size rendering's balanced superpixels (mlvfs_amd/render.py, stages()["n"]); the parameters, the matrix, the tone table and the
file's header are that rendering's too: only the area average in between is new.

    p = render.params_from_header(dng_header_bytes, gain_q8=256)
    ow, oh = scale.fit(W, H, 1280, 720)
    rgb = scale.render(frame_u16, p, ow, oh)                   # (oh, ow, 3) uint8
    file = render.tiff_header(ow, oh) + rgb.tobytes()
"""
from __future__ import annotations

import numpy as np

from . import render as _render

HEADER_BYTES = _render.HEADER_BYTES
MAX_SIDE = 65535                         # of the W' x H' grid
MAX_PIXELS = 1 << 27                     # W * H stays below it


def geom(w: int, h: int, ow: int | None = None, oh: int | None = None) -> tuple[int, int]:
    """W', H' of a frame the scaled rendering takes; with ow, oh: and that size is one it gives"""
    pw, ph = w // 2, h // 2
    if w < 2 or h < 2 or w * h >= MAX_PIXELS or pw > MAX_SIDE or ph > MAX_SIDE:
        raise ValueError(f"a scaled rendering takes frames of 2x2 up to 2^27 pixels and {MAX_SIDE} a side at half size, not {w}x{h}")
    if ow is not None and not (1 <= ow <= pw and 1 <= oh <= ph):
        raise ValueError(f"a scaled rendering of a {w}x{h} frame is 1x1 up to {pw}x{ph}, not {ow}x{oh}")
    return pw, ph


def fit(w: int, h: int, box_w: int, box_h: int) -> tuple[int, int]:
    """the largest size inside a box at the frame's aspect (mlvfs_amd_rgb_fit)"""
    pw, ph = geom(w, h)
    if box_w < 1 or box_h < 1:
        raise ValueError(f"a box of {box_w}x{box_h}")
    if box_w >= pw and box_h >= ph:
        return pw, ph
    if box_w * ph <= box_h * pw:
        ow = min(box_w, pw)
        return ow, max(1, (2 * ow * ph + pw) // (2 * pw))
    oh = min(box_h, ph)
    return max(1, (2 * oh * pw + ph) // (2 * ph)), oh


def weights(n_src: int, n_out: int) -> np.ndarray:
    """w[u, X] = max(0, min((X + 1) n_out, (u + 1) n_src) - max(X n_out, u n_src)): (n_out, n_src) int64"""
    assert 1 <= n_out <= n_src
    X = np.arange(n_src, dtype=np.int64)[None, :]
    u = np.arange(n_out, dtype=np.int64)[:, None]
    return np.maximum(0, np.minimum((X + 1) * n_out, (u + 1) * n_src) - np.maximum(X * n_out, u * n_src))


def spans(n_src: int, n_out: int) -> tuple[np.ndarray, np.ndarray]:
    """the first and the last source index with a weight above 0, per output index"""
    u = np.arange(n_out, dtype=np.int64)
    return u * n_src // n_out, ((u + 1) * n_src - 1) // n_out


def average(a: np.ndarray, n_out: int) -> np.ndarray:
    """one pass of the definition along the last axis of an int64 array of 16-bit values:
    floor((sum_X w[u, X] a[..., X] + (n_src >> 1)) / n_src).  The sums come from one running sum -- w[u, .] is the overlap of two
    intervals, so sum_X w[u, X] a[X] = F((u + 1) n_src) - F(u n_src) with F(t) the integral of a over [0, t) in units of 1 / n_out --
    which is weights(n_src, n_out) @ a without the matrix (tests/test_scale_cases.py holds the two against each other)."""
    a = np.asarray(a, np.int64)
    n_src = a.shape[-1]
    assert 1 <= n_out <= n_src
    run = np.concatenate([np.zeros(a.shape[:-1] + (1,), np.int64), np.cumsum(a, axis=-1)], axis=-1) * n_out      # F(X n_out)
    pad = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), np.int64)], axis=-1)
    t = np.arange(n_out + 1, dtype=np.int64) * n_src
    F = run[..., t // n_out] + (t % n_out) * pad[..., t // n_out]
    s = F[..., 1:] - F[..., :-1]
    assert s.max(initial=0) + (n_src >> 1) < 1 << 32
    return (s + (n_src >> 1)) // n_src


def stages(frame, p, ow: int, oh: int) -> dict:
    """every intermediate of the definition as int64 arrays: n (3, H', W') the source, hm (3, H', ow), m (3, oh, ow), acc, t"""
    f = np.asarray(frame)
    assert f.dtype == np.uint16 and f.ndim == 2
    h, w = f.shape
    geom(w, h, ow, oh)
    n = _render.stages(f, p)["n"]
    hm = average(n, ow)
    m = average(hm.transpose(0, 2, 1), oh).transpose(0, 2, 1)
    K = p[4:13]
    acc = np.stack([sum(np.int64(K[3 * i + j]) * m[j] for j in range(3)) for i in range(3)])
    t = np.clip((acc + 32768) >> 16, 0, 4095)
    return dict(n=n, hm=hm, m=m, acc=acc, t=t, t16=_render.index16(acc))


def render(frame, p, ow: int, oh: int, lut=None, look=None, look16=None) -> np.ndarray:
    """(oh, ow, 3) uint8, R G B; look: step 4 with a look (mlvfs_amd/look.py) instead of the table; look16: the 16-bit rendering
    through a deep look, uint16"""
    return _render.develop(stages(frame, p, ow, oh), lut, look, look16)


def split_file(file, ow: int, oh: int) -> np.ndarray:
    """the pixels of one served file"""
    return _render.split_file(file, ow, oh)
