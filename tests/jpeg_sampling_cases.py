"""The chroma samplings of the rendered JPEG files (include/mlvfs_amd.h, "the chroma sampling of the JPEG files"): the
cases the CPU and GPU tests share for 4:2:2 and 4:4:4.  The definition itself is mlvfs_amd/jpeg.py; the contents are those of
tests/jpeg_cases.py and one more.  Shapes follow from each sampling's MCU and from the kernels' group and chunk constants, which are read
from csrc/jpeg.h.  tests/test_jpeg_sampling_cases.py proves that the cases are not vacuous."""
import functools
import os
import re

import numpy as np

from mlvfs_amd import jpeg

import jpeg_cases as jc

SAMPLINGS = (422, 444)                                    # the two this file adds; 420 is tests/jpeg_cases.py's
CODE = {s: jpeg.SAMPLINGS[s][4] for s in jpeg.SAMPLINGS}  # the C interface's number: MLVFS_AMD_JPEG_420, _422, _444
QUALITIES = jc.QUALITIES
assert QUALITIES == [1, 50, 75, 90, 100]


def _constants():
    """MCUs per workgroup of the transform kernel (JPG_GROUP*) and of the emit kernel (JPG_CHUNK*), per sampling, from csrc/jpeg.h"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "mlvfs_amd", "csrc", "jpeg.h")).read()
    value = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    return ({420: value("JPG_GROUP"), 422: value("JPG_GROUP_422"), 444: value("JPG_GROUP_444")},
            {420: value("JPG_CHUNK"), 422: value("JPG_CHUNK_422"), 444: value("JPG_CHUNK_444")})


GROUP, CHUNK = _constants()


def mcu(sampling):
    return jpeg.SAMPLINGS[sampling][:2]


def shapes(sampling):
    """(W', H') in the issue's order: one pixel, one MCU, one MCU plus one pixel on both axes, odd on both axes, a row whose last MCU is
    partly empty, two MCU rows, exactly one group of the transform kernel, one MCU more, one chunk of the emit kernel plus three MCUs (two
    workgroups share a dword), ten MCU rows (the RST index wraps), 13 x 9 MCUs"""
    w, h = mcu(sampling)
    g, c = GROUP[sampling], CHUNK[sampling]
    return [(1, 1), (w, h), (w + 1, h + 1), (2 * w - 1, 4 * h + 1), (w + w // 2, h), (2 * w + w // 2, h + h // 2), (g * w, h), (g * w + w, h),
            ((c + 3) * w - 4, h + 4), (w + 4, 10 * h - 2), (13 * w, 8 * h + h // 4)]


# the scans' thresholds, one quality each: 257 MCUs in a row (the row scan takes a second round of 256) and 1025 MCU rows (a thread of
# the scans across rows takes two)
LONG = {444: [(2056, 8), (8, 8200)], 422: [(4112, 8), (16, 8200)]}
# the issue's cross-check shapes, used for the PSNR as well
PINNED = [(17, 9), (40, 24), (100, 83), (208, 132)]


def chroma_steps(sampling):
    """blocks of one chrominance block's pixels each, alternating between blue and yellow (Cb 255 and 1) from block to block: chrominance
    DC differences of category 11 at quality 100"""
    w, h = mcu(sampling)

    def content(pw, ph, seed=0):
        y, x = np.mgrid[0:ph, 0:pw]
        blue = (((x // w) + (y // h) + seed) & 1).astype(bool)
        v = np.where(blue, 0, 255).astype(np.uint8)
        return np.stack([v, v, 255 - v], -1)
    content.__name__ = "chroma_steps"
    return content


def chroma_basis(sampling):
    """tests/jpeg_cases.py's basis in blue and yellow, on the chrominance blocks' grid: the largest coefficient a chrominance block can
    give at every position -- AC category 10 of the chrominance table at quality 100"""
    w, h = mcu(sampling)

    def content(pw, ph, seed=0):
        y, x = np.mgrid[0:ph, 0:pw]
        x, y = x // (w // 8), y // (h // 8)                   # in chrominance samples
        k = ((x // 8) * 5 + (y // 8) * 3 + 4 + seed) % 64
        sign = np.sign(jpeg.DCT_T)
        v = np.where(sign[k // 8, y % 8] * sign[k % 8, x % 8] > 0, 255, 0).astype(np.uint8)
        return np.stack([v, v, 255 - v], -1)
    content.__name__ = "chroma_basis"
    return content


CONTENT = {s: jc.CONTENT + (chroma_steps(s), chroma_basis(s)) for s in SAMPLINGS}


def all_cases(sampling):
    """[(W', H', content, quality)]"""
    return [(pw, ph, c, q) for pw, ph in shapes(sampling) for c in CONTENT[sampling] for q in QUALITIES]


@functools.lru_cache(maxsize=None)
def expected(sampling, pw, ph, content_index, quality, seed=0):
    """the yardstick's stream for a case, computed once and shared"""
    return jpeg.encode(CONTENT[sampling][content_index](pw, ph, seed), quality, None, sampling)


def batch(sampling, n, first=0):
    """n renderings of distinct content, cycling from `first` on: [(content index, seed)]"""
    return [((first + k) % len(CONTENT[sampling]), first + k) for k in range(n)]
