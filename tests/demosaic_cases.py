"""Rendered full-size sRGB frames (include/mlvfs_amd.h, "rendered full-size sRGB frames"): the cases the CPU and GPU
tests share.  The definition itself is mlvfs_amd/demosaic.py.  The parameter sets, levels and content generators are those of
tests/render_cases.py; this module adds frames and one parameter set of its own.  tests/test_demosaic_cases.py proves that the cases
are not vacuous."""
import numpy as np

from mlvfs_amd import render

import render_cases as rc

STRIP, RUN = 512, 32                     # k_render1_x16: the columns of a workgroup's strip and the rows it walks down (csrc/k_demosaic.hip)

# (width, height) for mlvfs_amd_render1_dev: the minimum, where every window reflects on two sides; odd sizes; one and two groups of
# 16 wide with an odd height; a width the fast form does not take; one group of 16 short of, equal to and one past the strip (the
# fast form takes multiples of 16), and the 8-pixel steps between them, which the generic form takes; one row short of, equal to
# and one past the run of rows; both at once with a second run that is one row long; exactly one strip and one wave per row with one
# lane more in a second strip; the mount tests' size
SIZES = [(4, 4), (5, 4), (4, 5), (7, 5), (6, 6), (16, 4), (32, 5), (48, 8), (30, 10),
         (STRIP - 16, 6), (STRIP - 8, 5), (STRIP, 6), (STRIP + 8, 5), (STRIP + 16, 6),
         (16, RUN - 1), (16, RUN), (16, RUN + 1), (STRIP + 16, 2 * RUN + 1),
         (1024, 6), (1040, 6), (416, 264)]
BIG_W, BIG_H = rc.BIG_W, rc.BIG_H
MOUNT_SIZES = rc.MOUNT_SIZES


def wide_param_set(k):
    """a forward matrix three times a camera's (its entries still fit the header's shorts) at a third of the gain: the rows of K
    fail sum_j |K[i][j]| * 65535 + 32768 < 2^31, so step 3 needs its 64 bits, and t still runs through its range"""
    black, white = rc.LEVELS[k % len(rc.LEVELS)]
    fm = tuple(3 * v for v in rc.FORWARD[k % len(rc.FORWARD)])
    return (black, white), render.params(black, white, rc.NEUTRALS[k % len(rc.NEUTRALS)], fm, 85)


def param_set(k):
    """the k-th set: every third is a wide one, so a batch of three holds a frame of each matrix path"""
    return wide_param_set(k) if k % 3 == 1 else rc.param_set(k)


# ---- content of this module's own
def speckle_frame(w, h, black, white, seed=0):
    """isolated extremes: single pixels at 0 and at the top of the range in a field of mid grey, and a mid-grey pixel in a field of
    extremes -- the negative lobes of every sum drive it below zero, the positive ones above 65535 after the balance"""
    g = np.random.default_rng(5000 + seed)
    lo, hi = max(black - 8, 0), min(white + 8, 65535)
    kind = g.integers(0, 5, (h, w))
    level = np.array([lo, hi, (lo + hi) // 2, lo + (hi - lo) // 4, hi - (hi - lo) // 4])[kind]
    return np.clip(level + g.integers(-3, 4, (h, w)), 0, 65535).astype(np.uint16)


def rim_frame(w, h, black, white, seed=0):
    """every one of the two outermost rows and columns unlike its neighbours, the interior noise: a reflection that takes the wrong
    row or column changes the sums along the whole border"""
    g = np.random.default_rng(6000 + seed)
    f = g.integers(black, min(white, 65535) + 1, (h, w)).astype(np.int64)
    span = max(min(white, 65535) - black, 4)
    y, x = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(y, h - 1 - y), np.minimum(x, w - 1 - x))
    f = np.where(d == 0, black + span // 8 + (x + y) % 5, f)
    f = np.where(d == 1, black + span - span // 8 - (x * 3 + y) % 7, f)
    f = np.where(d == 2, black + span // 2 + (x + 2 * y) % 3, f)
    return np.clip(f, 0, 65535).astype(np.uint16)


CONTENT = rc.CONTENT + (speckle_frame, rim_frame)


def batch(w, h, n, first=0):
    """n frames of distinct content and parameters, cycling from `first` on: [(frame, 13 parameters)]"""
    out = []
    for k in range(first, first + n):
        (black, white), p = param_set(k)
        out.append((CONTENT[k % len(CONTENT)](w, h, black, white, seed=k), p))
    return out


PLACEMENTS = rc.PLACEMENTS               # (frames, source offset, destination offset, aligned strides)


def dev_cases(w, h):
    """what tests/test_gpu_demosaic.py runs at one size: [(frames with parameters, src_off, dst_off, aligned)]"""
    out, first = [], (w * 7 + h) % 11          # sizes start at different places of the cycles
    for n, src_off, dst_off, aligned in PLACEMENTS:
        out.append((batch(w, h, n, first), src_off, dst_off, aligned))
        first += n
    return out


def flat_frame(w, h, r, g, b):
    """flat per CFA colour"""
    y, x = np.mgrid[0:h, 0:w]
    return np.array([r, g, b], np.uint16)[(y & 1) + (x & 1)]


params_array = rc.params_array
