"""Rendered frames as baseline JPEG files (include/mlvfs_amd.h, "rendered frames as baseline JPEG files"): the cases
the CPU and GPU tests share.  The definition itself is mlvfs_amd/jpeg.py.  tests/test_jpeg_cases.py proves that the cases are not
vacuous."""
import functools

import numpy as np

from mlvfs_amd import jpeg

# rendering shapes as (W', H'): one pixel, one block, one MCU, one pixel more on both axes, odd on both axes, a row of MCUs whose last is
# half empty, more than one MCU row, four MCUs (a whole group of the transform kernel), ten MCU rows (the RST index wraps), and 13 x 9 MCUs
SHAPES = [(1, 1), (8, 8), (16, 16), (17, 17), (15, 33), (24, 8), (40, 24), (64, 16), (20, 150), (208, 132)]
# a row of 19 MCUs: two workgroups of the emit kernel (16 MCUs each) share a dword
WIDE = (300, 20)
# the kernels' other thresholds, one quality each: 257 MCUs a row (the row scan takes a second round of 256), 1025 MCU rows (a thread
# of the scans across rows takes two)
LONG = [(4112, 8), (8, 16400)]
QUALITIES = [1, 50, 75, 90, 100]
BIG = (1792, 660)


def flat(pw, ph, seed=0):
    return np.full((ph, pw, 3), (40 + 50 * seed) & 255, np.uint8)


def formula(pw, ph, seed=0):
    """the issue's cross-check image"""
    y, x = np.mgrid[0:ph, 0:pw]
    x = x + 3 * seed
    return np.stack([(7 * x + 3 * y) & 255, (x * y + 5 * x) & 255, 255 - ((11 * y + x * x) & 255)], -1).astype(np.uint8)


def gradient(pw, ph, seed=0):
    y, x = np.mgrid[0:ph, 0:pw]
    d = max(pw + ph - 2, 1)
    return np.stack([255 * x // max(pw - 1, 1), 255 * y // max(ph - 1, 1), 255 - 255 * (x + y) // d], -1).astype(np.uint8) ^ np.uint8(seed)


def noise(pw, ph, seed=0):
    return np.random.default_rng(500 + seed).integers(0, 256, (ph, pw, 3), dtype=np.uint8)


def primaries(pw, ph, seed=0):
    """a checkerboard of saturated primaries and their complements: Cb and Cr at both clamps, large AC values"""
    y, x = np.mgrid[0:ph, 0:pw]
    which = (x + y * 3 + seed) % 8
    return np.stack([np.where(which & 1, 255, 0), np.where(which & 2, 255, 0), np.where(which & 4, 255, 0)], -1).astype(np.uint8)


def block_steps(pw, ph, seed=0):
    """8 x 8 blocks whose means alternate between 0 and 255: DC differences of category 11 at quality 100"""
    y, x = np.mgrid[0:ph, 0:pw]
    v = np.where(((x // 8) + (y // 8) + seed) & 1, 255, 0).astype(np.uint8)
    return np.stack([v, v, v], -1)


def basis(pw, ph, seed=0):
    """grey 8 x 8 blocks of 0 and 255 in the sign pattern of one DCT basis function each, (v, u) cycling from block to block: the
    largest coefficient an 8-bit block can give at every position -- AC category 10 at quality 100"""
    y, x = np.mgrid[0:ph, 0:pw]
    k = ((x // 8) * 5 + (y // 8) * 3 + 4 + seed) % 64                 # block (0, 0): v = 0, u = 4
    sign = np.sign(jpeg.DCT_T)
    v = np.where(sign[k // 8, y % 8] * sign[k % 8, x % 8] > 0, 255, 0).astype(np.uint8)
    return np.stack([v, v, v], -1)


CONTENT = (flat, formula, gradient, noise, primaries, block_steps, basis)
SMOOTH = (formula, gradient, noise)                       # the contents whose PSNR is compared with PIL's encoder


def all_cases():
    """[(W', H', content, quality)]"""
    return [(pw, ph, c, q) for pw, ph in SHAPES + [WIDE] for c in CONTENT for q in QUALITIES]


@functools.lru_cache(maxsize=None)
def expected(pw, ph, content_index, quality, seed=0):
    """the oracle's stream for a case, computed once and shared"""
    return jpeg.encode(CONTENT[content_index](pw, ph, seed), quality)


def batch(pw, ph, n, first=0):
    """n renderings of distinct content, cycling from `first` on: [(content index, seed)]"""
    return [((first + k) % len(CONTENT), first + k) for k in range(n)]
