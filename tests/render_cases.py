"""Rendered half-size sRGB frames (include/mlvfs_amd.h, "rendered half-size sRGB frames"): the cases the CPU and GPU
tests share.  The definition itself is mlvfs_amd/render.py.  tests/test_render_cases.py proves that the cases are not vacuous."""
import numpy as np

from mlvfs_amd import render

# (width, height) for mlvfs_amd_render2_dev: the smallest frame, a second superpixel, odd sizes that drop a column and a row, the
# smallest fast shapes (a width that is a multiple of 16), more than one superpixel row, a width the fast form does not take, exactly
# one wave per row of 16-pixel groups (1024 / 16 = 64 lanes), one lane more, and the mount tests' size
SIZES = [(2, 2), (4, 2), (6, 6), (7, 5), (16, 4), (32, 2), (48, 4), (30, 10), (1024, 4), (1040, 4), (416, 264)]
BIG_W, BIG_H = 3584, 1320
MOUNT_SIZES = [(64, 48), (418, 266)]               # the second drops nothing but is no multiple of 16: the generic form in the mount

# (black, white): 10-, 12-, 14- and 16-bit clips, and the x4 levels a dual-ISO conversion leaves (of a 14- and of a 16-bit clip)
LEVELS = [(128, 1000), (512, 4000), (2048, 15000), (8000, 65000), (8192, 60000), (32000, 260000)]

# ForwardMatrix2 of three camera rows (csrc/dngheader.cpp: 5D Mark III, 5D Mark II, 50D), over 10000
FORWARD = [(7637, 805, 1201, 2649, 9179, -1828, 137, -2456, 10570),
           (8924, -1041, 1760, 4351, 6621, -972, 505, -1562, 9308),
           (9485, -1150, 1308, 4313, 7807, -2120, 293, -2826, 10785)]

# AsShotNeutral as num, den per channel: daylight as the Kelvin path writes it, a custom balance, unity, tungsten-like
NEUTRALS = [(1000000, 2105347, 1000000, 1000000, 1000000, 1532101),
            (1024, 2200, 1024, 1024, 1024, 1700),
            (1, 1, 1, 1, 1, 1),
            (1000000, 1403112, 1000000, 1000000, 1000000, 2711030)]
GAINS = [256, 1024, 100, 300]


def param_set(k):
    """the k-th combination of levels, matrix, neutral and gain: (black, white), 13 parameters"""
    black, white = LEVELS[k % len(LEVELS)]
    p = render.params(black, white, NEUTRALS[k % len(NEUTRALS)], FORWARD[k % len(FORWARD)], GAINS[(k // 2) % len(GAINS)])
    return (black, white), p


# ---- content
def range_frame(w, h, black, white, seed=0):
    """a little below black up to a little above white, every parity of the green sum"""
    return np.random.default_rng(2000 + seed).integers(max(black - 64, 0), min(white + 64, 65535) + 1, (h, w), dtype=np.uint16)


def full_frame(w, h, black, white, seed=0):
    """the whole 16-bit range: most pixels clip at the min of step 2"""
    return np.random.default_rng(3000 + seed).integers(0, 65536, (h, w), dtype=np.uint16)


def dark_frame(w, h, black, white, seed=0):
    """mostly below black: the clamp of step 1"""
    return np.random.default_rng(4000 + seed).integers(0, black + 17, (h, w), dtype=np.uint16)


def grey_ramp(w, h, black, white, seed=0):
    """a neutral ramp by position from black to white (what the camera sees of a grey wedge: each channel at its neutral's share), so
    t runs through its range; any swap of rows or columns shows"""
    y, x = np.mgrid[0:h, 0:w]
    pos = ((y // 2) * (w // 2) + x // 2) * 37 % 1021 / 1020.0
    neutral = np.array([[0.47, 1.0], [1.0, 0.65]])[y & 1, x & 1]
    return np.minimum(black + pos * neutral * (white - black), 65535).astype(np.uint16)


def primaries(w, h, black, white, seed=0):
    """superpixels of one saturated channel, of two, of all and of none: the negative matrix entries drive acc below 0, the sums of
    a row above 4095"""
    y, x = np.mgrid[0:h, 0:w]
    which = ((y // 2) * 3 + x // 2) % 8                               # bit 0: red, bit 1: green, bit 2: blue
    chan = np.array([[1, 2], [2, 4]])[y & 1, x & 1]
    return np.where(which & chan, min(white, 65535), black).astype(np.uint16)


CONTENT = (range_frame, full_frame, grey_ramp, primaries, dark_frame)


def batch(w, h, n, first=0):
    """n frames of distinct content and parameters, cycling from `first` on: [(frame, 13 parameters)]"""
    out = []
    for k in range(first, first + n):
        (black, white), p = param_set(k)
        out.append((CONTENT[k % len(CONTENT)](w, h, black, white, seed=k), p))
    return out


# (frames, source offset, destination offset, aligned strides): both forms at shapes either could take
PLACEMENTS = [(1, 0, 0, True), (3, 0, 0, True), (3, 2, 0, False), (1, 0, 1, False), (3, 16, 8, True), (3, 2, 3, False)]


def dev_cases(w, h):
    """what tests/test_gpu_render.py runs at one size: [(frames with parameters, src_off, dst_off, aligned)]"""
    out, first = [], 0
    for n, src_off, dst_off, aligned in PLACEMENTS:
        out.append((batch(w, h, n, first), src_off, dst_off, aligned))
        first += n
    return out


def params_array(ps):
    return np.ascontiguousarray(np.array(ps, np.int64).astype(np.int32).reshape(-1, 13))
