"""Rendered full-size frames demosaiced by AMaZE (include/mlvfs_amd.h, "rendered full-size frames demosaiced by AMaZE"; DESIGN.md
3.19): the cases the CPU and GPU tests share.  The definition itself is mlvfs_amd/amaze_render.py; AMaZE is the checker's
(oracle.amaze_demosaic).  Frames and parameter sets come from tests/render_cases.py and tests/demosaic_cases.py.
tests/test_amaze_render_cases.py proves that the cases are not vacuous."""
import ctypes as C
import functools

import numpy as np

from mlvfs_amd import amaze_render, demosaic, lib

import demosaic_cases as dm
import render_cases as rc

# (width, height): one AMaZE tile, two and three across, two down (a tile advances by 128 pixels; the first starts 16 before the image)
SIZES = [(36, 36), (40, 38), (148, 40), (164, 148), (292, 36)]
# a width the fast forms of the two element-wise kernels take (a multiple of 16); none of the sizes above is one
FAST_SIZE = (48, 37)
BIG_W, BIG_H = rc.BIG_W, rc.BIG_H
CONTENT = (rc.range_frame, dm.speckle_frame)
NSETS = 3                                # demosaic_cases.param_set(0 .. 2); the second is a wide one (64-bit matrix)


@functools.lru_cache(maxsize=None)
def rows_size():
    """the smallest plane (by pixels, then by width) with one complete tile, which k_amaze_rows takes: found with
    mlvfs_amd_amaze_rows_extent (host code)"""
    L = lib.load()
    best = None
    for w in range(36, 420, 4):
        for h in range(36, 420):
            if best is not None and w * h >= best[0]:
                break
            a, b = C.c_int(-1), C.c_int(-1)
            L.mlvfs_amd_amaze_rows_extent(w, h, C.byref(a), C.byref(b))
            if a.value * b.value >= 1:
                best = (w * h, w, h, a.value, b.value)
                break
    assert best is not None
    return best[1:]


def wide_set():
    """one more set of the 64-bit matrix path, at other levels than param_set(1)"""
    return dm.wide_param_set(4)


def cases(sizes=SIZES):
    """[(w, h, frame, parameters, label)]: every size with both contents and the three parameter sets"""
    out = []
    for w, h in sizes:
        for c, content in enumerate(CONTENT):
            for k in range(NSETS):
                (black, white), p = dm.param_set(k)
                out.append((w, h, content(w, h, black, white), p, f"{w}x{h}:{content.__name__}:{k}"))
    return out


def batch(w, h, n, first=0):
    """n frames of alternating content, each with parameters of its own, cycling from `first` on; every fourth set is the extra wide one"""
    out = []
    for k in range(first, first + n):
        (black, white), p = wide_set() if k % 4 == 3 else dm.param_set(k % NSETS)
        out.append((CONTENT[k % 2](w, h, black, white, seed=100 + k), p))
    return out


# (frames, source offset, destination offset, aligned strides): the fast forms need both bases aligned
PLACEMENTS = [(1, 0, 0, True), (3, 0, 0, True), (3, 2, 1, False)]

# step 3 on crafted values: v -> n.  k + 0.5 is exact in binary32 and floors to k + 1; 65535.49 becomes 65535.4921875, whose sum
# 65535.9921875 is exact and floors to 65535; 0.49999997 is 0.5 - 2^-25, whose sum 1 - 2^-25 lies midway between 1 - 2^-24 and 1
# and rounds to the even one, 1.0: the definition's float32 sum gives 1
CRAFTED = [(float("nan"), 0), (float("inf"), 65535), (float("-inf"), 0), (-0.0, 0), (0.0, 0), (0.5, 1), (1.5, 2), (2.5, 3), (1000.5, 1001),
           (32767.5, 32768), (65534.5, 65535), (65535.49, 65535), (65535.5, 65535), (65535.0, 65535), (65536.0, 65535), (1e30, 65535),
           (-0.49, 0), (-1e30, 0), (0.49999997, 1), (0.49, 0), (0.4999999, 0), (1e-30, 0), (12345.25, 12345), (12345.75, 12346)]


def crafted_planes(w, h):
    """three float32 planes (H, W) that run through CRAFTED with a different phase each, and the n (3, H, W) they give"""
    v = np.array([c[0] for c in CRAFTED], np.float32)
    n = np.array([c[1] for c in CRAFTED], np.int64)
    i = np.arange(w * h).reshape(h, w)
    idx = np.stack([(i + i // w + 7 * c) % len(CRAFTED) for c in range(3)])
    return v[idx], n[idx]


# ---- wrong definitions the cases must tell from the right one: each gives n (3, H, W)
def variant_n(kind, frame, p, amaze):
    st = amaze_render.stages(frame, p, amaze)
    v = st["planes"]
    fin = np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=1e12, neginf=-1e12)
    if kind == "truncate":                                       # no rounding
        return np.floor(np.clip(fin, 0, 65535)).astype(np.int64)
    if kind == "no clamp":                                       # the matrix takes what AMaZE overshoots
        return np.floor(fin + 0.5).astype(np.int64)
    if kind == "swap":                                           # R and B exchanged
        return st["n"][::-1]
    if kind == "shift":                                          # AMaZE reads the CFA one column off
        planes = [np.roll(c, -1, axis=1) for c in amaze(np.roll(st["raw"], 1, axis=1))]
        return amaze_render.sample16(np.stack(planes))
    if kind == "unit":                                           # raw scaled to 0 .. 1, the planes scaled back
        planes = np.stack(amaze(st["raw"] / np.float32(65535))) * np.float32(65535)
        return amaze_render.sample16(planes)
    raise ValueError(kind)


VARIANTS = ("truncate", "no clamp", "swap", "shift", "unit")


def matrix(p, n):
    """steps 3 of the renderings on any n: t and t16"""
    K = [int(v) for v in p[4:13]]
    acc = np.stack([sum(np.int64(K[3 * i + k]) * n[k] for k in range(3)) for i in range(3)])
    from mlvfs_amd import render
    return np.clip((acc + 32768) >> 16, 0, 4095), render.index16(acc)


params_array = rc.params_array
matrix_fits_32 = demosaic.matrix_fits_32
