"""Resampled rendered frames demosaiced by AMaZE (include/mlvfs_amd.h, "resampled rendered frames demosaiced by AMaZE"; DESIGN.md
3.20): the cases the CPU and GPU tests share.  The definition itself is mlvfs_amd/amaze_resample.py; AMaZE is the checker's
(oracle.amaze_demosaic).  The sources are those of tests/amaze_render_cases.py and four more that the fast form's plan needs; every
source goes to the sizes of out_sizes().  tests/test_amaze_resample_cases.py proves that the cases are not vacuous."""
import ctypes as C

import numpy as np

from mlvfs_amd import amaze_render, lib, resample, scale

import amaze_render_cases as ac
import demosaic_cases as dm

# (width, height): a fast-form width (a multiple of 8) in one strip and one band; two strips; a band seam; many bands
ADDED = [(48, 37), (528, 36), (48, 70), (48, 600)]
SOURCES = ac.SIZES + ADDED
BIG_W, BIG_H = ac.BIG_W, ac.BIG_H
BIG_SIZE = (1920, 707)


def out_sizes(w, h):
    """the identity, one less, just above the half, two thirds, a third of the rows alone, one row, one column, one pixel, and a
    third of both (2 ow < W: the generic form alone) -- without repeats, in that order"""
    out = []
    for s in [(w, h), (w - 1, h - 1), (w // 2 + 1, h // 2 + 1), (2 * w // 3 + 1, 2 * h // 3 + 1), (w, -(-h // 3)), (w, 1), (1, h), (1, 1),
              (w // 3, h // 3)]:
        if s not in out:
            out.append(s)
    return out


def cases():
    """[(w, h, frame, parameters, label)]: amaze_render_cases.cases() and the added sources, each of those with both contents -- the
    first with a 32-bit matrix set, the second with the wide one"""
    out = list(ac.cases())
    for w, h in ADDED:
        for c, content in enumerate(ac.CONTENT):
            (black, white), p = dm.param_set(c)
            out.append((w, h, content(w, h, black, white), p, f"{w}x{h}:{content.__name__}:{c}"))
    return out


def plan(L, w, h, ow, oh, nframes=1):
    """mlvfs_amd_test_amz_resample_plan as a dict (host code)"""
    out = np.full(8, -7, np.int32)
    lib.check(L.mlvfs_amd_test_amz_resample_plan(w, h, ow, oh, nframes, lib.ptr(out)), "test_amz_resample_plan")
    return dict(zip(("fast", "strip", "uo", "nstrips", "bo", "nbands", "band_rows", "rows"), (int(v) for v in out)))


def takes_fast(w, ow):
    """the width rule of k_amz_resample_x16, restated"""
    return w % 8 == 0 and 2 * ow >= w


# ---- wrong definitions the cases must tell from the right one: each gives m (3, oh, ow) from the AMaZE stages of a case
def both_passes(n, ow, oh):
    hd = scale.average(n, ow)
    return scale.average(hd.transpose(0, 2, 1), oh).transpose(0, 2, 1)


def _weights(n_src, n_out):
    """(n_out, n_src) overlaps of the definition, as integers"""
    u = np.arange(n_out, dtype=np.int64)[:, None]
    x = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((x + 1) * n_out, (u + 1) * n_src) - np.maximum(x * n_out, u * n_src))


def variant_m(kind, frame, p, st, ow, oh):
    """st: amaze_render.stages of the case"""
    v = st["planes"]
    fin = np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=1e12, neginf=-1e12)
    h, w = frame.shape
    if kind == "linear":                                         # the linear resampled rendering
        return resample.stages(frame, p, ow, oh)["m"]
    if kind == "float average":                                  # the clamped float planes averaged, rounded once
        c = np.clip(fin, 0, 65535)
        wx, wy = _weights(w, ow).astype(np.float64), _weights(h, oh).astype(np.float64)
        return np.floor(wy @ (c @ wx.T) / (w * h) + 0.5).astype(np.int64)
    if kind == "truncate":                                       # no rounding in step 3
        return both_passes(np.floor(np.clip(fin, 0, 65535)).astype(np.int64), ow, oh)
    if kind == "no clamp":                                       # the average takes what AMaZE overshoots (signed, floored)
        n = np.floor(fin + 0.5).astype(np.int64)
        hd = (n @ _weights(w, ow).T + (w >> 1)) // w
        return (_weights(h, oh) @ hd + (h >> 1)) // h
    if kind == "vertical first":
        vd = scale.average(st["n"].transpose(0, 2, 1), oh).transpose(0, 2, 1)
        return scale.average(vd, ow)
    if kind == "swap":                                           # R and B exchanged
        return both_passes(st["n"], ow, oh)[::-1]
    raise ValueError(kind)


VARIANTS = ("linear", "float average", "truncate", "no clamp", "vertical first", "swap")

matrix = ac.matrix
params_array = ac.params_array
matrix_fits_32 = ac.matrix_fits_32
crafted_planes = ac.crafted_planes
batch = ac.batch
wide_set = ac.wide_set
