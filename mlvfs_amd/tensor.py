"""A clip's frames as device-resident tensors: the definition in numpy (include/mlvfs_amd.h, "a clip's frames as device-resident tensors";
csrc/k_tensor.hip computes it on the GPU).  Tests and tools share this file: it is what the GPU's results are held against.

    rgb(samples, bits, dtype, layout, scale, bias)       samples: (ph, pw, 3) uint8 or uint16, a rendering as a file route serves it
    bayer(px, black, white, dtype, layout, scale, bias)  px: (H, W) uint16, the frame mlvfs_amd_mount_dng serves, with its header's levels

Per element of channel c, v the sample (RGB) or px - black as a signed integer, clamped at neither end (Bayer):
    F32   y = fl32(fl32(fl32(v) * unit) * scale_c), out = fl32(y + bias_c) -- three operations, each rounded to binary32 on its own
    F16   that value converted by round-to-nearest-even (subnormal halves kept, overflow to infinity)
    BF16  that value converted by round-to-nearest-even, as bit arithmetic on the float's bits
    U8, U16   the sample itself (Bayer: the raw px); scale and bias are not read
unit = fl32(1 / 255), fl32(1 / 65535) or fl32(1.0 / max(white - black, 1)): the double quotient rounded once.
Results are returned as arrays of the element's bits (uint32 for F32, uint16 for F16, BF16 and U16, uint8 for U8), so that comparisons
are for equality of bits."""
from __future__ import annotations

import numpy as np

F32, F16, BF16, U8, U16 = 0, 1, 2, 3, 4
NCHW, NHWC = 0, 1
RGB, BAYER = 0, 1
HALF, FULL, SCALED, RESAMPLED = 0, 1, 2, 3
DTYPE_NAMES = {"float32": F32, "float16": F16, "bfloat16": BF16, "uint8": U8, "uint16": U16}
LAYOUTS = {"NCHW": NCHW, "NHWC": NHWC}
ELEM = {F32: 4, F16: 2, BF16: 2, U8: 1, U16: 2}
BITS_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8, U16: np.uint16}
FACTOR_MIN, FACTOR_MAX = 2.0 ** -64, 2.0 ** 64
BLACK_MAX = 1 << 30


def legal(dtype: int, src_bits: int) -> bool:
    """the float dtypes for every source; of the integer ones the source's own depth (Bayer: 16)"""
    return dtype in (F32, F16, BF16) or dtype == (U8 if src_bits == 8 else U16)


def factor_ok(x) -> bool:
    """a scale or a bias: finite, and zero or of magnitude within [2^-64, 2^64]"""
    x = float(np.float32(x))
    return bool(np.isfinite(x)) and (x == 0.0 or FACTOR_MIN <= abs(x) <= FACTOR_MAX)


def unit_of(bits: int) -> np.float32:
    return np.float32(1.0 / 255.0) if bits == 8 else np.float32(1.0 / 65535.0)


def bayer_levels(black: int, white: int):
    """-> (black, range, unit) as mlvfs_amd_tensor_bayer_params gives them"""
    if abs(int(black)) > BLACK_MAX:
        raise ValueError(f"a black level of {black} (|black| <= 2^30)")
    rng = max(int(white) - int(black), 1)
    return int(black), rng, np.float32(1.0 / float(rng))


def normalisation(mean, std, channels: int):
    """mean / std -> (scale, bias) as float32 arrays of 4: scale = 1 / std, bias = -mean / std, computed in double and rounded once"""
    def per_channel(v, default):
        a = np.full(channels, default, np.float64) if v is None else np.broadcast_to(np.asarray(v, np.float64), (channels,)).copy()
        return a
    m, s = per_channel(mean, 0.0), per_channel(std, 1.0)
    scale, bias = np.ones(4, np.float32), np.zeros(4, np.float32)
    scale[:channels] = (1.0 / s).astype(np.float32)
    bias[:channels] = (-m / s).astype(np.float32)
    return scale, bias


def f32_value(v: np.ndarray, unit, scale, bias) -> np.ndarray:
    """v: integers (..., C) -> float32 (..., C); every operation is numpy's float32 one, rounded on its own"""
    c = v.shape[-1]
    x = v.astype(np.int64).astype(np.float32)                       # exact below 2^24, round-to-nearest-even above
    x = x * np.float32(unit)
    y = x * np.asarray(scale, np.float32)[:c]
    return y + np.asarray(bias, np.float32)[:c]


def bf16_bits(f: np.ndarray) -> np.ndarray:
    """float32 -> the bfloat16's 16 bits, round-to-nearest-even on the float's bits (finite values)"""
    b = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def f16_bits(f: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(f, np.float32).astype(np.float16).view(np.uint16)


def element_bits(v: np.ndarray, raw: np.ndarray, dtype: int, unit, scale, bias) -> np.ndarray:
    if dtype in (U8, U16):
        return raw.astype(BITS_DTYPE[dtype])
    f = f32_value(v, unit, scale, bias)
    return f.view(np.uint32) if dtype == F32 else f16_bits(f) if dtype == F16 else bf16_bits(f)


def lay_out(e: np.ndarray, layout: int) -> np.ndarray:
    """(h, w, C) -> (C, h, w) for NCHW, as it is for NHWC"""
    return np.ascontiguousarray(e.transpose(2, 0, 1)) if layout == NCHW else np.ascontiguousarray(e)


def rgb(samples: np.ndarray, bits: int, dtype: int, layout: int, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0)) -> np.ndarray:
    if not legal(dtype, bits):
        raise ValueError(f"dtype {dtype} is illegal for a {bits}-bit source")
    s = np.asarray(samples)
    assert s.ndim == 3 and s.shape[2] == 3 and s.dtype == (np.uint8 if bits == 8 else np.uint16)
    return lay_out(element_bits(s.astype(np.int64), s, dtype, unit_of(bits), scale, bias), layout)


def bayer_planes(px: np.ndarray) -> np.ndarray:
    """(H, W) -> (H // 2, W // 2, 4): R, G1, G2, B; an odd last row or column is dropped"""
    h2, w2 = px.shape[0] // 2, px.shape[1] // 2
    p = px[:2 * h2, :2 * w2]
    return np.stack([p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]], axis=-1)


def bayer(px: np.ndarray, black: int, white: int, dtype: int, layout: int, scale=(1, 1, 1, 1), bias=(0, 0, 0, 0)) -> np.ndarray:
    if not legal(dtype, 16):
        raise ValueError(f"dtype {dtype} is illegal for a Bayer source")
    black, _, unit = bayer_levels(black, white)
    p = bayer_planes(np.asarray(px, np.uint16))
    return lay_out(element_bits(p.astype(np.int64) - black, p, dtype, unit, scale, bias), layout)


def shape_of(channels: int, h: int, w: int, layout: int):
    return (channels, h, w) if layout == NCHW else (h, w, channels)
