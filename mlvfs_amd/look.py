"""A look for the rendered frames: the definition of include/mlvfs_amd.h ("a look for the rendered frames") restated in
numpy integers, the handle of the library's side, and the way from a .cube file to the integers both take.  The tests and the tools
share apply() as the yardstick; nothing in it runs on a GPU and no floating point takes part.

    n, table = look.read_cube("grade.cube")                    # exact: decimals -> Fractions -> 16 bits
    S = look.shaper_srgb()                                     # what the table's input axis means: sRGB, linear, or log2 over some stops
    rgb = render.render(frame_u16, p, look=(S, n, table))      # likewise demosaic.render, scale.render
    with look.Look(S, n, table) as lk:                         # the same on the GPU
        mount.set_look(lk)

A look is (S, N, T): S 4096 uint16, N 2 .. 65, T (N^3, 3) uint16 indexed (b N + g) N + r -- red fastest, the order of a .cube file.

A deep look (S16, N, T) is the 16-bit routes' ("rendered frames at 16 bits"): S16 65536 uint16 on the 16-bit index, N 0 or
2 .. 65 (0: no table, T absent), 16-bit samples out and no step 4d -- stages16, apply16, image16, Look16 and the shaper16_* functions.

    rgb16 = render.render(frame_u16, p, look16=(look.shaper16_log2(12), 0, None))     # (H // 2, W // 2, 3) uint16
    with look.Look16(look.shaper16_srgb(), n, table) as lk:
        files = mount.rgb(0, 16, look16=lk)                                             # 16-bit TIFF files
"""
from __future__ import annotations

import ctypes as C
import re
from fractions import Fraction

import numpy as np

N_MIN, N_MAX = 2, 65
SHAPER_BYTES = 4096 * 2


def _look(shaper, n: int, table) -> tuple[np.ndarray, int, np.ndarray]:
    S = np.ascontiguousarray(shaper, np.uint16)
    n = int(n)
    if not N_MIN <= n <= N_MAX:
        raise ValueError(f"a table of {n} a side ({N_MIN} .. {N_MAX})")
    T = np.ascontiguousarray(table, np.uint16)
    if S.shape != (4096,) or T.size != 3 * n ** 3:
        raise ValueError(f"a look takes a shaper of 4096 values and a table of {n}^3 x 3, not {S.shape} and {T.shape}")
    return S, n, T.reshape(n ** 3, 3)


def stages(t, shaper, n: int, table, axis: int = 0, prefer=(0, 1, 2)) -> dict:
    """every intermediate of step 4 as int64 arrays with the channel axis in front: u, i, f (3, ...); order (3, ...): the axes a, b, c
    with f_a >= f_b >= f_c; w (4, ...); v, out (3, ...).  t: 12-bit indices (masked), its axis `axis` of length 3 is r, g, b.
    prefer: which axis comes first among equal fractions -- any permutation gives the same v (the tests show it)."""
    S, n, T = _look(shaper, n, table)
    t = np.moveaxis(np.asarray(t).astype(np.int64) & 4095, axis, 0)
    assert t.shape[0] == 3
    u = S.astype(np.int64)[t]                                                       # 4a
    p = u * (n - 1)                                                                 # 4b
    i, f = p >> 16, p & 65535
    assert i.max(initial=0) <= n - 2
    rank = np.empty(3, np.int64)
    rank[list(prefer)] = np.arange(3)
    order = np.argsort(-f * 4 + rank.reshape((3,) + (1,) * (t.ndim - 1)), axis=0, kind="stable")
    fs = np.take_along_axis(f, order, 0)                                            # f_a >= f_b >= f_c
    stride = np.array([1, n, n * n], np.int64)
    base = (i[2] * n + i[1]) * n + i[0]
    at = [base, base + stride[order[0]], base + stride[order[0]] + stride[order[1]], base + 1 + n + n * n]
    w = np.stack([65536 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]])
    Tl = T.astype(np.int64)
    acc = sum(w[j][..., None] * Tl[at[j]] for j in range(4)) + 32768                # (..., 3), 64 bits
    assert acc.max(initial=0) < 1 << 32
    v = np.moveaxis(acc >> 16, -1, 0)                                               # 4c
    out = (v + 128) // 257                                                          # 4d
    return dict(u=u, i=i, f=f, order=order, w=w, v=v, out=out)


def apply(t, shaper, n: int, table, axis: int = 0) -> np.ndarray:
    """step 4 with the look: uint8 of t's shape"""
    return np.moveaxis(stages(t, shaper, n, table, axis)["out"], 0, axis).astype(np.uint8)


def image(shaper, n: int, table) -> bytes:
    """the device image mlvfs_amd_look_pack writes: S, then the entries as R, G, B, 0"""
    S, n, T = _look(shaper, n, table)
    e = np.zeros((n ** 3, 4), "<u2")
    e[:, :3] = T
    return S.astype("<u2").tobytes() + e.tobytes()


def identity(n: int) -> np.ndarray:
    """T[g] = floor((2 * 65535 g + (N - 1)) / (2 (N - 1))) per axis: (N^3, 3) uint16"""
    if not N_MIN <= n <= N_MAX:
        raise ValueError(f"a table of {n} a side ({N_MIN} .. {N_MAX})")
    g = (2 * 65535 * np.arange(n, dtype=np.int64) + (n - 1)) // (2 * (n - 1))
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([r, gg, b], -1).reshape(n ** 3, 3).astype(np.uint16)


def shaper_srgb() -> np.ndarray:
    """257 * LUT: the table's input axis is the sRGB byte the plain rendering would write"""
    from . import render
    return (257 * render.srgb_lut12().astype(np.int64)).astype(np.uint16)


def shaper_linear() -> np.ndarray:
    t = np.arange(4096, dtype=np.int64)
    return ((t * 65535 + 2047) // 4095).astype(np.uint16)


def shaper_log2(stops: float) -> np.ndarray:
    """round(65535 * max(0, 1 + log2(max(t / 4095, 2^-stops)) / stops)): `stops` below white is 0.  Float, here only: data to the library"""
    if not stops > 0:
        raise ValueError("stops must be positive")
    x = np.maximum(np.arange(4096, dtype=np.float64) / 4095.0, 2.0 ** -stops)
    return np.floor(65535.0 * np.maximum(0.0, 1.0 + np.log2(x) / stops) + 0.5).astype(np.uint16)


def shaper(name: str) -> np.ndarray:
    """srgb | linear | log2:STOPS"""
    if name == "srgb":
        return shaper_srgb()
    if name == "linear":
        return shaper_linear()
    if name.startswith("log2:"):
        return shaper_log2(float(name[5:]))
    raise ValueError(f"a shaper is srgb, linear or log2:STOPS, not {name!r}")


# ---- the deep look of the 16-bit routes

def _look16(shaper16, n: int = 0, table=None) -> tuple[np.ndarray, int, np.ndarray]:
    S = np.ascontiguousarray(shaper16, np.uint16)
    n = int(n)
    if n != 0 and not N_MIN <= n <= N_MAX:
        raise ValueError(f"a table of {n} a side (0, or {N_MIN} .. {N_MAX})")
    if n and table is None:
        raise ValueError(f"a deep look with n = {n} takes a table")
    T = np.zeros((0, 3), np.uint16) if n == 0 else np.ascontiguousarray(table, np.uint16)
    if S.shape != (65536,) or T.size != 3 * n ** 3:
        raise ValueError(f"a deep look takes a shaper of 65536 values and a table of {n}^3 x 3, not {S.shape} and {T.shape}")
    return S, n, T.reshape(n ** 3, 3)


def stages16(t, shaper16, n: int = 0, table=None, axis: int = 0) -> dict:
    """every intermediate of the 16-bit step 4 as int64 arrays with the channel axis in front: u (3, ...), out (3, ...), and with a table
    i, f, order, w, v as stages() gives them (out is v: there is no step 4d).  t: 16-bit indices, its axis `axis` of length 3 is r, g, b."""
    S, n, T = _look16(shaper16, n, table)
    t = np.moveaxis(np.asarray(t).astype(np.int64), axis, 0)
    assert t.shape[0] == 3 and t.min(initial=0) >= 0 and t.max(initial=0) <= 65535
    u = S.astype(np.int64)[t]                                                       # 4a
    if n == 0:
        return dict(u=u, out=u)
    p = u * (n - 1)                                                                 # 4b
    i, f = p >> 16, p & 65535
    assert i.max(initial=0) <= n - 2
    order = np.argsort(-f * 4 + np.arange(3).reshape((3,) + (1,) * (t.ndim - 1)), axis=0, kind="stable")
    fs = np.take_along_axis(f, order, 0)                                            # f_a >= f_b >= f_c
    stride = np.array([1, n, n * n], np.int64)
    base = (i[2] * n + i[1]) * n + i[0]
    at = [base, base + stride[order[0]], base + stride[order[0]] + stride[order[1]], base + 1 + n + n * n]
    w = np.stack([65536 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]])
    Tl = T.astype(np.int64)
    acc = sum(w[j][..., None] * Tl[at[j]] for j in range(4)) + 32768                # (..., 3), 64 bits
    assert acc.max(initial=0) < 1 << 32
    v = np.moveaxis(acc >> 16, -1, 0)                                               # 4c
    return dict(u=u, i=i, f=f, order=order, w=w, v=v, out=v)


def apply16(t, shaper16, n: int = 0, table=None, axis: int = 0) -> np.ndarray:
    """step 4 of the 16-bit routes: uint16 of t's shape"""
    return np.moveaxis(stages16(t, shaper16, n, table, axis)["out"], 0, axis).astype(np.uint16)


def image16(shaper16, n: int = 0, table=None) -> bytes:
    """the device image mlvfs_amd_look16_pack writes: S16, then the entries as R, G, B, 0"""
    S, n, T = _look16(shaper16, n, table)
    e = np.zeros((n ** 3, 4), "<u2")
    e[:, :3] = T
    return S.astype("<u2").tobytes() + e.tobytes()


def shaper16_linear() -> np.ndarray:
    """the identity: the file holds t itself, a linear 16-bit TIFF"""
    return np.arange(65536, dtype=np.uint16)


def shaper16_srgb() -> np.ndarray:
    """round(65535 * oetf(t / 65535)) in float64.  Here only: data to the library (tests/test_deep_cases.py pins all 65536 entries in
    integers)"""
    x = np.arange(65536, dtype=np.float64) / 65535.0
    return np.floor(65535.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055) + 0.5).astype(np.uint16)


def shaper16_log2(stops: float) -> np.ndarray:
    """round(65535 * max(0, 1 + log2(max(t / 65535, 2^-stops)) / stops)): `stops` below white is 0.  Float, here only"""
    if not stops > 0:
        raise ValueError("stops must be positive")
    x = np.maximum(np.arange(65536, dtype=np.float64) / 65535.0, 2.0 ** -stops)
    return np.floor(65535.0 * np.maximum(0.0, 1.0 + np.log2(x) / stops) + 0.5).astype(np.uint16)


def shaper16(name: str) -> np.ndarray:
    """srgb | linear | log2:STOPS"""
    if name == "srgb":
        return shaper16_srgb()
    if name == "linear":
        return shaper16_linear()
    if name.startswith("log2:"):
        return shaper16_log2(float(name[5:]))
    raise ValueError(f"a shaper is srgb, linear or log2:STOPS, not {name!r}")


def quantise(v: Fraction) -> int:
    """q = clamp(floor(v * 65535 + 1/2), 0, 65535)"""
    return min(max((v * 65535 + Fraction(1, 2)).__floor__(), 0), 65535)


_DECIMAL = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")


def _decimal(word: str) -> Fraction:
    """the exact value of a decimal number as a .cube file writes it"""
    if not _DECIMAL.match(word):
        raise ValueError(f"{word!r} is not a decimal number")
    return Fraction(word)


def parse_cube(text: str) -> tuple[int, np.ndarray]:
    """(n, table) of a .cube file's text: LUT_3D_SIZE, an optional TITLE, # comments and blank lines, DOMAIN_MIN 0 0 0 and DOMAIN_MAX
    1 1 1 only; N^3 rows of three decimals, red fastest, each taken as an exact Fraction.  ValueError for anything else."""
    n, rows = None, []
    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        word = line.split()[0]
        if word == "TITLE":
            continue
        if word == "LUT_3D_SIZE":
            if n is not None or len(line.split()) != 2:
                raise ValueError(f"line {ln}: a second or malformed LUT_3D_SIZE")
            try:
                n = int(line.split()[1])
            except ValueError:
                raise ValueError(f"line {ln}: LUT_3D_SIZE {line.split()[1]!r}") from None
            if not N_MIN <= n <= N_MAX:
                raise ValueError(f"line {ln}: a table of {n} a side ({N_MIN} .. {N_MAX})")
            continue
        if word in ("DOMAIN_MIN", "DOMAIN_MAX"):
            try:
                vals = [_decimal(x) for x in line.split()[1:]]
            except ValueError:
                raise ValueError(f"line {ln}: {line!r}") from None
            if vals != [Fraction(0 if word == "DOMAIN_MIN" else 1)] * 3:
                raise ValueError(f"line {ln}: only the domain 0 .. 1 is taken, not {line!r}")
            continue
        if word[0].isalpha() or word[0] == "_":
            raise ValueError(f"line {ln}: {word} is not taken (a 3D table over 0 .. 1 only)")
        try:
            vals = [_decimal(x) for x in line.split()]
        except ValueError:
            raise ValueError(f"line {ln}: {line!r}") from None
        if len(vals) != 3:
            raise ValueError(f"line {ln}: a row has three values, not {len(vals)}")
        rows.append([quantise(v) for v in vals])
    if n is None:
        raise ValueError("no LUT_3D_SIZE")
    if len(rows) != n ** 3:
        raise ValueError(f"{len(rows)} rows, LUT_3D_SIZE {n} takes {n ** 3}")
    return n, np.array(rows, np.uint16)


def read_cube(path) -> tuple[int, np.ndarray]:
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        return parse_cube(f.read())


class Look:
    """The look on the GPU (mlvfs_amd_look_create): packed, uploaded once, independent of any mount.  It must stay open while a mount
    or a call uses it."""

    def __init__(self, shaper, n: int, table):
        from . import lib
        self.shaper, self.n, self.table = _look(shaper, n, table)
        self.L = lib.load()
        self.h = self.L.mlvfs_amd_look_create(lib.ptr(self.shaper), self.n, lib.ptr(self.table))
        if not self.h:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())

    def apply(self, t, axis: int = 0) -> np.ndarray:
        """the definition on the host, for comparisons"""
        return apply(t, self.shaper, self.n, self.table, axis)

    def close(self) -> None:
        if self.h:
            self.L.mlvfs_amd_look_destroy(C.c_void_p(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Look16:
    """The deep look on the GPU (mlvfs_amd_look16_create), with the lifetime rules of Look: it must stay open while a call uses it."""

    def __init__(self, shaper16, n: int = 0, table=None):
        from . import lib
        self.shaper, self.n, self.table = _look16(shaper16, n, table)
        self.L = lib.load()
        self.h = self.L.mlvfs_amd_look16_create(lib.ptr(self.shaper), self.n, lib.ptr(self.table) if self.n else None)
        if not self.h:
            raise lib.MlvfsAmdError(self.L.mlvfs_amd_last_error().decode())

    def apply(self, t, axis: int = 0) -> np.ndarray:
        """the definition on the host, for comparisons"""
        return apply16(t, self.shaper, self.n, self.table, axis)

    def close(self) -> None:
        if self.h:
            self.L.mlvfs_amd_look16_destroy(C.c_void_p(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def as_tuple16(look16) -> tuple[np.ndarray, int, np.ndarray]:
    """(S16, n, T) of a Look16 or of such a tuple: what render(..., look16=) takes"""
    if isinstance(look16, Look16):
        return look16.shaper, look16.n, look16.table
    return _look16(*look16)


def as_tuple(look) -> tuple[np.ndarray, int, np.ndarray]:
    """(S, n, T) of a Look or of such a tuple: what render(..., look=) takes"""
    if isinstance(look, Look):
        return look.shaper, look.n, look.table
    return _look(*look)
