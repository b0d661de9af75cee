"""Flat fields (mlvfs_amd_flat_*, csrc/cal.cpp, csrc/k_cal.hip): gain correction against a clip of an evenly lit target -- vignetting,
dust shadows, per-pixel and per-column gain -- applied on the GPU directly after the dark frame and before any other stage.

    s[p]    = max(F[p] - black_f, 1)                                black_f: the black level of the clip F was averaged from
    M_c     = (sum of s[p] over channel c + n_c // 2) // n_c        c = (y & 1) * 2 + (x & 1)
    gain[p] = min((M_c * 16384 + s[p] // 2) // s[p], 65535)         Q14; gains stop just under 4.0
    out     = clamp(black + ((px - black) * gain[p] + 8192 >> 14), 0, 2^bpp - 1)        the frame's own black level and depth

    with mlvfile.MlvReader("DARK.MLV") as dr, Dark.from_clip(dr) as dark, mlvfile.MlvReader("FLAT.MLV") as fr, \
            Flat.from_clip(fr, dark=dark) as flat, mlvfile.MlvReader("M07-1234.MLV") as r:
        with Mount(r, MlvfsOptions(chroma_smooth=5), dark=dark, flat=flat) as m:
            files = m.dng(0, 16)
        r.transcode("OUT.MLV", lj92=True, dark=dark, flat=flat)

A gain plane has no depth: a flat shot at 14 bits corrects a 12- or 10-bit clip of the same size.  A Flat must outlive the mounts
that use it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib


class Flat:
    def __init__(self, handle):
        self.L = lib.load()
        self.h = handle

    @classmethod
    def from_plane(cls, plane: np.ndarray, bpp: int, black: int) -> "Flat":
        """plane: (height, width) uint16, the flat plane F; black: its pedestal black_f.  Host code: needs no GPU."""
        L = lib.load()
        if not (isinstance(plane, np.ndarray) and plane.ndim == 2 and plane.dtype == np.uint16):
            raise ValueError("a flat plane is a (height, width) uint16 array")
        p = np.ascontiguousarray(plane)
        geom = lib.Geom(p.shape[1], p.shape[0], bpp, black, 0, 0, 0)
        h = L.mlvfs_amd_flat_create(C.byref(geom), lib.ptr(p))
        if not h:
            raise lib.MlvfsAmdError("flat_create failed: " + L.mlvfs_amd_last_error().decode())
        return cls(h)

    @classmethod
    def from_clip(cls, reader, first: int = 0, count: int | None = None, dark=None, batch: int = 0, io_threads: int = 0) -> "Flat":
        """The gain plane of the rounded mean of frames first .. first + count - 1 (default: to the end of the clip) of an open
        mlvfile.MlvReader, computed on the GPU; dark: a mlvfs_amd.dark.Dark of the flat clip's geometry, subtracted from the mean."""
        L = lib.load()
        handle = getattr(reader, "h", reader)
        if count is None:
            count = L.mlvfs_amd_mlv_frame_count(handle) - first
        h = L.mlvfs_amd_flat_from_clip(handle, first, count, None if dark is None else dark.h, batch, io_threads)
        if not h:
            raise lib.MlvfsAmdError("flat_from_clip failed: " + L.mlvfs_amd_last_error().decode())
        return cls(h)

    def info(self) -> dict:
        geom, n, means = lib.Geom(), C.c_int(0), (C.c_uint32 * 4)()
        lib.check(self.L.mlvfs_amd_flat_info(self.h, C.byref(geom), C.byref(n), means), "flat_info")
        return dict(width=geom.width, height=geom.height, bpp=geom.bpp, black=geom.black, frames_averaged=n.value, means=list(means))

    def gain(self) -> np.ndarray:
        """the Q14 gain plane, (height, width) uint16"""
        i = self.info()
        out = np.zeros((i["height"], i["width"]), np.uint16)
        lib.check(self.L.mlvfs_amd_flat_gain(self.h, lib.ptr(out), out.size), "flat_gain")
        return out

    def close(self) -> None:
        if self.h:
            self.L.mlvfs_amd_flat_destroy(self.h)
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
