"""Dark frames (mlvfs_amd_dark_*, csrc/cal.cpp, csrc/k_cal.hip): a sensor's fixed offset pattern, subtracted on the GPU before
any other stage looks at the pixels.

    out     = clamp(px - dark + black_d, 0, 2^bpp - 1)          black_d: the black level of the clip the plane was averaged from
    dark[p] = (sum over n frames of px_f[p] + n // 2) // n

    with mlvfile.MlvReader("DARK.MLV") as dr, Dark.from_clip(dr) as dark, mlvfile.MlvReader("M07-1234.MLV") as r:
        with Mount(r, MlvfsOptions(chroma_smooth=5), dark=dark) as m:
            files = m.dng(0, 16)
        r.transcode("OUT.MLV", lj92=True, dark=dark)

A Dark must outlive the mounts that use it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib


class Dark:
    def __init__(self, handle):
        self.L = lib.load()
        self.h = handle

    @classmethod
    def from_plane(cls, plane: np.ndarray, bpp: int, black: int) -> "Dark":
        """plane: (height, width) uint16; black: the pedestal black_d.  Host code: needs no GPU."""
        L = lib.load()
        if not (isinstance(plane, np.ndarray) and plane.ndim == 2 and plane.dtype == np.uint16):
            raise ValueError("a dark plane is a (height, width) uint16 array")
        p = np.ascontiguousarray(plane)
        geom = lib.Geom(p.shape[1], p.shape[0], bpp, black, 0, 0, 0)
        h = L.mlvfs_amd_dark_create(C.byref(geom), lib.ptr(p))
        if not h:
            raise lib.MlvfsAmdError("dark_create failed: " + L.mlvfs_amd_last_error().decode())
        return cls(h)

    @classmethod
    def from_clip(cls, reader, first: int = 0, count: int | None = None, batch: int = 0, io_threads: int = 0) -> "Dark":
        """The rounded mean of frames first .. first + count - 1 (default: to the end of the clip) of an open mlvfile.MlvReader."""
        L = lib.load()
        handle = getattr(reader, "h", reader)
        if count is None:
            count = L.mlvfs_amd_mlv_frame_count(handle) - first
        h = L.mlvfs_amd_dark_from_clip(handle, first, count, batch, io_threads)
        if not h:
            raise lib.MlvfsAmdError("dark_from_clip failed: " + L.mlvfs_amd_last_error().decode())
        return cls(h)

    def info(self) -> dict:
        geom, n = lib.Geom(), C.c_int(0)
        lib.check(self.L.mlvfs_amd_dark_info(self.h, C.byref(geom), C.byref(n)), "dark_info")
        return dict(width=geom.width, height=geom.height, bpp=geom.bpp, black=geom.black, frames_averaged=n.value)

    def plane(self) -> np.ndarray:
        i = self.info()
        out = np.zeros((i["height"], i["width"]), np.uint16)
        lib.check(self.L.mlvfs_amd_dark_plane(self.h, lib.ptr(out), out.size), "dark_plane")
        return out

    def close(self) -> None:
        if self.h:
            self.L.mlvfs_amd_dark_destroy(self.h)
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
