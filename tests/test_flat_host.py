"""Flat fields, the library's host code (csrc/cal.cpp; no GPU): mlvfs_amd_flat_create and mlvfs_amd_flat_gain against the numpy
oracle of tests/flat_cases.py, every refusal of the host and device entry points (before any device work), the export table and the
Python binding -- and the same planes once more through a stand-alone C++ program (tests/flat_host_check.cpp) built with
-fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).  The GPU side: tests/test_gpu_flat.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.flat import Flat
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import dark_cases as dc
import flat_cases as fc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
FLAT_SYMBOLS = ["mlvfs_amd_flat_create", "mlvfs_amd_flat_from_clip", "mlvfs_amd_flat_info", "mlvfs_amd_flat_gain", "mlvfs_amd_flat_destroy",
                "mlvfs_amd_flat_apply_dev", "mlvfs_amd_mount_set_flat", "mlvfs_amd_mlv_transcode_cal"]


def host_planes():
    """(w, h, bpp, black_f, plane): the edge geometries at 14 bits, a constant plane, 16-bit planes with the exact-half gain and with
    channel sums beyond 32 bits"""
    out = [(w, h, 14, dc.clip_black(14), fc.flat_plane(w, h)) for (w, h) in fc.HOST_GEOMETRIES]
    out.append((30, 10, 12, 512, fc.constant_plane(30, 10, 900)))
    out.append((64, 48, 16, 0, fc.flat_plane(64, 48, 16, 0)))
    out.append((640, 480, 16, 0, fc.overflow_plane()))
    return out


def test_create_and_gain_equal_the_oracle(amd):
    assert [(w, h) for w, h, *_ in host_planes()][:8] == [(2, 2), (3, 3), (5, 4), (3, 16), (30, 10), (1, 8), (8, 1), (416, 264)]
    for w, h, bpp, black_f, plane in host_planes():
        want, means = fc.gains(plane, black_f), fc.channel_means(plane, black_f)
        with Flat.from_plane(plane, bpp, black_f) as f:
            assert f.info() == dict(width=w, height=h, bpp=bpp, black=black_f, frames_averaged=0, means=means), (w, h)
            got = f.gain()
            assert got.dtype == np.uint16 and np.array_equal(got, want), (w, h, int((got != want).sum()))
            plane[0, 0] ^= 1                                                 # the handle keeps nothing of the caller's
            assert np.array_equal(f.gain(), want)
            big = np.full(w * h + 3, 0xABCD, np.uint16)
            assert amd.mlvfs_amd_flat_gain(f.h, lib.ptr(big), big.size) == 0 and (big[w * h:] == 0xABCD).all()
            assert amd.mlvfs_amd_flat_info(f.h, None, None, None) == 0
        assert f.h is None
    with Flat.from_plane(fc.flat_plane(1, 8), 14, 2048) as f:                # channels without pixels: no M_c
        assert f.info()["means"][1] == 0 and f.info()["means"][3] == 0


def test_host_refusals(amd):
    plane = np.full((4, 16), 3000, np.uint16)

    def create(w, h, bpp, black, p=plane):
        g = lib.Geom(w, h, bpp, black, 0, 0, 0)
        return amd.mlvfs_amd_flat_create(C.byref(g), None if p is None else lib.ptr(p))

    assert create(16, 4, 14, 2048, None) is None and b"null" in amd.mlvfs_amd_last_error()
    assert amd.mlvfs_amd_flat_create(None, lib.ptr(plane)) is None
    for bpp in (0, 17, -1, 32):
        assert create(16, 4, bpp, 2048) is None and b"bits_per_pixel" in amd.mlvfs_amd_last_error(), bpp
    for w, h in ((0, 4), (16, 0), (-16, 4), (16, -4), (1 << 14, 1 << 13)):
        assert create(w, h, 14, 2048) is None and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    for black in (-1, 65536):
        assert create(16, 4, 14, black) is None and b"pedestal" in amd.mlvfs_amd_last_error(), black
    h = create(16, 4, 14, 2048)
    assert h
    try:
        out = np.full(64, 7, np.uint16)
        assert amd.mlvfs_amd_flat_gain(h, lib.ptr(out), 63) == lib.ERR_ARG and (out == 7).all()           # cap_pixels too small
        assert amd.mlvfs_amd_flat_gain(h, None, 64) == lib.ERR_ARG and amd.mlvfs_amd_flat_gain(None, lib.ptr(out), 64) == lib.ERR_ARG
        assert amd.mlvfs_amd_flat_info(None, None, None, None) == lib.ERR_ARG
        # the device entry point refuses on the host, before any device work: the pointers are never followed
        app, buf = amd.mlvfs_amd_flat_apply_dev, lib.ptr(out)
        g = lambda w, hh, bpp, black=2048: C.byref(lib.Geom(w, hh, bpp, black, 0, 0, 0))
        for w, hh in ((16, 2), (8, 4), (4, 16)):
            assert app(h, None, g(w, hh, 14), buf, 128, 1, None) == lib.ERR_ARG, (w, hh)                  # only the size must match ...
        for bpp in (0, 17):
            assert app(h, None, g(16, 4, bpp), buf, 128, 1, None) == lib.ERR_ARG, bpp
        for black in (-1, 65536):
            assert app(h, None, g(16, 4, 14, black), buf, 128, 1, None) == lib.ERR_ARG, black
        assert app(None, None, g(16, 4, 14), buf, 128, 1, None) == lib.ERR_ARG and app(h, None, None, buf, 128, 1, None) == lib.ERR_ARG
        assert app(h, None, g(16, 4, 14), None, 128, 1, None) == lib.ERR_ARG and app(h, None, g(16, 4, 14), buf, 128, -1, None) == lib.ERR_ARG
        assert app(h, None, g(16, 4, 14), buf, 126, 2, None) == lib.ERR_ARG and app(h, None, g(16, 4, 14), buf, 129, 2, None) == lib.ERR_ARG
        assert app(h, None, g(16, 4, 14), C.c_void_p(out.ctypes.data + 1), 128, 1, None) == lib.ERR_ARG
        for shape, bpp in (((4, 8), 12), ((4, 16), 14)):                      # ... but a dark frame has the frames' size AND depth
            with Dark.from_plane(np.zeros(shape, np.uint16), bpp, 512) as d:
                assert app(h, d.h, g(16, 4, 12), buf, 128, 1, None) == lib.ERR_ARG and b"dark" in amd.mlvfs_amd_last_error()
        for bpp in (10, 12, 16):                                             # ... a flat of another depth than the frames' is fine
            assert app(h, None, g(16, 4, bpp), buf, 128, 0, None) == 0
        assert (out == 7).all()
    finally:
        amd.mlvfs_amd_flat_destroy(h)
    amd.mlvfs_amd_flat_destroy(None)
    with pytest.raises(ValueError):
        Flat.from_plane(np.zeros((4, 16), np.int32), 14, 2048)


def test_from_clip_and_the_users_refuse_on_the_host(amd, tmp_path):
    """Frames outside the clip, too many frames, a dark frame of another geometry, a flat field of another size, out_bpp out of
    range: refused before any device work and before any output file exists."""
    frames = [synth.normal_frame(64, 48, seed=3, frame=k) for k in range(3)]
    names = mlvfile.write_clip(str(tmp_path / "A.MLV"), [synth.pack_bits(f).tobytes() for f in frames], 64, 48)
    out = tmp_path / "out"
    out.mkdir()
    stats = (C.c_longlong * 4)()
    with mlvfile.MlvReader(names[0]) as r:
        for first, count in ((0, 4), (2, 2), (3, 1), (-1, 2), (0, 0), (0, -1), (0, 65537), (0, 1 << 20)):
            assert amd.mlvfs_amd_flat_from_clip(r.h, first, count, None, 3, 2) is None, (first, count)
        assert amd.mlvfs_amd_flat_from_clip(None, 0, 1, None, 3, 2) is None
        for shape, bpp in (((48, 32), 14), ((48, 64), 12)):
            with Dark.from_plane(np.zeros(shape, np.uint16), bpp, 2048) as d:
                assert amd.mlvfs_amd_flat_from_clip(r.h, 0, 3, d.h, 3, 2) is None and b"dark frame's geometry" in amd.mlvfs_amd_last_error()
        for shape in ((48, 32), (24, 64), (64, 48)):
            with Flat.from_plane(np.full(shape, 3000, np.uint16), 14, 2048) as f:
                with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                    Mount(r, MlvfsOptions(), flat=f)
                with Mount(r, MlvfsOptions()) as m:
                    assert amd.mlvfs_amd_mount_set_flat(m.h, f.h) == lib.ERR_ARG
                for lj92 in (False, True):
                    with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                        r.transcode(str(out / "B.MLV"), lj92=lj92, flat=f)
                    assert list(out.iterdir()) == []
        with Flat.from_plane(np.full((48, 64), 3000, np.uint16), 12, 512) as f:       # the right size (at another depth: fine)
            with Mount(r, MlvfsOptions(), flat=f) as m:
                m.set_flat(None)                                             # NULL clears
                assert m._flat is None
            assert amd.mlvfs_amd_mount_set_flat(None, f.h) == lib.ERR_ARG
            for bits in (7, 17, -1):
                rc = amd.mlvfs_amd_mlv_transcode_cal(r.h, str(out / "B.MLV").encode(), lib.MLV_PLAIN, bits, None, f.h, 2, 2, stats)
                assert rc == lib.ERR_ARG and list(out.iterdir()) == [], bits
            assert amd.mlvfs_amd_mlv_transcode_cal(None, str(out / "B.MLV").encode(), lib.MLV_PLAIN, 0, None, f.h, 2, 2, stats) == lib.ERR_ARG
        # without a flat field mlvfs_amd_mlv_transcode_cal is mlvfs_amd_mlv_transcode_bits, the host-only route included
        assert amd.mlvfs_amd_mlv_transcode_cal(r.h, str(out / "C.MLV").encode(), lib.MLV_PLAIN, 0, None, None, 2, 2, stats) == 0
        assert r.transcode(str(out / "D.MLV"), lj92=False, batch=2, io_threads=2) == dict(frames=int(stats[0]), bytes_in=int(stats[1]),
                                                                                        bytes_out=int(stats[2]), files=int(stats[3]))
        assert (out / "C.MLV").read_bytes() == (out / "D.MLV").read_bytes() and stats[0] == 3


def test_flat_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in FLAT_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert {s for s in exported if s.startswith("mlvfs_amd_flat_")} == {s for s in FLAT_SYMBOLS if s.startswith("mlvfs_amd_flat_")}
    assert inspect.signature(Mount.__init__).parameters["flat"].default is None
    assert inspect.signature(mlvfile.MlvReader.transcode).parameters["flat"].default is None


def test_the_same_planes_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/flat_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: mlvfs_amd_flat_create reads exactly width * height entries and mlvfs_amd_flat_gain writes exactly as many (the
    program's buffers are that long and no longer), and the 16-bit planes' 64-bit sums and 2^30-sized numerators stay defined."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for w, h, bpp, black_f, plane in host_planes():
            f.write(struct.pack("<4i4I", w, h, bpp, black_f, *fc.channel_means(plane, black_f)))
            f.write(np.ascontiguousarray(plane, "<u2").tobytes() + np.ascontiguousarray(fc.gains(plane, black_f), "<u2").tobytes())
    exe = tmp_path / "flat_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "flat_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"flat_host_check: {len(host_planes())} planes" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
