"""Rendered full-size sRGB frames, the library's host code (no GPU): mlvfs_amd_rgb_full_geom, the sizes the mount reports, every
refusal of mlvfs_amd_render1_dev and of the mount's full-size calls that happens before any device work, the export table and the
Python binding -- and the geometry and the refusals once more through a stand-alone C++ program (tests/demosaic_host_check.cpp) built
with -fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).
Nothing is loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_demosaic.py, tests/test_gpu_mount_full.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import demosaic_cases as dm
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
FULL_SYMBOLS = ["mlvfs_amd_rgb_full_geom", "mlvfs_amd_render1_dev", "mlvfs_amd_mount_rgb_full", "mlvfs_amd_mount_jpeg_full",
                "mlvfs_amd_mount_rgb_full_size"]
GOOD = dm.SIZES + dm.MOUNT_SIZES + [(dm.BIG_W, dm.BIG_H), (4, 1 << 22), (8191, 4095), (5793, 5792)]
BAD = [(3, 4), (4, 3), (2, 2), (0, 0), (-4, 8), (8, -4), (1 << 13, 1 << 12), (1 << 25, 4), (5793, 5793), (1 << 30, 1 << 30)]


def geom(amd, w, h):
    pw, ph = C.c_int(-7), C.c_int(-7)
    return amd.mlvfs_amd_rgb_full_geom(w, h, C.byref(pw), C.byref(ph)), pw.value, ph.value


def test_rgb_full_geom(amd):
    for w, h in GOOD:
        assert geom(amd, w, h) == (0, w, h) == (0,) + demosaic.geom(w, h), (w, h)
    for w, h in BAD:
        assert geom(amd, w, h) == (lib.ERR_ARG, -7, -7) and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
        with pytest.raises(ValueError):
            demosaic.geom(w, h)
    one = C.c_int(5)
    assert amd.mlvfs_amd_rgb_full_geom(16, 16, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_rgb_full_geom(16, 16, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def test_render1_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(8192, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p = src.ctypes.data, dst.ctypes.data, par.ctypes.data
    vp = lambda a: C.c_void_p(a) if a else None
    r1 = lambda sp, st, w, h, pp, dp, ost, n: amd.mlvfs_amd_render1_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    for args in ((0, 256, 16, 8, p, d, 384, 1), (s, 256, 16, 8, 0, d, 384, 1), (s, 256, 16, 8, p, 0, 384, 1)):
        assert r1(*args) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error(), args
    for w, h in ((3, 16), (16, 3), (2, 2), (0, 16), (16, -1), (1 << 13, 1 << 12)):
        assert r1(s, 256, w, h, p, d, 384, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    assert r1(s, 256, 16, 8, p, d, 384, -1) == lib.ERR_ARG
    assert r1(s, 254, 16, 8, p, d, 384, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a frame
    assert r1(s, 256, 16, 8, p, d, 383, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a rendering
    assert r1(s, 257, 16, 8, p, d, 384, 2) == lib.ERR_ARG                                                   # an odd source stride
    assert r1(s + 1, 256, 16, 8, p, d, 384, 1) == lib.ERR_ARG and r1(s, 256, 16, 8, p + 2, d, 384, 1) == lib.ERR_ARG
    # overlap: in place, the destination inside the source, either end reaching the other, the destination on the parameters
    for dp, n in ((s, 1), (s + 128, 1), (s + 255, 1), (s + 512 + 255, 3), (s - 383, 1), (s - 384 - 2 * 512 + 1, 3)):
        assert r1(s + 4096, 256, 16, 8, p, dp + 4096, 512, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - s, n)
    for dp, n in ((p, 1), (p + 51, 1), (p - 383, 1), (p + 2 * 52 + 51, 3)):
        assert r1(s, 256, 16, 8, p, dp, 384, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - p, n)
    assert r1(s, 256, 16, 8, p, d, 384, 0) == 0                                  # nothing to do
    assert (src == 7).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_full_refusals_and_sizes_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r:
        with Mount(r, MlvfsOptions()) as m:
            size = 256 + 64 * 48 * 3
            assert m.rgb_size(full=True) == m.rgb_size(1, full=True) == size == amd.mlvfs_amd_mount_rgb_full_size(m.h, 0)
            assert m.rgb_size() == 256 + 32 * 24 * 3                             # the default is the half-size file
            assert amd.mlvfs_amd_mount_rgb_full_size(m.h, 2) == 0 and amd.mlvfs_amd_mount_rgb_full_size(m.h, -1) == 0
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(2, full=True)
            out = np.full(2 * size, 0xA5, np.uint8)
            sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
            O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
            rgb = lambda h, first, count, o, stride, gain: amd.mlvfs_amd_mount_rgb_full(h, first, count, o, stride, gain, 2, 1, None)
            jpg = lambda h, first, count, o, stride, gain, q, s, f: amd.mlvfs_amd_mount_jpeg_full(h, first, count, o, stride, gain, q, s, f, 2, 1, None)
            # the half-size file's room is not enough, nor one byte less than the file
            assert rgb(m.h, 0, 2, O, m.rgb_size(), 256) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
            assert rgb(m.h, 0, 2, O, size - 1, 256) == lib.ERR_ARG and jpg(m.h, 0, 2, O, size - 1, 256, 90, S, F) == lib.ERR_ARG
            for gain in (0, -256, 65536):
                assert rgb(m.h, 0, 2, O, size, gain) == lib.ERR_ARG and b"gain" in amd.mlvfs_amd_last_error(), gain
                assert jpg(m.h, 0, 2, O, size, gain, 90, S, F) == lib.ERR_ARG
            for q in (0, 101, -1):
                assert jpg(m.h, 0, 2, O, size, 256, q, S, F) == lib.ERR_ARG and b"quality" in amd.mlvfs_amd_last_error(), q
            assert jpg(m.h, 0, 2, O, size, 256, 90, None, F) == lib.ERR_ARG and jpg(m.h, 0, 2, O, size, 256, 90, S, None) == lib.ERR_ARG
            assert rgb(m.h, 0, 3, O, size, 256) == lib.ERR_ARG and rgb(m.h, -1, 1, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 2, None, size, 256) == lib.ERR_ARG and rgb(None, 0, 2, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, -1, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 0, O, size, 256) == 0 and jpg(m.h, 0, 0, O, size, 256, 90, S, F) == 0        # nothing to do
            for gain in (0.0, -1.0, 256.0):
                with pytest.raises(ValueError):
                    m.rgb(0, 2, gain=gain, full=True)
            with pytest.raises(ValueError):
                m.jpeg(0, 2, quality=0, full=True)
            m.set_proxy(2)                                                       # nothing was served: a refusal serves nothing
            assert rgb(m.h, 0, 2, O, size, 256) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            assert jpg(m.h, 0, 2, O, size, 256, 90, S, F) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb(0, 2, full=True)
            assert m.rgb_size(full=True) == size                                 # the size of a rendering does not depend on it
            assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
    assert amd.mlvfs_amd_mount_rgb_full_size(None, 0) == 0
    with mlvfile.MlvReader(clips("B.MLV", 16, 3)) as r, Mount(r, MlvfsOptions()) as m:        # a frame below 4x4: the half-size call takes it
        assert amd.mlvfs_amd_mount_rgb_full_size(m.h, 0) == 0 and b"4x4" in amd.mlvfs_amd_last_error()
        assert m.rgb_size() == 256 + 8 * 1 * 3
        out = np.full(4096, 0xA5, np.uint8)
        assert amd.mlvfs_amd_mount_rgb_full(m.h, 0, 1, lib.ptr(out), 4096, 256, 1, 1, None) == lib.ERR_ARG and b"4x4" in amd.mlvfs_amd_last_error()
        assert (out == 0xA5).all()
    with mlvfile.MlvReader(clips("C.MLV", 418, 267)) as r, Mount(r, MlvfsOptions()) as m:     # odd sizes keep their last row
        assert m.rgb_size(full=True) == 256 + 418 * 267 * 3


def test_full_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in FULL_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    for f in (Mount.rgb, Mount.jpeg, Mount.rgb_size):
        assert inspect.signature(f).parameters["full"].default is False
    assert list(inspect.signature(Mount.rgb).parameters)[1:4] == ["first", "count", "gain"]


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/demosaic_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the geometry writes exactly two ints, the size arithmetic overflows nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for w, h in GOOD:
            f.write(struct.pack("<5i", w, h, 0, w, h))
        for w, h in BAD:
            f.write(struct.pack("<5i", w, h, lib.ERR_ARG, -7, -7))
    exe = tmp_path / "demosaic_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "demosaic_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"demosaic_host_check: {len(GOOD) + len(BAD)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
