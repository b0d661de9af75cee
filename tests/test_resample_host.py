"""Rendered frames resampled from the full-size rendering, the library's host code (no GPU): mlvfs_amd_rgb_fit_full, the sizes the
mount reports, every refusal of mlvfs_amd_render_resampled_dev and of the mount's resampled calls that happens before any device work,
the export table and the Python binding -- and the geometry and the refusals once more through a stand-alone C++ program
(tests/resample_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of the host code
(`make hostcheck`, built here if it is not yet).  Nothing is loaded into Python under a sanitizer.  The GPU side:
tests/test_gpu_resample.py, tests/test_gpu_mount_resampled.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, resample, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
SYMBOLS = ["mlvfs_amd_rgb_fit_full", "mlvfs_amd_render_resampled_dev", "mlvfs_amd_render_resampled_look_dev", "mlvfs_amd_render_resampled_deep_dev",
           "mlvfs_amd_mount_rgb_resampled", "mlvfs_amd_mount_jpeg_resampled", "mlvfs_amd_mount_rgb16_resampled",
           "mlvfs_amd_mount_rgb_resampled_size", "mlvfs_amd_mount_rgb16_resampled_size", "mlvfs_amd_test_resample_plan"]
# (w, h, box_w, box_h): both limits, a box larger than the frame, boxes of one pixel, the issue's sizes, the longest sides, products
# that need the 64 bits
FIT_GOOD = [(3584, 1320, 1920, 1080), (3584, 1320, 2560, 1440), (3584, 1320, 1280, 100), (1736, 976, 1280, 720), (3584, 1320, 3584, 1320),
            (3584, 1320, 5000, 5000), (3584, 1320, 3584, 1319), (3584, 1320, 1, 1), (3584, 1320, 1 << 30, 1), (3584, 1320, 1, 1 << 30),
            (4, 4, 1, 1), (5, 7, 9, 9), (418, 267, 300, 300), (65535, 4, 1 << 30, 1 << 30), (65535, 4, 65534, 1), (4, 65535, 1, 65534),
            (65535, 511, 65535, 2), (65535, 511, 2147483647, 510), (511, 65535, 510, 2147483647), (16, 600, 3, 599)]
FIT_BAD = [(3, 8, 4, 4), (8, 3, 4, 4), (0, 0, 4, 4), (-8, 8, 4, 4), (1 << 13, 1 << 12, 4, 4), (65536, 4, 4, 4), (4, 65536, 4, 4),
           (1 << 30, 1 << 30, 4, 4), (64, 48, 0, 4), (64, 48, 4, 0), (64, 48, -1, 4), (64, 48, 4, -(1 << 31))]


def fit(amd, w, h, bw, bh):
    ow, oh = C.c_int(-7), C.c_int(-7)
    return amd.mlvfs_amd_rgb_fit_full(w, h, bw, bh, C.byref(ow), C.byref(oh)), ow.value, oh.value


def test_rgb_fit_full(amd):
    for args in FIT_GOOD:
        assert fit(amd, *args) == (0,) + resample.fit(*args), args
        ow, oh = resample.fit(*args)
        assert 1 <= ow <= min(args[2], args[0]) and 1 <= oh <= min(args[3], args[1]), args
    assert resample.fit(3584, 1320, 1920, 1080) == (1920, 707) and resample.fit(3584, 1320, 2560, 1440) == (2560, 943)
    assert resample.fit(1736, 976, 1280, 720) == (1280, 720) and resample.fit(3584, 1320, 5000, 5000) == (3584, 1320)
    assert resample.fit(3584, 1320, 5000, 330) == (896, 330)
    for args in FIT_BAD:
        assert fit(amd, *args) == (lib.ERR_ARG, -7, -7), args
        with pytest.raises(ValueError):
            resample.fit(*args)
    one = C.c_int(5)
    assert amd.mlvfs_amd_rgb_fit_full(64, 48, 8, 8, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_rgb_fit_full(64, 48, 8, 8, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def test_render_resampled_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(8192, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p = src.ctypes.data, dst.ctypes.data, par.ctypes.data
    vp = lambda a: C.c_void_p(a) if a else None
    rs = lambda sp, st, w, h, pp, ow, oh, dp, ost, n: amd.mlvfs_amd_render_resampled_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, None)
    # a 32 x 8 frame, 512 bytes, to 20 x 5: 300 bytes
    for args in ((0, 512, 32, 8, p, 20, 5, d, 304, 1), (s, 512, 32, 8, 0, 20, 5, d, 304, 1), (s, 512, 32, 8, p, 20, 5, 0, 304, 1)):
        assert rs(*args) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error(), args
    for w, h in ((3, 16), (16, 3), (0, 16), (16, -1), (1 << 13, 1 << 12), (65536, 4), (4, 65536)):
        assert rs(s, 512, w, h, p, 1, 1, d, 304, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    for ow, oh in ((0, 5), (20, 0), (-1, 5), (20, -1), (33, 5), (20, 9), (33, 9), (1 << 30, 1 << 30)):
        assert rs(s, 512, 32, 8, p, ow, oh, d, 304, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (ow, oh)
    assert rs(s, 512, 32, 8, p, 20, 5, d, 304, -1) == lib.ERR_ARG
    assert rs(s, 510, 32, 8, p, 20, 5, d, 304, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()       # smaller than a frame
    assert rs(s, 512, 32, 8, p, 20, 5, d, 299, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()       # smaller than a rendering
    assert rs(s, 513, 32, 8, p, 20, 5, d, 304, 2) == lib.ERR_ARG                                                    # an odd source stride
    assert rs(s + 1, 512, 32, 8, p, 20, 5, d, 304, 1) == lib.ERR_ARG and rs(s, 512, 32, 8, p + 2, 20, 5, d, 304, 1) == lib.ERR_ARG
    # overlap: in place, the destination inside the source, either end reaching the other, the destination on the parameters
    for dp, n in ((s, 1), (s + 128, 1), (s + 511, 1), (s + 1024 + 511, 3), (s - 299, 1), (s - 300 - 2 * 304 + 1, 3)):
        assert rs(s + 4096, 512, 32, 8, p, 20, 5, dp + 4096, 304, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - s, n)
    for dp, n in ((p, 1), (p + 51, 1), (p - 299, 1), (p + 2 * 52 + 51, 3)):
        assert rs(s, 512, 32, 8, p, 20, 5, dp, 304, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - p, n)
    assert rs(s, 512, 32, 8, p, 20, 5, d, 304, 0) == 0                           # nothing to do
    # the look and deep forms: a null look, and the stride of six bytes per pixel
    assert amd.mlvfs_amd_render_resampled_look_dev(vp(s), 512, 32, 8, vp(p), 20, 5, vp(d), 304, 1, None, None) == lib.ERR_ARG
    assert amd.mlvfs_amd_render_resampled_deep_dev(vp(s), 512, 32, 8, vp(p), 20, 5, vp(d), 608, 1, None, None) == lib.ERR_ARG
    assert amd.mlvfs_amd_render_resampled_deep_dev(vp(s), 512, 32, 8, vp(p), 20, 5, vp(d), 599, 2, vp(d), None) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()
    assert (src == 7).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_resampled_refusals_and_sizes_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r:
        with Mount(r, MlvfsOptions()) as m:
            size = 256 + 50 * 40 * 3
            assert m.rgb_size(size=(50, 40), resample=True) == m.rgb_size(1, size=(50, 40), resample=True) == size == amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 50, 40)
            assert m.rgb_size(size=(50, 40), resample=True, bits=16) == 256 + 50 * 40 * 6 == amd.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, 50, 40)
            assert m.rgb_size(full=True) == m.rgb_size(size=(64, 48), resample=True) == 256 + 64 * 48 * 3 and m.rgb_size(size=(1, 1), resample=True) == 259
            assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 2, 50, 40) == 0 and amd.mlvfs_amd_mount_rgb_resampled_size(m.h, -1, 50, 40) == 0
            for ow, oh in ((65, 48), (64, 49), (0, 15), (20, 0), (-20, 15), (1 << 30, 1 << 30)):
                assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, ow, oh) == 0 and amd.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, ow, oh) == 0, (ow, oh)
                with pytest.raises(lib.MlvfsAmdError):
                    m.rgb_size(size=(ow, oh), resample=True)
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(size=(50, 40))                                        # the scaled route keeps its limit
            out = np.full(2 * 8192, 0xA5, np.uint8)
            sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
            O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
            rgb = lambda h, first, count, o, stride, gain, ow=50, oh=40: amd.mlvfs_amd_mount_rgb_resampled(h, first, count, o, stride, gain, ow, oh, 2, 1, None)
            jpg = lambda h, first, count, o, stride, gain, q, s, f, ow=50, oh=40: amd.mlvfs_amd_mount_jpeg_resampled(h, first, count, o, stride, gain, q, ow, oh, s, f, 2, 1, None)
            r16 = lambda h, first, count, o, stride, gain, lk, ow=50, oh=40: amd.mlvfs_amd_mount_rgb16_resampled(h, first, count, o, stride, gain, ow, oh, lk, 2, 1, None)
            # one byte less than the file is not room enough
            assert rgb(m.h, 0, 2, O, size - 1, 256) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
            assert jpg(m.h, 0, 2, O, size - 1, 256, 90, S, F) == lib.ERR_ARG
            for ow, oh in ((65, 48), (64, 49), (0, 15), (20, 0), (-20, 15), (1 << 30, 1 << 30)):
                assert rgb(m.h, 0, 2, O, 8192, 256, ow, oh) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error(), (ow, oh)
                assert jpg(m.h, 0, 2, O, 8192, 256, 90, S, F, ow, oh) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error(), (ow, oh)
                assert r16(m.h, 0, 2, O, 8192, 256, O, ow, oh) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error(), (ow, oh)
            for gain in (0, -256, 65536):
                assert rgb(m.h, 0, 2, O, size, gain) == lib.ERR_ARG and b"gain" in amd.mlvfs_amd_last_error(), gain
                assert jpg(m.h, 0, 2, O, size, gain, 90, S, F) == lib.ERR_ARG and r16(m.h, 0, 2, O, 8192, gain, O) == lib.ERR_ARG
            for q in (0, 101, -1):
                assert jpg(m.h, 0, 2, O, size, 256, q, S, F) == lib.ERR_ARG and b"quality" in amd.mlvfs_amd_last_error(), q
            assert jpg(m.h, 0, 2, O, size, 256, 90, None, F) == lib.ERR_ARG and jpg(m.h, 0, 2, O, size, 256, 90, S, None) == lib.ERR_ARG
            assert r16(m.h, 0, 2, O, 8192, 256, None) == lib.ERR_ARG and r16(m.h, 0, 2, O, 256 + 50 * 40 * 6 - 1, 256, O) == lib.ERR_ARG
            assert rgb(m.h, 0, 3, O, size, 256) == lib.ERR_ARG and rgb(m.h, -1, 1, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 2, None, size, 256) == lib.ERR_ARG and rgb(None, 0, 2, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, -1, O, size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 0, O, size, 256) == 0 and jpg(m.h, 0, 0, O, size, 256, 90, S, F) == 0        # nothing to do
            for gain in (0.0, -1.0, 256.0):
                with pytest.raises(ValueError):
                    m.rgb(0, 2, gain=gain, size=(50, 40), resample=True)
            with pytest.raises(ValueError):
                m.jpeg(0, 2, quality=0, size=(50, 40), resample=True)
            for call in (lambda: m.rgb(0, 2, full=True, size=(50, 40), resample=True), lambda: m.jpeg(0, 2, full=True, size=(50, 40), resample=True),
                         lambda: m.rgb_size(0, full=True, size=(50, 40), resample=True), lambda: m.rgb(0, 2, resample=True),
                         lambda: m.jpeg(0, 2, resample=True), lambda: m.rgb_size(0, resample=True), lambda: m.rgb(0, 2, full=True, resample=True),
                         lambda: m.rgb(0, 2, full=True, size=(20, 15))):
                with pytest.raises(ValueError):
                    call()
            m.set_proxy(2)                                                       # nothing was served: a refusal serves nothing
            assert rgb(m.h, 0, 2, O, size, 256) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            assert jpg(m.h, 0, 2, O, size, 256, 90, S, F) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            assert r16(m.h, 0, 2, O, 8192, 256, O) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb(0, 2, size=(50, 40), resample=True)
            assert m.rgb_size(size=(50, 40), resample=True) == size              # the size of a rendering does not depend on it
            assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
    assert amd.mlvfs_amd_mount_rgb_resampled_size(None, 0, 20, 15) == 0
    with mlvfile.MlvReader(clips("B.MLV", 16, 3)) as r, Mount(r, MlvfsOptions()) as m:        # three rows: the half-size route takes it, this one not
        assert m.rgb_size() == 256 + 8 * 3 and amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 8, 1) == 0 and b"resampled" in amd.mlvfs_amd_last_error()
    with mlvfile.MlvReader(clips("C.MLV", 418, 267)) as r, Mount(r, MlvfsOptions()) as m:     # odd sizes keep their last row and column
        assert m.rgb_size(size=(418, 267), resample=True) == 256 + 418 * 267 * 3
        assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 419, 267) == 0


def test_resampled_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    for f in (Mount.rgb, Mount.jpeg, Mount.rgb_size):
        par = inspect.signature(f).parameters
        assert par["resample"].default is False and list(par)[-1] == "resample" and par["size"].default is None
    for name in ("geom", "fit", "stages", "render", "split_file"):
        assert callable(getattr(resample, name))


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/resample_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the fit writes exactly two ints, its products and the plan's overflow nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for args in FIT_GOOD:
            f.write(struct.pack("<7i", *args, 0, *resample.fit(*args)))
        for args in FIT_BAD:
            f.write(struct.pack("<7i", *args, lib.ERR_ARG, -7, -7))
    exe = tmp_path / "resample_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "resample_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"resample_host_check: {len(FIT_GOOD) + len(FIT_BAD)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
