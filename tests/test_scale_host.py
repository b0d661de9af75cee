"""Rendered frames at any smaller size, the library's host code (no GPU): mlvfs_amd_rgb_fit, the sizes the mount reports, every
refusal of mlvfs_amd_render_scaled_dev and of the mount's scaled calls that happens before any device work, the export table and the
Python binding -- and the geometry and the refusals once more through a stand-alone C++ program (tests/scale_host_check.cpp) built
with -fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).
Nothing is loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_scale.py, tests/test_gpu_mount_scaled.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, scale, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import scale_cases as sc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
SCALE_SYMBOLS = ["mlvfs_amd_rgb_fit", "mlvfs_amd_render_scaled_dev", "mlvfs_amd_mount_rgb_scaled", "mlvfs_amd_mount_jpeg_scaled",
                 "mlvfs_amd_mount_rgb_scaled_size", "mlvfs_amd_test_scale_div", "mlvfs_amd_test_scale_plan"]
# (w, h, box_w, box_h): both limits, a box larger than the frame, boxes of one pixel, the bench's sizes, the longest sides, products
# that need the 64 bits
FIT_GOOD = [(3584, 1320, 1280, 720), (3584, 1320, 1280, 100), (3584, 1320, 448, 448), (3584, 1320, 160, 160), (3584, 1320, 1792, 660),
            (3584, 1320, 5000, 5000), (3584, 1320, 1792, 659), (3584, 1320, 1, 1), (3584, 1320, 1 << 30, 1), (3584, 1320, 1, 1 << 30),
            (2, 2, 1, 1), (3, 3, 7, 7), (418, 267, 100, 100), (131070, 2, 1 << 30, 1 << 30), (131070, 2, 65534, 1), (2, 131070, 1, 65534),
            (131070, 1022, 65535, 2), (131070, 1022, 2147483647, 510), (1022, 131070, 510, 2147483647), (16, 600, 3, 299)]
FIT_BAD = [(1, 8, 4, 4), (8, 1, 4, 4), (0, 0, 4, 4), (-8, 8, 4, 4), (1 << 14, 1 << 13, 4, 4), (131072, 2, 4, 4), (2, 131072, 4, 4),
           (1 << 30, 1 << 30, 4, 4), (64, 48, 0, 4), (64, 48, 4, 0), (64, 48, -1, 4), (64, 48, 4, -(1 << 31))]


def fit(amd, w, h, bw, bh):
    ow, oh = C.c_int(-7), C.c_int(-7)
    return amd.mlvfs_amd_rgb_fit(w, h, bw, bh, C.byref(ow), C.byref(oh)), ow.value, oh.value


def test_rgb_fit(amd):
    for args in FIT_GOOD:
        assert fit(amd, *args) == (0,) + scale.fit(*args), args
        ow, oh = scale.fit(*args)
        assert 1 <= ow <= min(args[2], args[0] // 2) and 1 <= oh <= min(args[3], args[1] // 2), args
    assert scale.fit(3584, 1320, 1280, 720) == (1280, 471) and scale.fit(3584, 1320, 160, 160) == (160, 59)
    assert scale.fit(3584, 1320, 5000, 5000) == (1792, 660) and scale.fit(3584, 1320, 5000, 330) == (896, 330)
    for args in FIT_BAD:
        assert fit(amd, *args) == (lib.ERR_ARG, -7, -7), args
        with pytest.raises(ValueError):
            scale.fit(*args)
    one = C.c_int(5)
    assert amd.mlvfs_amd_rgb_fit(64, 48, 8, 8, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_rgb_fit(64, 48, 8, 8, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def test_render_scaled_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(8192, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p = src.ctypes.data, dst.ctypes.data, par.ctypes.data
    vp = lambda a: C.c_void_p(a) if a else None
    rs = lambda sp, st, w, h, pp, ow, oh, dp, ost, n: amd.mlvfs_amd_render_scaled_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, None)
    # a 32 x 8 frame, 512 bytes, to 7 x 3: 63 bytes
    for args in ((0, 512, 32, 8, p, 7, 3, d, 64, 1), (s, 512, 32, 8, 0, 7, 3, d, 64, 1), (s, 512, 32, 8, p, 7, 3, 0, 64, 1)):
        assert rs(*args) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error(), args
    for w, h in ((1, 16), (16, 1), (0, 16), (16, -1), (1 << 14, 1 << 13), (131072, 2), (2, 131072)):
        assert rs(s, 512, w, h, p, 1, 1, d, 64, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    for ow, oh in ((0, 3), (7, 0), (-1, 3), (7, -1), (17, 3), (7, 5), (16, 5), (1 << 30, 1 << 30)):
        assert rs(s, 512, 32, 8, p, ow, oh, d, 64, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (ow, oh)
    assert rs(s, 512, 32, 8, p, 7, 3, d, 64, -1) == lib.ERR_ARG
    assert rs(s, 510, 32, 8, p, 7, 3, d, 64, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()         # smaller than a frame
    assert rs(s, 512, 32, 8, p, 7, 3, d, 62, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()         # smaller than a rendering
    assert rs(s, 513, 32, 8, p, 7, 3, d, 64, 2) == lib.ERR_ARG                                                      # an odd source stride
    assert rs(s + 1, 512, 32, 8, p, 7, 3, d, 64, 1) == lib.ERR_ARG and rs(s, 512, 32, 8, p + 2, 7, 3, d, 64, 1) == lib.ERR_ARG
    # overlap: in place, the destination inside the source, either end reaching the other, the destination on the parameters
    for dp, n in ((s, 1), (s + 128, 1), (s + 511, 1), (s + 1024 + 511, 3), (s - 62, 1), (s - 63 - 2 * 64 + 1, 3)):
        assert rs(s + 4096, 512, 32, 8, p, 7, 3, dp + 4096, 64, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - s, n)
    for dp, n in ((p, 1), (p + 51, 1), (p - 62, 1), (p + 2 * 52 + 51, 3)):
        assert rs(s, 512, 32, 8, p, 7, 3, dp, 64, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - p, n)
    assert rs(s, 512, 32, 8, p, 7, 3, d, 64, 0) == 0                             # nothing to do
    assert (src == 7).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_scaled_refusals_and_sizes_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r:
        with Mount(r, MlvfsOptions()) as m:
            size = 256 + 20 * 15 * 3
            assert m.rgb_size(size=(20, 15)) == m.rgb_size(1, size=(20, 15)) == size == amd.mlvfs_amd_mount_rgb_scaled_size(m.h, 0, 20, 15)
            assert m.rgb_size() == m.rgb_size(size=(32, 24)) == 256 + 32 * 24 * 3 and m.rgb_size(size=(1, 1)) == 259
            assert amd.mlvfs_amd_mount_rgb_scaled_size(m.h, 2, 20, 15) == 0 and amd.mlvfs_amd_mount_rgb_scaled_size(m.h, -1, 20, 15) == 0
            for ow, oh in ((33, 24), (32, 25), (0, 15), (20, 0), (-20, 15), (1 << 30, 1 << 30)):
                assert amd.mlvfs_amd_mount_rgb_scaled_size(m.h, 0, ow, oh) == 0, (ow, oh)
                with pytest.raises(lib.MlvfsAmdError):
                    m.rgb_size(size=(ow, oh))
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(2, size=(20, 15))
            out = np.full(2 * 4096, 0xA5, np.uint8)
            sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
            O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
            rgb = lambda h, first, count, o, stride, gain, ow=20, oh=15: amd.mlvfs_amd_mount_rgb_scaled(h, first, count, o, stride, gain, ow, oh, 2, 1, None)
            jpg = lambda h, first, count, o, stride, gain, q, s, f, ow=20, oh=15: amd.mlvfs_amd_mount_jpeg_scaled(h, first, count, o, stride, gain, q, ow, oh, s, f, 2, 1, None)
            # one byte less than the file is not room enough
            assert rgb(m.h, 0, 2, O, size - 1, 256) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
            assert jpg(m.h, 0, 2, O, size - 1, 256, 90, S, F) == lib.ERR_ARG
            for ow, oh in ((33, 24), (32, 25), (0, 15), (20, 0), (-20, 15), (1 << 30, 1 << 30)):
                assert rgb(m.h, 0, 2, O, 4096, 256, ow, oh) == lib.ERR_ARG and b"scaled" in amd.mlvfs_amd_last_error(), (ow, oh)
                assert jpg(m.h, 0, 2, O, 4096, 256, 90, S, F, ow, oh) == lib.ERR_ARG and b"scaled" in amd.mlvfs_amd_last_error(), (ow, oh)
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
                    m.rgb(0, 2, gain=gain, size=(20, 15))
            with pytest.raises(ValueError):
                m.jpeg(0, 2, quality=0, size=(20, 15))
            for call in (lambda: m.rgb(0, 2, full=True, size=(20, 15)), lambda: m.jpeg(0, 2, full=True, size=(20, 15)),
                         lambda: m.rgb_size(0, full=True, size=(20, 15))):
                with pytest.raises(ValueError):
                    call()
            m.set_proxy(2)                                                       # nothing was served: a refusal serves nothing
            assert rgb(m.h, 0, 2, O, size, 256) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            assert jpg(m.h, 0, 2, O, size, 256, 90, S, F) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb(0, 2, size=(20, 15))
            assert m.rgb_size(size=(20, 15)) == size                             # the size of a rendering does not depend on it
            assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
    assert amd.mlvfs_amd_mount_rgb_scaled_size(None, 0, 20, 15) == 0
    with mlvfile.MlvReader(clips("B.MLV", 16, 3)) as r, Mount(r, MlvfsOptions()) as m:        # one superpixel row: 8 x 1 and nothing taller
        assert m.rgb_size(size=(8, 1)) == m.rgb_size() == 256 + 8 * 3 and m.rgb_size(size=(3, 1)) == 256 + 9
        assert amd.mlvfs_amd_mount_rgb_scaled_size(m.h, 0, 8, 2) == 0 and b"scaled" in amd.mlvfs_amd_last_error()
    with mlvfile.MlvReader(clips("C.MLV", 418, 267)) as r, Mount(r, MlvfsOptions()) as m:     # odd sizes drop their last row
        assert m.rgb_size(size=(209, 133)) == 256 + 209 * 133 * 3
        assert amd.mlvfs_amd_mount_rgb_scaled_size(m.h, 0, 209, 134) == 0


def test_scaled_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in SCALE_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    for f in (Mount.rgb, Mount.jpeg, Mount.rgb_size):
        par = inspect.signature(f).parameters
        assert par["size"].default is None and par["full"].default is False and list(par).index("size") == list(par).index("full") + 1
    assert list(inspect.signature(Mount.rgb).parameters)[1:4] == ["first", "count", "gain"]
    for name in ("fit", "weights", "stages", "render"):
        assert callable(getattr(scale, name))


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/scale_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the fit writes exactly two ints, its products and the plan's overflow nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for args in FIT_GOOD:
            f.write(struct.pack("<7i", *args, 0, *scale.fit(*args)))
        for args in FIT_BAD:
            f.write(struct.pack("<7i", *args, lib.ERR_ARG, -7, -7))
    exe = tmp_path / "scale_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "scale_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"scale_host_check: {len(FIT_GOOD) + len(FIT_BAD)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
