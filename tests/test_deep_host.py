"""Rendered frames at 16 bits, the library's host code (no GPU): mlvfs_amd_look16_image_size and mlvfs_amd_look16_pack against the layout
computed in Python (mlvfs_amd/look.py: image16), mlvfs_amd_rgb16_header against render.tiff_header(bits=16), every refusal of the three
_deep_dev calls, of mlvfs_amd_look16_apply_dev and of the mount's 16-bit calls that happens before any device work, with no pointer
followed, the export table and the Python binding -- and the same once more through a stand-alone C++ program
(tests/deep_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`,
built here if it is not yet).  Nothing is loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_deep.py,
tests/test_gpu_mount_deep.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, look, render

import deep_cases as dp
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
DEEP_SYMBOLS = ["mlvfs_amd_look16_image_size", "mlvfs_amd_look16_pack", "mlvfs_amd_look16_create", "mlvfs_amd_look16_destroy",
                "mlvfs_amd_look16_apply_dev", "mlvfs_amd_rgb16_header", "mlvfs_amd_render2_deep_dev", "mlvfs_amd_render1_deep_dev",
                "mlvfs_amd_render_scaled_deep_dev", "mlvfs_amd_mount_rgb16", "mlvfs_amd_mount_rgb16_full", "mlvfs_amd_mount_rgb16_scaled",
                "mlvfs_amd_mount_rgb16_size", "mlvfs_amd_mount_rgb16_full_size", "mlvfs_amd_mount_rgb16_scaled_size"]
PACKED = ["linear0", "case0", "random2", "random3", "random65", "edge2"]


def test_look16_image_size(amd):
    S = np.zeros(65536, np.uint16)
    assert amd.mlvfs_amd_look16_image_size(0) == 131072 == len(look.image16(S))
    for n in range(2, 66):
        assert amd.mlvfs_amd_look16_image_size(n) == 131072 + 8 * n ** 3 == len(look.image16(S, n, np.zeros((n ** 3, 3), np.uint16)))
    for n in (-(1 << 31), -1, 1, 66, 1 << 20):
        assert amd.mlvfs_amd_look16_image_size(n) == 0 and b"2 .. 65" in amd.mlvfs_amd_last_error(), n


@pytest.mark.parametrize("name", PACKED)
def test_look16_pack_writes_the_layout(amd, name):
    S, n, T = dp.look_of(name)
    S = np.ascontiguousarray(S, np.uint16)
    want = np.frombuffer(look.image16(S, n, T), np.uint8)
    assert want[:131072].tobytes() == S.astype("<u2").tobytes()
    if n:
        e = want[131072:].view("<u2").reshape(n, n, n, 4)
        b, g, r = n - 1, 0, 1
        assert e[b, g, r].tolist() == T[(b * n + g) * n + r].tolist() + [0]
    size = want.size
    vp = lambda a: None if a is None else lib.ptr(a)
    for extra in (0, 1, 64):                                     # cap: exactly the size, and anything above; the bytes behind stay
        img = np.full(size + extra + 16, 0xA5, np.uint8)
        assert amd.mlvfs_amd_look16_pack(lib.ptr(S), n, vp(T), lib.ptr(img), size + extra) == 0
        assert np.array_equal(img[:size], want) and (img[size:] == 0xA5).all()
    img = np.full(size + 80, 0xA5, np.uint8)
    T2 = np.zeros((8, 3), np.uint16)
    for s_, n_, t_, i_, cap in ((None, n, T, img, size), (S, n or 2, None, img, size + 80), (S, n, T, None, size), (S, n, T, img, size - 1), (S, n, T, img, 0),
                                (S, 1, T2, img, size), (S, 66, T2, img, 1 << 30), (S, -2, T2, img, size), (S, 1 << 30, T2, img, size)):
        assert amd.mlvfs_amd_look16_pack(vp(s_), n_, vp(t_), vp(i_), cap) == lib.ERR_ARG, (n_, cap)
        assert (img == 0xA5).all()
    assert amd.mlvfs_amd_look16_pack(lib.ptr(S), n, vp(T), lib.ptr(img), size - 1) == lib.ERR_ARG and b"room" in amd.mlvfs_amd_last_error()


@pytest.mark.parametrize("pw,ph", [(1, 1), (7, 5), (1792, 660), (3584, 1320), (5792, 5792)])
def test_rgb16_header(amd, pw, ph):
    buf = np.full(300, 0xA5, np.uint8)
    assert amd.mlvfs_amd_rgb16_header(pw, ph, lib.ptr(buf), 256) == 256
    assert buf[:256].tobytes() == render.tiff_header(pw, ph, bits=16) and (buf[256:] == 0xA5).all()
    h8 = np.zeros(256, np.uint8)
    assert amd.mlvfs_amd_rgb_header(pw, ph, lib.ptr(h8), 256) == 256 and h8.tobytes() == render.tiff_header(pw, ph)
    differ = set(np.flatnonzero(h8 != buf[:256]).tolist())
    assert {158, 160, 162} <= differ <= {158, 160, 162, 126, 127, 128, 129}
    assert struct.unpack_from("<I", buf, 126)[0] == 6 * pw * ph and struct.unpack_from("<3H", buf, 158) == (16, 16, 16)


def test_rgb16_header_refusals(amd):
    buf = np.full(300, 0xA5, np.uint8)
    for pw, ph, out, cap in ((0, 5, buf, 256), (5, 0, buf, 256), (-1, 5, buf, 256), (1 << 13, 1 << 12, buf, 256), (7, 5, None, 256), (7, 5, buf, 255), (7, 5, buf, 0)):
        assert amd.mlvfs_amd_rgb16_header(pw, ph, None if out is None else lib.ptr(out), cap) == 0 and b"rgb16_header" in amd.mlvfs_amd_last_error()
    assert (buf == 0xA5).all()


def test_deep_calls_refuse_on_the_host(amd):
    """every check happens before any device work: no pointer is followed (they are host memory here), the look's least of all"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(16384, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p, lk = src.ctypes.data, dst.ctypes.data, par.ctypes.data, dst.ctypes.data + 8192
    vp = lambda a: C.c_void_p(a) if a else None
    r2 = lambda sp, st, w, h, pp, dp_, ost, n, look_: amd.mlvfs_amd_render2_deep_dev(vp(sp), st, w, h, vp(pp), vp(dp_), ost, n, vp(look_), None)
    r1 = lambda sp, st, w, h, pp, dp_, ost, n, look_: amd.mlvfs_amd_render1_deep_dev(vp(sp), st, w, h, vp(pp), vp(dp_), ost, n, vp(look_), None)
    rs = lambda sp, st, w, h, pp, dp_, ost, n, look_: amd.mlvfs_amd_render_scaled_deep_dev(vp(sp), st, w, h, vp(pp), 7, 3, vp(dp_), ost, n, vp(look_), None)
    # a 32 x 8 frame: 512 bytes in; 384, 1536 or 126 bytes out
    for call, who, pimg in ((r2, b"render2", 384), (r1, b"render1", 1536), (rs, b"render_scaled", 126)):
        for args in ((s, 512, 32, 8, p, d, 2048, 1, 0), (0, 512, 32, 8, p, d, 2048, 1, lk), (s, 512, 32, 8, 0, d, 2048, 1, lk), (s, 512, 32, 8, p, 0, 2048, 1, lk)):
            assert call(*args) == lib.ERR_ARG and who + b": null" in amd.mlvfs_amd_last_error(), (who, args)
        for w, h in ((1, 16), (16, 1), (0, 16), (16, -1), (1 << 14, 1 << 13)):
            assert call(s, 512, w, h, p, d, 2048, 1, lk) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (who, w, h)
        assert call(s, 512, 32, 8, p, d, 2048, -1, lk) == lib.ERR_ARG
        assert call(s, 510, 32, 8, p, d, 2048, 2, lk) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()
        # the stride checks use 6 bytes per pixel: one byte short of a rendering is refused, the rendering's size is not (then the
        # overlap check refuses what overlaps: the destination here is the source)
        assert call(s, 512, 32, 8, p, d, pimg - 1, 2, lk) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()
        assert call(s, 512, 32, 8, p, s, pimg, 2, lk) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error()
        assert call(s, 513, 32, 8, p, d, 2048, 2, lk) == lib.ERR_ARG
        assert call(s + 1, 512, 32, 8, p, d, 2048, 1, lk) == lib.ERR_ARG and call(s, 512, 32, 8, p + 2, d, 2048, 1, lk) == lib.ERR_ARG
        for dp_ in (s, s + 128, s + 511, s - pimg + 1, p, p + 51):
            assert call(s, 512, 32, 8, p, dp_, 2048, 1, lk) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (who, dp_ - s)
        assert call(s, 512, 32, 8, p, d, 2048, 0, lk) == 0                      # nothing to do
    assert r1(s, 512, 2, 2, p, d, 2048, 1, lk) == lib.ERR_ARG
    for ow, oh in ((0, 3), (7, 0), (17, 3), (7, 5)):
        assert amd.mlvfs_amd_render_scaled_deep_dev(vp(s), 512, 32, 8, vp(p), ow, oh, vp(d), 2048, 1, vp(lk), None) == lib.ERR_ARG
    ap = lambda look_, tp, n, dp_: amd.mlvfs_amd_look16_apply_dev(vp(look_), vp(tp), n, vp(dp_), None)
    for args in ((0, s, 8, d), (lk, 0, 8, d), (lk, s, 8, 0), (lk, s + 1, 8, d), (lk, s, 8, d + 1), (lk, s, 8, s), (lk, s, 8, s + 46), (lk, s + 46, 8, s),
                 (lk, s, 1 << 41, d)):
        assert ap(*args) == lib.ERR_ARG, args
    assert ap(lk, s, 0, d) == 0
    S, n, T = dp.look_of("random3")
    for s_, n_, t_ in ((None, n, lib.ptr(T)), (lib.ptr(S), n, None), (lib.ptr(S), 1, lib.ptr(T)), (lib.ptr(S), 66, lib.ptr(T)), (None, 0, None)):
        assert not amd.mlvfs_amd_look16_create(s_, n_, t_)
    amd.mlvfs_amd_look16_destroy(None)
    # the mount's calls: a null deep look, a null handle, a gain and a size that are none -- before the handle is followed (d is no handle)
    res = np.full(2, 5, np.int32)
    m = lambda *a: amd.mlvfs_amd_mount_rgb16(*a)
    for call, size in ((amd.mlvfs_amd_mount_rgb16, ()), (amd.mlvfs_amd_mount_rgb16_full, ()), (amd.mlvfs_amd_mount_rgb16_scaled, (7, 3))):
        assert call(vp(d), 0, 1, vp(d + 4096), 2048, 256, *size, None, 2, 0, lib.ptr(res)) == lib.ERR_ARG and b"deep look" in amd.mlvfs_amd_last_error()
        assert call(None, 0, 1, vp(d + 4096), 2048, 256, *size, vp(lk), 2, 0, lib.ptr(res)) == lib.ERR_ARG
        for gain in (0, -1, 65536):
            assert call(vp(d), 0, 1, vp(d + 4096), 2048, gain, *size, vp(lk), 2, 0, lib.ptr(res)) == lib.ERR_ARG and b"gain_q8" in amd.mlvfs_amd_last_error()
    for ow, oh in ((0, 3), (7, 0), (-7, 3)):
        assert amd.mlvfs_amd_mount_rgb16_scaled(vp(d), 0, 1, vp(d + 4096), 2048, 256, ow, oh, vp(lk), 2, 0, lib.ptr(res)) == lib.ERR_ARG
    assert amd.mlvfs_amd_mount_rgb16_size(None, 0) == 0 and amd.mlvfs_amd_mount_rgb16_full_size(None, 0) == 0
    assert amd.mlvfs_amd_mount_rgb16_scaled_size(None, 0, 7, 3) == 0
    assert (src == 7).all() and (dst == 9).all() and not par.any() and (res == 5).all()


def test_deep_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in DEEP_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert amd.mlvfs_amd_look16_image_size.restype == C.c_size_t and amd.mlvfs_amd_mount_rgb16_scaled_size.restype == C.c_size_t
    assert amd.mlvfs_amd_look16_create.restype == C.c_void_p


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/deep_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the packing reads exactly S16 and T and writes exactly the image, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for name in PACKED:
            S, n, T = look._look16(*dp.look_of(name))
            f.write(struct.pack("<i", n) + S.astype("<u2").tobytes() + T.astype("<u2").tobytes() + look.image16(S, n, T if n else None))
    exe = tmp_path / "deep_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "deep_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"deep_host_check: {len(PACKED)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
