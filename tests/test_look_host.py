"""A look for the rendered frames, the library's host code (no GPU): mlvfs_amd_look_image_size and mlvfs_amd_look_pack against the
layout computed in Python (mlvfs_amd/look.py: image), every refusal with the image untouched, the refusals of the three _look_dev
calls, of mlvfs_amd_look_apply_dev and of mlvfs_amd_mount_set_look that happen before any device work, the export table and the Python
binding -- and the same once more through a stand-alone C++ program (tests/look_host_check.cpp) built with
-fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).  Nothing is
loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_look.py, tests/test_gpu_mount_look.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, look, render, scale
from mlvfs_amd.mount import Mount

import look_cases as lc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
LOOK_SYMBOLS = ["mlvfs_amd_look_image_size", "mlvfs_amd_look_pack", "mlvfs_amd_look_create", "mlvfs_amd_look_destroy", "mlvfs_amd_look_apply_dev",
                "mlvfs_amd_render2_look_dev", "mlvfs_amd_render1_look_dev", "mlvfs_amd_render_scaled_look_dev", "mlvfs_amd_mount_set_look"]
PACKED = ["random2", "random3", "random17", "random65", "edge2", "allwhite5"]


def test_look_image_size(amd):
    for n in range(2, 66):
        assert amd.mlvfs_amd_look_image_size(n) == 8192 + 8 * n ** 3 == len(look.image(np.zeros(4096, np.uint16), n, np.zeros((n ** 3, 3), np.uint16)))
    for n in (-(1 << 31), -1, 0, 1, 66, 1 << 20):
        assert amd.mlvfs_amd_look_image_size(n) == 0 and b"2 .. 65" in amd.mlvfs_amd_last_error(), n
    assert amd.mlvfs_amd_look_image_size(33) == 295688 and amd.mlvfs_amd_look_image_size(65) == 2205192


@pytest.mark.parametrize("name", PACKED)
def test_look_pack_writes_the_layout(amd, name):
    S, n, T = lc.look_of(name)
    want = np.frombuffer(look.image(S, n, T), np.uint8)
    # by hand: S as it is, then per entry R, G, B, 0 -- red fastest
    assert want[:8192].tobytes() == S.astype("<u2").tobytes()
    e = want[8192:].view("<u2").reshape(n, n, n, 4)
    b, g, r = n - 1, 0, 1
    assert e[b, g, r].tolist() == T[(b * n + g) * n + r].tolist() + [0]
    size = want.size
    for extra in (0, 1, 64):                                     # cap: exactly the size, and anything above; the bytes behind stay
        img = np.full(size + extra + 16, 0xA5, np.uint8)
        assert amd.mlvfs_amd_look_pack(lib.ptr(S), n, lib.ptr(T), lib.ptr(img), size + extra) == 0
        assert np.array_equal(img[:size], want) and (img[size:] == 0xA5).all()
    img = np.full(size + 16, 0xA5, np.uint8)
    vp = lambda a: None if a is None else lib.ptr(a)
    for s_, n_, t_, i_, cap in ((None, n, T, img, size), (S, n, None, img, size), (S, n, T, None, size), (S, n, T, img, size - 1), (S, n, T, img, 0),
                                (S, 1, T, img, size), (S, 66, T, img, 1 << 30), (S, 0, T, img, size), (S, -n, T, img, size), (S, 1 << 30, T, img, size)):
        assert amd.mlvfs_amd_look_pack(vp(s_), n_, vp(t_), vp(i_), cap) == lib.ERR_ARG, (n_, cap)
        assert (img == 0xA5).all()
    assert amd.mlvfs_amd_look_pack(lib.ptr(S), n, lib.ptr(T), lib.ptr(img), size - 1) == lib.ERR_ARG and b"room" in amd.mlvfs_amd_last_error()


def test_look_calls_refuse_on_the_host(amd):
    """every check happens before any device work: no pointer is followed (they are host memory here), the look's least of all"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(8192, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p, lk = src.ctypes.data, dst.ctypes.data, par.ctypes.data, dst.ctypes.data + 4096
    vp = lambda a: C.c_void_p(a) if a else None
    r2 = lambda sp, st, w, h, pp, dp, ost, n, look_: amd.mlvfs_amd_render2_look_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(look_), None)
    r1 = lambda sp, st, w, h, pp, dp, ost, n, look_: amd.mlvfs_amd_render1_look_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(look_), None)
    rs = lambda sp, st, w, h, pp, dp, ost, n, look_: amd.mlvfs_amd_render_scaled_look_dev(vp(sp), st, w, h, vp(pp), 7, 3, vp(dp), ost, n, vp(look_), None)
    for call, who in ((r2, b"render2"), (r1, b"render1"), (rs, b"render_scaled")):
        for args in ((s, 512, 32, 8, p, d, 1024, 1, 0), (0, 512, 32, 8, p, d, 1024, 1, lk), (s, 512, 32, 8, 0, d, 1024, 1, lk), (s, 512, 32, 8, p, 0, 1024, 1, lk)):
            assert call(*args) == lib.ERR_ARG and who + b": null" in amd.mlvfs_amd_last_error(), (who, args)
        for w, h in ((1, 16), (16, 1), (0, 16), (16, -1), (1 << 14, 1 << 13)):
            assert call(s, 512, w, h, p, d, 1024, 1, lk) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (who, w, h)
        assert call(s, 512, 32, 8, p, d, 1024, -1, lk) == lib.ERR_ARG
        assert call(s, 510, 32, 8, p, d, 1024, 2, lk) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()
        assert call(s, 512, 32, 8, p, d, 40, 2, lk) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()
        assert call(s, 513, 32, 8, p, d, 1024, 2, lk) == lib.ERR_ARG
        assert call(s + 1, 512, 32, 8, p, d, 1024, 1, lk) == lib.ERR_ARG and call(s, 512, 32, 8, p + 2, d, 1024, 1, lk) == lib.ERR_ARG
        for dp in (s, s + 128, s + 511, p, p + 51):
            assert call(s, 512, 32, 8, p, dp, 1024, 1, lk) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (who, dp - s)
        assert call(s, 512, 32, 8, p, d, 1024, 0, lk) == 0                      # nothing to do
    assert r1(s, 512, 2, 2, p, d, 1024, 1, lk) == lib.ERR_ARG
    for ow, oh in ((0, 3), (7, 0), (17, 3), (7, 5)):
        assert amd.mlvfs_amd_render_scaled_look_dev(vp(s), 512, 32, 8, vp(p), ow, oh, vp(d), 1024, 1, vp(lk), None) == lib.ERR_ARG
    ap = lambda look_, tp, n, dp: amd.mlvfs_amd_look_apply_dev(vp(look_), vp(tp), n, vp(dp), None)
    for args in ((0, s, 8, d), (lk, 0, 8, d), (lk, s, 8, 0), (lk, s + 1, 8, d), (lk, s, 8, s), (lk, s, 8, s + 47), (lk, s + 24, 8, s + 1), (lk, s, 1 << 41, d)):
        assert ap(*args) == lib.ERR_ARG, args
    assert ap(lk, s, 0, d) == 0
    assert amd.mlvfs_amd_mount_set_look(None, vp(lk)) == lib.ERR_ARG and amd.mlvfs_amd_mount_set_look(None, None) == lib.ERR_ARG
    S, n, T = lc.look_of("random3")
    for s_, n_, t_ in ((None, n, lib.ptr(T)), (lib.ptr(S), n, None), (lib.ptr(S), 1, lib.ptr(T)), (lib.ptr(S), 66, lib.ptr(T))):
        assert not amd.mlvfs_amd_look_create(s_, n_, t_)
    amd.mlvfs_amd_look_destroy(None)
    assert (src == 7).all() and (dst == 9).all() and not par.any()


def test_look_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in LOOK_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    for f in (render.render, demosaic.render, scale.render):
        assert inspect.signature(f).parameters["look"].default is None
    assert callable(Mount.set_look) and list(inspect.signature(look.Look.__init__).parameters)[1:] == ["shaper", "n", "table"]
    for name in ("apply", "stages", "read_cube", "identity", "shaper_srgb", "shaper_linear", "shaper_log2"):
        assert callable(getattr(look, name))


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/look_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the packing reads exactly S and T and writes exactly the image, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for name in PACKED:
            S, n, T = lc.look_of(name)
            f.write(struct.pack("<i", n) + S.astype("<u2").tobytes() + T.astype("<u2").tobytes() + look.image(S, n, T))
    exe = tmp_path / "look_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "look_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"look_host_check: {len(PACKED)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
