"""Rendered full-size frames demosaiced by AMaZE, the library's host code (no GPU): mlvfs_amd_rgb_amaze_geom, the sub-batch arithmetic
(mlvfs_amd_test_amaze_render_plan), every refusal of mlvfs_amd_amaze_balance_dev, mlvfs_amd_amaze_tone_dev, the three
mlvfs_amd_render1_amaze calls and the mount's setter that happens before any device work, the export table and the Python binding --
and the geometry, the arithmetic and the refusals once more through a stand-alone C++ program (tests/amaze_render_host_check.cpp) built
with -fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).
Nothing is loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_amaze_render.py, tests/test_gpu_mount_amaze.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import amaze_render, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import amaze_render_cases as ac
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
SYMBOLS = ["mlvfs_amd_rgb_amaze_geom", "mlvfs_amd_amaze_balance_dev", "mlvfs_amd_amaze_tone_dev", "mlvfs_amd_render1_amaze_dev",
           "mlvfs_amd_render1_amaze_look_dev", "mlvfs_amd_render1_amaze_deep_dev", "mlvfs_amd_mount_set_demosaic",
           "mlvfs_amd_test_amaze_render_plan"]
GOOD = ac.SIZES + [ac.FAST_SIZE, (ac.BIG_W, ac.BIG_H), (36, 1 << 19), (8188, 4097), (5792, 5792)]
BAD = [(34, 36), (36, 35), (32, 32), (38, 38), (37, 37), (39, 40), (4, 4), (16, 8), (0, 0), (-36, 36), (36, -36), (1 << 13, 1 << 12),
       (1 << 25, 36), (5796, 5796), (1 << 30, 1 << 30)]

TILE_FLOATS = 13 * 160 * 160 + 13 * 160 * 160 // 2          # amaze_demosaic_RT.c's planes of one 160 x 160 tile
CAP = 6 << 30


def plan_restated(w, h, n, cap):
    """four float planes of W H floats rounded up to 64, and a block of planes for every tile of the grid that advances by 128 and
    starts 16 before the image; as many frames as fit the cap, at least one, at most the batch"""
    plane = (w * h + 63) // 64 * 64
    tiles = -(-(w + 16) // 128) * -(-(h + 16) // 128) * TILE_FLOATS
    frame = 4 * (4 * plane + tiles)
    return [plane, tiles, frame, min(max((cap or CAP) // frame, 1), n)]


def plan_cases():
    frame = plan_restated(ac.BIG_W, ac.BIG_H, 1, 0)[2]
    out = [(ac.BIG_W, ac.BIG_H, n, cap) for n in (1, 3, 8, 9, 10, 64)
           for cap in (0, 1, frame - 1, frame, frame + 1, 2 * frame - 1, 3 * frame + 5, 8 * frame, 1 << 40)]
    out += [(w, h, n, cap) for w, h in ac.SIZES + [ac.FAST_SIZE, (1920, 1080), (5792, 5792)] for n in (1, 8, 1000) for cap in (0, 1 << 20, 1 << 28)]
    return out


def geom(amd, w, h):
    pw, ph = C.c_int(-7), C.c_int(-7)
    return amd.mlvfs_amd_rgb_amaze_geom(w, h, C.byref(pw), C.byref(ph)), pw.value, ph.value


def plan(amd, w, h, n, cap):
    out = np.full(4, -7, np.int64)
    return amd.mlvfs_amd_test_amaze_render_plan(w, h, n, cap, lib.ptr(out)), list(out)


def test_rgb_amaze_geom(amd):
    for w, h in GOOD:
        assert geom(amd, w, h) == (0, w, h) == (0,) + amaze_render.geom(w, h), (w, h)
    for w, h in BAD:
        assert geom(amd, w, h) == (lib.ERR_ARG, -7, -7) and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
        with pytest.raises(ValueError):
            amaze_render.geom(w, h)
    one = C.c_int(5)
    assert amd.mlvfs_amd_rgb_amaze_geom(64, 64, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_rgb_amaze_geom(64, 64, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def test_sub_batch_arithmetic(amd):
    """0.71 GB per 3584 x 1320 frame; a batch of 8 fits the library's cap in one piece, one of 10 goes in sub-batches of 9; no cap is
    too small for one frame"""
    assert plan(amd, ac.BIG_W, ac.BIG_H, 8, 0) == (0, [4730880, 319 * TILE_FLOATS, 712673280, 8])
    assert plan(amd, ac.BIG_W, ac.BIG_H, 10, 0)[1][3] == 9 and plan(amd, ac.BIG_W, ac.BIG_H, 10, 1)[1][3] == 1
    for w, h, n, cap in plan_cases():
        assert plan(amd, w, h, n, cap) == (0, plan_restated(w, h, n, cap)), (w, h, n, cap)
    for w, h, n in ((34, 36, 1), (36, 36, 0), (36, 36, -1), (1 << 13, 1 << 12, 1)):
        assert plan(amd, w, h, n, 0) == (lib.ERR_ARG, [-7] * 4), (w, h, n)
    assert amd.mlvfs_amd_test_amaze_render_plan(64, 64, 1, 0, None) == lib.ERR_ARG


def test_the_device_calls_refuse_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    W, H, IMG, NP, OUT = 48, 36, 3456, 1728, 5184
    src, pl, dst, par = np.full(3 * NP, 0x0707, np.uint16), np.full(9 * NP, 5.0, np.float32), np.full(6 * OUT, 9, np.uint8), np.zeros(64, np.int32)
    s, q, d, p = src.ctypes.data, pl.ctypes.data, dst.ctypes.data, par.ctypes.data
    qr, qg, qb = q, q + 12 * NP, q + 24 * NP
    vp = lambda a: C.c_void_p(a) if a else None
    bal = lambda sp, st, w, h, pp, qp, ps, n: amd.mlvfs_amd_amaze_balance_dev(vp(sp), st, w, h, vp(pp), vp(qp), ps, n, None)
    tone = lambda r, g, b, ps, w, h, pp, dp, ost, n, l=0, l16=0: amd.mlvfs_amd_amaze_tone_dev(vp(r), vp(g), vp(b), ps, w, h, vp(pp), vp(dp), ost, n, vp(l), vp(l16), None)
    r1 = lambda sp, st, w, h, pp, dp, ost, n: amd.mlvfs_amd_render1_amaze_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    err = amd.mlvfs_amd_last_error
    # balance
    for args in ((0, IMG, W, H, p, q, NP, 1), (s, IMG, W, H, 0, q, NP, 1), (s, IMG, W, H, p, 0, NP, 1)):
        assert bal(*args) == lib.ERR_ARG and b"null" in err(), args
    for w, h in ((34, H), (W, 35), (46, H), (16, 8), (0, 0), (-48, H), (1 << 13, 1 << 12)):
        assert bal(s, IMG, w, h, p, q, NP, 1) == lib.ERR_ARG and b"not supported" in err(), (w, h)
        assert tone(qr, qg, qb, NP, w, h, p, d, OUT, 1) == lib.ERR_ARG and b"not supported" in err(), (w, h)
        assert r1(s, IMG, w, h, p, d, OUT, 1) == lib.ERR_ARG and b"not supported" in err(), (w, h)
    assert bal(s, IMG, W, H, p, q, NP, -1) == lib.ERR_ARG
    for st, ps in ((IMG - 2, NP), (IMG, NP - 1), (IMG + 1, NP)):
        assert bal(s, st, W, H, p, q, ps, 2) == lib.ERR_ARG and b"stride" in err(), (st, ps)
    assert bal(s + 1, IMG, W, H, p, q, NP, 1) == lib.ERR_ARG and bal(s, IMG, W, H, p + 2, q, NP, 1) == lib.ERR_ARG and bal(s, IMG, W, H, p, q + 2, NP, 1) == lib.ERR_ARG
    for qp in (s, s + IMG - 4, s - 4 * NP + 4, p, p + 48):
        assert bal(s, IMG, W, H, p, qp, NP, 1) == lib.ERR_ARG and b"overlap" in err(), qp - s
    assert bal(s, IMG, W, H, p, q, NP, 0) == 0
    # tone
    for args in ((0, qg, qb), (qr, 0, qb), (qr, qg, 0)):
        assert tone(*args, NP, W, H, p, d, OUT, 1) == lib.ERR_ARG and b"null" in err()
    assert tone(qr, qg, qb, NP, W, H, 0, d, OUT, 1) == lib.ERR_ARG and tone(qr, qg, qb, NP, W, H, p, 0, OUT, 1) == lib.ERR_ARG
    assert tone(qr, qg, qb, NP, W, H, p, d, OUT, 1, s, s) == lib.ERR_ARG and b"deep look" in err()           # both set: neither is followed
    assert tone(qr, qg, qb, NP, W, H, p, d, OUT, -1) == lib.ERR_ARG
    assert tone(qr, qg, qb, NP - 1, W, H, p, d, OUT, 2) == lib.ERR_ARG and b"stride" in err()
    assert tone(qr, qg, qb, NP, W, H, p, d, OUT - 1, 2) == lib.ERR_ARG and b"stride" in err()
    assert tone(qr, qg, qb, NP, W, H, p, d, 2 * OUT - 1, 2, 0, s) == lib.ERR_ARG and b"stride" in err()     # 6 bytes per pixel with a deep look
    assert tone(qr + 2, qg, qb, NP, W, H, p, d, OUT, 1) == lib.ERR_ARG and tone(qr, qg, qb, NP, W, H, p + 2, d, OUT, 1) == lib.ERR_ARG
    for dp in (qr, qg + 100, qb + 4 * NP - 1, qr - OUT + 1, p, p + 51):
        assert tone(qr, qg, qb, NP, W, H, p, dp, OUT, 1) == lib.ERR_ARG and b"overlap" in err(), dp - q
    assert tone(qr, qg, qb, NP, W, H, p, d, OUT, 0) == 0
    # the three passes in one call: render1's checks
    for args in ((0, IMG, W, H, p, d, OUT, 1), (s, IMG, W, H, 0, d, OUT, 1), (s, IMG, W, H, p, 0, OUT, 1)):
        assert r1(*args) == lib.ERR_ARG and b"null" in err(), args
    assert r1(s, IMG, W, H, p, d, OUT, -1) == lib.ERR_ARG
    for st, ost in ((IMG - 2, OUT), (IMG, OUT - 1), (IMG + 1, OUT)):
        assert r1(s, st, W, H, p, d, ost, 2) == lib.ERR_ARG and b"stride" in err(), (st, ost)
    assert r1(s + 1, IMG, W, H, p, d, OUT, 1) == lib.ERR_ARG and r1(s, IMG, W, H, p + 2, d, OUT, 1) == lib.ERR_ARG
    for dp in (s, s + IMG - 1, s - OUT + 1, p, p + 51, p - OUT + 1):
        assert r1(s, IMG, W, H, p, dp, OUT, 1) == lib.ERR_ARG and b"overlap" in err(), dp - s
    assert amd.mlvfs_amd_render1_amaze_look_dev(vp(s), IMG, W, H, vp(p), vp(d), OUT, 1, None, None) == lib.ERR_ARG and b"null" in err()
    assert amd.mlvfs_amd_render1_amaze_deep_dev(vp(s), IMG, W, H, vp(p), vp(d), 2 * OUT, 1, None, None) == lib.ERR_ARG and b"null" in err()
    assert amd.mlvfs_amd_render1_amaze_deep_dev(vp(s), IMG, W, H, vp(p), vp(d), 2 * OUT - 1, 2, vp(s), None) == lib.ERR_ARG and b"stride" in err()
    assert r1(s, IMG, W, H, p, d, OUT, 0) == 0                                   # nothing to do
    assert (src == 0x0707).all() and (pl == 5.0).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_set_demosaic_on_the_host(amd, clips):
    """the setter, the size call and the refusals that need no device: frames AMaZE does not take, the resampled calls, a proxy handle"""
    assert amd.mlvfs_amd_mount_set_demosaic(None, 1) == lib.ERR_ARG
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r, Mount(r, MlvfsOptions()) as m:
        size = 256 + 64 * 48 * 3
        assert m.demosaic == "linear" and m.rgb_size(full=True) == size
        for which in (2, -1, 256):
            assert amd.mlvfs_amd_mount_set_demosaic(m.h, which) == lib.ERR_ARG and b"demosaic" in amd.mlvfs_amd_last_error()
        with pytest.raises(ValueError):
            m.set_demosaic("bilinear")
        m.set_demosaic("amaze")
        assert m.demosaic == "amaze" and m.rgb_size(full=True) == size and m.rgb_size(full=True, bits=16) == 256 + 64 * 48 * 6
        assert m.rgb_size() == 256 + 32 * 24 * 3 and m.rgb_size(size=(20, 10), resample=True) == 256 + 600      # the sizes of the other calls stay
        out = np.full(2 * size, 0xA5, np.uint8)
        sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
        assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, O, size, 256, 20, 10, 2, 1, None) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, O, size, 256, 90, 20, 10, S, F, 2, 1, None) == lib.ERR_ARG and b"AMaZE" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, O, size, 256, 20, 10, O, 2, 1, None) == lib.ERR_ARG and b"AMaZE" in amd.mlvfs_amd_last_error()
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, size=(20, 10), resample=True)
        assert amd.mlvfs_amd_mount_rgb_full(m.h, 0, 2, O, size - 1, 256, 2, 1, None) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
        m.set_proxy(2)                                                           # nothing was served: a refusal serves nothing
        assert amd.mlvfs_amd_mount_rgb_full(m.h, 0, 2, O, size, 256, 2, 1, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_jpeg_full(m.h, 0, 2, O, size, 256, 90, S, F, 2, 1, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
        m.set_demosaic("linear")
        assert m.demosaic == "linear"
    for name, w, h in (("B.MLV", 34, 40), ("C.MLV", 40, 34), ("D.MLV", 38, 40)):           # the linear filter takes them, AMaZE does not
        with mlvfile.MlvReader(clips(name, w, h)) as r, Mount(r, MlvfsOptions()) as m:
            size = 256 + w * h * 3
            assert amd.mlvfs_amd_mount_rgb_full_size(m.h, 0) == size
            m.set_demosaic("amaze")
            assert amd.mlvfs_amd_mount_rgb_full_size(m.h, 0) == 0 and b"36x36" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_rgb16_full_size(m.h, 0) == 0
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(full=True)
            out = np.full(size, 0xA5, np.uint8)
            assert amd.mlvfs_amd_mount_rgb_full(m.h, 0, 1, lib.ptr(out), size, 256, 1, 1, None) == lib.ERR_ARG and b"36x36" in amd.mlvfs_amd_last_error()
            assert (out == 0xA5).all() and m.rgb_size() == 256 + (w // 2) * (h // 2) * 3
            m.set_demosaic("linear")
            assert amd.mlvfs_amd_mount_rgb_full_size(m.h, 0) == size


def test_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert Mount.DEMOSAICS == {"linear": 0, "amaze": 1}


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/amaze_render_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and
    run directly: the geometry writes exactly two ints, the plan exactly four, the arithmetic overflows nowhere, and the refusals follow
    no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    geoms, plans = tmp_path / "geom.bin", tmp_path / "plan.bin"
    with open(geoms, "wb") as f:
        for w, h in GOOD:
            f.write(struct.pack("<5i", w, h, 0, w, h))
        for w, h in BAD:
            f.write(struct.pack("<5i", w, h, lib.ERR_ARG, -7, -7))
    cases = plan_cases()
    with open(plans, "wb") as f:
        for w, h, n, cap in cases:
            f.write(struct.pack("<9q", w, h, n, cap, 0, *plan_restated(w, h, n, cap)))
        for w, h, n in ((34, 36, 1), (36, 36, 0), (1 << 13, 1 << 12, 1)):
            f.write(struct.pack("<9q", w, h, n, 0, lib.ERR_ARG, -7, -7, -7, -7))
    exe = tmp_path / "amaze_render_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "amaze_render_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(geoms), str(plans)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"amaze_render_host_check: {len(GOOD) + len(BAD)} records, {len(cases) + 3} plans" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
