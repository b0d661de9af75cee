"""Resampled rendered frames demosaiced by AMaZE, the library's host code (no GPU): mlvfs_amd_rgb_amaze_resample_geom, the plan of the
fast form (mlvfs_amd_test_amz_resample_plan), every refusal of mlvfs_amd_amaze_resample_dev and the three
mlvfs_amd_render_resampled_amaze calls that happens before any device work, the mount's setter and size calls, the export table and the
Python binding -- and the geometry, the plan and the refusals once more through a stand-alone C++ program
(tests/amaze_resample_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of the host code
(`make hostcheck`, built here if it is not yet).  Nothing is loaded into Python under a sanitizer.  The GPU side:
tests/test_gpu_amaze_resample.py, tests/test_gpu_mount_amaze_resampled.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import amaze_resample, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import amaze_resample_cases as arc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
SYMBOLS = ["mlvfs_amd_rgb_amaze_resample_geom", "mlvfs_amd_amaze_resample_dev", "mlvfs_amd_render_resampled_amaze_dev",
           "mlvfs_amd_render_resampled_amaze_look_dev", "mlvfs_amd_render_resampled_amaze_deep_dev", "mlvfs_amd_mount_set_resample_demosaic",
           "mlvfs_amd_test_amz_resample_plan"]
GOOD_FRAMES = arc.SOURCES + [(arc.BIG_W, arc.BIG_H), (36, 65535), (65532, 500), (5792, 5792)]
BAD_FRAMES = [(34, 36), (36, 35), (32, 32), (38, 38), (37, 37), (4, 4), (16, 8), (0, 0), (-36, 36), (36, -36), (1 << 13, 1 << 12), (36, 65536),
              (36, 1 << 19), (65536, 36), (1 << 25, 36), (5796, 5796), (1 << 30, 1 << 30)]


def geom_cases():
    """[(w, h, ow, oh, expected return code)]"""
    out = []
    for w, h in GOOD_FRAMES:
        out += [(w, h, ow, oh, 0) for ow, oh in arc.out_sizes(w, h)]
        out += [(w, h, ow, oh, lib.ERR_ARG) for ow, oh in ((0, 1), (1, 0), (w + 1, h), (w, h + 1), (-1, -1), (1 << 30, 1 << 30), (-w, -h))]
    out += [(w, h, 1, 1, lib.ERR_ARG) for w, h in BAD_FRAMES]
    return out


def plan_restated(w, h, ow, oh, n):
    """the fast form where W % 8 == 0 and 2 ow >= W; strips of (512 - 16) ow / W output columns -- 256 unless they fill half of a lane's
    second column --, and as many bands as give 1024 workgroups a launch, none of less than 32 source rows"""
    if w % 8 or 2 * ow < w:
        return [0, 512, 0, 0, 0, 0, 32, 4]
    uo = 496 * ow // w
    if 256 < uo < 384:
        uo = 256
    uo = min(max(uo, 1), ow)
    ns = -(-ow // uo)
    nb = min(max(max(1024 // n, 32) // ns, 1), oh)
    bo = min(max(-(-oh // nb), -(-32 * oh // h)), oh)
    return [1, 512, uo, ns, bo, -(-oh // bo), 32, 4]


def plan_cases():
    out = [(w, h, ow, oh, n) for w, h in arc.SOURCES for ow, oh in arc.out_sizes(w, h) for n in (1, 3)]
    out += [(arc.BIG_W, arc.BIG_H, ow, oh, n) for ow, oh in ((1920, 707), (2560, 943), (3584, 1320), (1792, 660), (1791, 1320), (3583, 1)) for n in (1, 8, 64, 2000)]
    out += [(65528, 500, 40000, 300, 1), (40, 65535, 39, 65535, 2), (5792, 5792, 5792, 3000, 8)]
    return out


def plan(amd, w, h, ow, oh, n):
    out = np.full(8, -7, np.int32)
    return amd.mlvfs_amd_test_amz_resample_plan(w, h, ow, oh, n, lib.ptr(out)), list(out)


def test_rgb_amaze_resample_geom(amd):
    for w, h, ow, oh, rc in geom_cases():
        assert amd.mlvfs_amd_rgb_amaze_resample_geom(w, h, ow, oh) == rc, (w, h, ow, oh)
        if rc:
            assert b"not supported" in amd.mlvfs_amd_last_error()
            with pytest.raises(ValueError):
                amaze_resample.geom(w, h, ow, oh)
        else:
            assert amaze_resample.geom(w, h, ow, oh) == (w, h)
    ow, oh = C.c_int(), C.c_int()
    assert amd.mlvfs_amd_rgb_fit_full(3584, 1320, 1920, 1080, C.byref(ow), C.byref(oh)) == 0 and (ow.value, oh.value) == (1920, 707)
    assert amd.mlvfs_amd_rgb_amaze_resample_geom(3584, 1320, ow.value, oh.value) == 0


def test_the_plan(amd):
    """3584 x 1320 to 1920 x 707 in batches of 8: strips of 256 columns, 128 workgroups a frame"""
    assert plan(amd, arc.BIG_W, arc.BIG_H, 1920, 707, 8) == (0, [1, 512, 256, 8, 45, 16, 32, 4])
    for w, h, ow, oh, n in plan_cases():
        assert plan(amd, w, h, ow, oh, n) == (0, plan_restated(w, h, ow, oh, n)), (w, h, ow, oh, n)
    for w, h, ow, oh, n in ((34, 36, 1, 1, 1), (48, 36, 48, 36, 0), (48, 36, 48, 36, -1), (48, 36, 49, 36, 1), (48, 36, 0, 0, 1), (1 << 13, 1 << 12, 1, 1, 1)):
        assert plan(amd, w, h, ow, oh, n) == (lib.ERR_ARG, [-7] * 8), (w, h, ow, oh, n)
    assert amd.mlvfs_amd_test_amz_resample_plan(64, 64, 40, 40, 1, None) == lib.ERR_ARG


def test_the_device_calls_refuse_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    W, H, IMG, NP, OW, OH, OUT = 48, 36, 3456, 1728, 30, 20, 1800
    src, pl, dst, par = np.full(3 * NP, 0x0707, np.uint16), np.full(9 * NP, 5.0, np.float32), np.full(6 * OUT, 9, np.uint8), np.zeros(64, np.int32)
    s, q, d, p = src.ctypes.data, pl.ctypes.data, dst.ctypes.data, par.ctypes.data
    qr, qg, qb = q, q + 12 * NP, q + 24 * NP
    vp = lambda a: C.c_void_p(a) if a else None
    rs = lambda r, g, b, ps, w, h, pp, ow, oh, dp, ost, n, l=0, l16=0: amd.mlvfs_amd_amaze_resample_dev(vp(r), vp(g), vp(b), ps, w, h, vp(pp), ow, oh, vp(dp), ost, n, vp(l), vp(l16), None)
    calls = {"plain": lambda sp, st, w, h, pp, ow, oh, dp, ost, n: amd.mlvfs_amd_render_resampled_amaze_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, None),
             "look": lambda sp, st, w, h, pp, ow, oh, dp, ost, n: amd.mlvfs_amd_render_resampled_amaze_look_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, vp(s), None),
             "deep": lambda sp, st, w, h, pp, ow, oh, dp, ost, n: amd.mlvfs_amd_render_resampled_amaze_deep_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), 2 * ost, n, vp(s), None)}
    err = amd.mlvfs_amd_last_error
    bad_geom = ((34, H, 1, 1), (W, 35, 1, 1), (46, H, 1, 1), (16, 8, 8, 8), (0, 0, 0, 0), (-48, H, 1, 1), (1 << 13, 1 << 12, 1, 1), (36, 65536, 1, 1),
                (W, H, 0, OH), (W, H, OW, 0), (W, H, W + 1, OH), (W, H, OW, H + 1), (W, H, -1, -1), (W, H, 1 << 30, 1 << 30))
    # the pass alone
    for args in ((0, qg, qb), (qr, 0, qb), (qr, qg, 0)):
        assert rs(*args, NP, W, H, p, OW, OH, d, OUT, 1) == lib.ERR_ARG and b"null" in err()
    assert rs(qr, qg, qb, NP, W, H, 0, OW, OH, d, OUT, 1) == lib.ERR_ARG and rs(qr, qg, qb, NP, W, H, p, OW, OH, 0, OUT, 1) == lib.ERR_ARG
    assert rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1, s, s) == lib.ERR_ARG and b"deep look" in err()           # both set: neither is followed
    for w, h, ow, oh in bad_geom:
        assert rs(qr, qg, qb, NP, w, h, p, ow, oh, d, OUT, 1) == lib.ERR_ARG and b"not supported" in err(), (w, h, ow, oh)
    assert rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, -1) == lib.ERR_ARG
    assert rs(qr, qg, qb, NP - 1, W, H, p, OW, OH, d, OUT, 2) == lib.ERR_ARG and b"stride" in err()
    assert rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT - 1, 2) == lib.ERR_ARG and b"stride" in err()
    assert rs(qr, qg, qb, NP, W, H, p, OW, OH, d, 2 * OUT - 1, 2, 0, s) == lib.ERR_ARG and b"stride" in err()     # 6 bytes per pixel with a deep look
    assert rs(qr + 2, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1) == lib.ERR_ARG and rs(qr, qg, qb, NP, W, H, p + 2, OW, OH, d, OUT, 1) == lib.ERR_ARG
    for dp in (qr, qg + 100, qb + 4 * NP - 1, qr - OUT + 1, p, p + 51):
        assert rs(qr, qg, qb, NP, W, H, p, OW, OH, dp, OUT, 1) == lib.ERR_ARG and b"overlap" in err(), dp - q
    assert rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 0) == 0
    # the three passes in one call: render1_amaze's checks with this route's geometry, in all three forms
    for form, ra in calls.items():
        for args in ((0, IMG, W, H, p, OW, OH, d, OUT, 1), (s, IMG, W, H, 0, OW, OH, d, OUT, 1), (s, IMG, W, H, p, OW, OH, 0, OUT, 1)):
            assert ra(*args) == lib.ERR_ARG and b"null" in err(), (form, args)
        for w, h, ow, oh in bad_geom:
            assert ra(s, IMG, w, h, p, ow, oh, d, OUT, 1) == lib.ERR_ARG and b"not supported" in err(), (form, w, h, ow, oh)
        assert ra(s, IMG, W, H, p, OW, OH, d, OUT, -1) == lib.ERR_ARG
        for st, ost in ((IMG - 2, OUT), (IMG + 1, OUT)):
            assert ra(s, st, W, H, p, OW, OH, d, ost, 2) == lib.ERR_ARG and b"stride" in err(), (form, st, ost)
        assert ra(s + 1, IMG, W, H, p, OW, OH, d, OUT, 1) == lib.ERR_ARG and ra(s, IMG, W, H, p + 2, OW, OH, d, OUT, 1) == lib.ERR_ARG
        for dp in (s, s + IMG - 1, p, p + 51):
            assert ra(s, IMG, W, H, p, OW, OH, dp, OUT, 1) == lib.ERR_ARG and b"overlap" in err(), (form, dp - s)
        assert ra(s, IMG, W, H, p, OW, OH, d, OUT, 0) == 0                       # nothing to do
    ra = calls["plain"]
    assert ra(s, IMG, W, H, p, OW, OH, d, OUT - 1, 2) == lib.ERR_ARG and b"stride" in err()
    for dp in (s - OUT + 1, p - OUT + 1):
        assert ra(s, IMG, W, H, p, OW, OH, dp, OUT, 1) == lib.ERR_ARG and b"overlap" in err()
    assert amd.mlvfs_amd_render_resampled_amaze_look_dev(vp(s), IMG, W, H, vp(p), OW, OH, vp(d), OUT, 1, None, None) == lib.ERR_ARG and b"null" in err()
    assert amd.mlvfs_amd_render_resampled_amaze_deep_dev(vp(s), IMG, W, H, vp(p), OW, OH, vp(d), 2 * OUT, 1, None, None) == lib.ERR_ARG and b"null" in err()
    assert amd.mlvfs_amd_render_resampled_amaze_deep_dev(vp(s), IMG, W, H, vp(p), OW, OH, vp(d), 2 * OUT - 1, 2, vp(s), None) == lib.ERR_ARG and b"stride" in err()
    assert (src == 0x0707).all() and (pl == 5.0).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_set_resample_demosaic_on_the_host(amd, clips):
    """the setter, the size calls and the refusals that need no device: the setter at 0 under set_demosaic("amaze"), frames AMaZE does
    not take, a proxy handle"""
    assert amd.mlvfs_amd_mount_set_resample_demosaic(None, 1) == lib.ERR_ARG and amd.mlvfs_amd_mount_set_resample_demosaic(None, 0) == lib.ERR_ARG
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r, Mount(r, MlvfsOptions()) as m:
        size = 256 + 20 * 10 * 3
        assert m.resample_demosaic == "linear" and m.demosaic == "linear" and m.rgb_size(size=(20, 10), resample=True) == size
        for which in (2, -1, 256):
            assert amd.mlvfs_amd_mount_set_resample_demosaic(m.h, which) == lib.ERR_ARG and b"demosaic" in amd.mlvfs_amd_last_error()
        with pytest.raises(ValueError):
            m.set_resample_demosaic("bilinear")
        out = np.full(2 * size, 0xA5, np.uint8)
        sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
        # set_demosaic("amaze") with the new setter at 0, never called or called: the resampled calls stay refused
        m.set_demosaic("amaze")
        for again in (False, True):
            if again:
                m.set_resample_demosaic("amaze")
                m.set_resample_demosaic("linear")
            assert m.resample_demosaic == "linear"
            assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, O, size, 256, 20, 10, 2, 1, None) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, O, size, 256, 90, 20, 10, S, F, 2, 1, None) == lib.ERR_ARG and b"AMaZE" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, O, size, 256, 20, 10, O, 2, 1, None) == lib.ERR_ARG and b"AMaZE" in amd.mlvfs_amd_last_error()
        m.set_demosaic("linear")
        m.set_resample_demosaic("amaze")
        assert m.resample_demosaic == "amaze" and m.demosaic == "linear"
        assert m.rgb_size(size=(20, 10), resample=True) == size and m.rgb_size(size=(64, 48), resample=True, bits=16) == 256 + 64 * 48 * 6
        assert m.rgb_size() == 256 + 32 * 24 * 3 and m.rgb_size(full=True) == 256 + 64 * 48 * 3 and m.rgb_size(size=(20, 10)) == size      # the other calls' sizes stay
        for ow, oh in ((65, 48), (64, 49), (0, 1), (1, -1)):
            assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, ow, oh) == 0 and amd.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, ow, oh) == 0
            assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, O, 65536, 256, ow, oh, 2, 1, None) == lib.ERR_ARG and b"resampled" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, O, size - 1, 256, 20, 10, 2, 1, None) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
        m.set_proxy(2)                                                           # nothing was served: a refusal serves nothing
        assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, O, size, 256, 20, 10, 2, 1, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, O, size, 256, 90, 20, 10, S, F, 2, 1, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        assert amd.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, O, size, 256, 20, 10, O, 2, 1, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
    for name, w, h in (("B.MLV", 34, 40), ("C.MLV", 40, 34), ("D.MLV", 38, 40)):           # the linear filter takes them, AMaZE does not
        with mlvfile.MlvReader(clips(name, w, h)) as r, Mount(r, MlvfsOptions()) as m:
            size = 256 + 20 * 30 * 3
            assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 20, 30) == size
            m.set_resample_demosaic("amaze")
            assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 20, 30) == 0 and b"36x36" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, 20, 30) == 0
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(size=(20, 30), resample=True)
            out = np.full(size, 0xA5, np.uint8)
            assert amd.mlvfs_amd_mount_rgb_resampled(m.h, 0, 1, lib.ptr(out), size, 256, 20, 30, 1, 1, None) == lib.ERR_ARG and b"36x36" in amd.mlvfs_amd_last_error()
            assert (out == 0xA5).all() and m.rgb_size(full=True) == 256 + w * h * 3
            m.set_resample_demosaic("linear")
            assert amd.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 20, 30) == size


def test_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert hasattr(Mount, "set_resample_demosaic")


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/amaze_resample_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and
    run directly: the plan writes exactly eight ints, the arithmetic overflows nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    geoms, plans = tmp_path / "geom.bin", tmp_path / "plan.bin"
    records = geom_cases()
    with open(geoms, "wb") as f:
        for rec in records:
            f.write(struct.pack("<5i", *rec))
    cases = plan_cases()
    bad = [(34, 36, 1, 1, 1), (48, 36, 48, 36, 0), (48, 36, 49, 36, 1), (1 << 13, 1 << 12, 1, 1, 1)]
    with open(plans, "wb") as f:
        for w, h, ow, oh, n in cases:
            f.write(struct.pack("<14i", w, h, ow, oh, n, 0, *plan_restated(w, h, ow, oh, n)))
        for w, h, ow, oh, n in bad:
            f.write(struct.pack("<14i", w, h, ow, oh, n, lib.ERR_ARG, *([-7] * 8)))
    exe = tmp_path / "amaze_resample_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "amaze_resample_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(geoms), str(plans)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"amaze_resample_host_check: {len(records)} records, {len(cases) + len(bad)} plans" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
