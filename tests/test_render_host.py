"""Rendered half-size sRGB frames, the library's host code (no GPU): mlvfs_amd_rgb_params against the Python-integer definition of
mlvfs_amd/render.py with the neutral and ForwardMatrix2 parsed from the bytes dng_get_header_data writes for the same headers, the
table, the TIFF header through PIL, every refusal of the host and device entry points (before any device work), the export table and
the Python binding -- and the parameter and header code once more through a stand-alone C++ program (tests/render_host_check.cpp)
built with -fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).
The GPU side: tests/test_gpu_render.py."""
import ctypes as C
import inspect
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import abi, lib, mlvfile, render, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import render_cases as rc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
RGB_SYMBOLS = ["mlvfs_amd_rgb_geom", "mlvfs_amd_rgb_header_size", "mlvfs_amd_rgb_lut", "mlvfs_amd_rgb_params", "mlvfs_amd_rgb_header",
               "mlvfs_amd_render2_dev", "mlvfs_amd_mount_rgb", "mlvfs_amd_mount_rgb_size"]
GAINS = (1, 256, 1024, 65535)


def lib_params(amd, fh, gain_q8):
    out = abi.RgbParams(*([-7] * 13))
    rc_ = amd.mlvfs_amd_rgb_params(C.byref(fh), gain_q8, out)
    return rc_, list(out)


def dng_header(amd, fh, fps, base):
    """the 65536 bytes dng_get_header_data writes for a copy of these headers"""
    copy = abi.FrameHeaders.from_buffer_copy(bytes(fh))
    out = np.zeros(65536, np.uint8)
    assert amd.dng_get_header_data(C.byref(copy), lib.ptr(out), 0, 65536, float(fps), base) == 65536
    return out.tobytes()


def param_cases():
    """[(label, FrameHeaders, fps, basename)]: every camera row and every white-balance mode of the header generator (30 cases walk
    both cycles), the x4 levels of a converted frame, white below black, a zero and a negative numerator, the cap on A"""
    out = [(f"generator {k}", *synth.header_case(k)) for k in range(30)]

    def case(label, k, levels=None, gains=None, mode=6):
        fh, fps, base = synth.header_case(k)
        if levels:
            fh.rawi_hdr.raw_info.black_level, fh.rawi_hdr.raw_info.white_level = levels
        if gains:
            fh.wbal_hdr.wb_mode = mode
            fh.wbal_hdr.wbgain_r, fh.wbal_hdr.wbgain_g, fh.wbal_hdr.wbgain_b = gains
        out.append((label, fh, fps, base))

    case("x4 levels", 3, levels=(8192, 60000))
    case("x4 levels of 16 bits", 4, levels=(32000, 260000))
    case("white below black", 5, levels=(4000, 3000))
    case("white = black", 5, levels=(2048, 2048))
    case("a negative black", 7, levels=(-100, 16000))
    case("a zero red numerator", 6, gains=(0, 1024, 700))
    case("a zero green: numerator and every denominator", 8, gains=(500, 0, 700))
    case("a negative blue numerator", 9, gains=(500, 1024, 0x80000001))
    case("the cap on A: range 1, a large denominator over a small numerator", 10, levels=(2048, 2049), gains=(1, 0x7FFFFFFF, 3))
    case("A near the cap", 11, levels=(2048, 2050), gains=(7, 1000, 1))
    return out


def test_rgb_params_equal_the_python_integers(amd):
    modes, cameras, capped, fallback = set(), set(), 0, 0
    for label, fh, fps, base in param_cases():
        header = dng_header(amd, fh, fps, base)
        black, white, neutral, fm = render.header_colour(header)
        ri = fh.rawi_hdr.raw_info
        assert (black, white) == (ri.black_level, ri.white_level), label
        modes.add(int(fh.wbal_hdr.wb_mode))
        cameras.add(tuple(fm))
        fallback += any(v <= 0 for v in neutral)
        before = bytes(fh)
        for gain in GAINS:
            want = render.params(black, white, neutral, fm, gain)
            rc_, got = lib_params(amd, fh, gain)
            assert rc_ == 0 and got == want, (label, gain, got, want)
            capped += want[1:4].count(render.A_MAX)
        assert bytes(fh) == before, "rgb_params changed the headers"
    assert modes >= {0, 1, 2, 3, 4, 5, 6, 8, 9} and len(cameras) >= 8 and capped >= 4 and fallback >= 3


def test_rgb_params_by_hand():
    """one set worked out on paper: range 12952, unit neutral, unity gain: A = round(65535 * 4096 / 12952)"""
    p = render.params(2048, 15000, (1, 1) * 3, rc.FORWARD[0], 256)
    assert p[:4] == [2048] + [(2 * 65535 * 4096 + 12952) // (2 * 12952)] * 3 == [2048, 20725, 20725, 20725]
    # K[0][0] = round(4096 * (3.1338561 * 0.7637 - 1.6168667 * 0.2649 - 0.4906146 * 0.0137))
    assert p[4] == 8021 and abs(p[4] - 4096 * (3.1338561 * 0.7637 - 1.6168667 * 0.2649 - 0.4906146 * 0.0137)) <= 0.5
    # the rows of K sum to 4096 within rounding where the forward matrix's rows sum to D50 white
    assert all(abs(sum(p[4 + 3 * i:7 + 3 * i]) - 4096) <= 8 for i in range(3))
    # floor towards -inf: a negative entry is rounded, not truncated
    exact = [sum(render.S[i][k] * rc.FORWARD[0][3 * k + j] for k in range(3)) * 4096 / 1e11 for i in range(3) for j in range(3)]
    assert all(abs(k - e) <= 0.5 for k, e in zip(p[4:], exact)) and any(k < 0 for k in p[4:])


def test_rgb_params_refusals(amd):
    fh, _, _ = synth.header_case(0)
    for gain in (0, -1, 65536, 1 << 20):
        rc_, got = lib_params(amd, fh, gain)
        assert rc_ == lib.ERR_ARG and got == [-7] * 13 and b"gain" in amd.mlvfs_amd_last_error(), gain
    out = abi.RgbParams(*([-7] * 13))
    assert amd.mlvfs_amd_rgb_params(None, 256, out) == lib.ERR_ARG and list(out) == [-7] * 13
    assert amd.mlvfs_amd_rgb_params(C.byref(fh), 256, None) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error()


def test_rgb_lut_is_the_golden_file(amd):
    out = np.full(4096 + 8, 0xA5, np.uint8)
    assert amd.mlvfs_amd_rgb_lut(lib.ptr(out)) == 0 and (out[4096:] == 0xA5).all()
    assert out[:4096].tobytes() == open(os.path.join(ROOT, "tests", "golden", "srgb_lut12.bin"), "rb").read()
    assert amd.mlvfs_amd_rgb_lut(None) == lib.ERR_ARG


def geom(amd, w, h):
    pw, ph = C.c_int(-7), C.c_int(-7)
    return amd.mlvfs_amd_rgb_geom(w, h, C.byref(pw), C.byref(ph)), pw.value, ph.value


def test_rgb_geom(amd):
    for w, h in rc.SIZES + rc.MOUNT_SIZES + [(rc.BIG_W, rc.BIG_H), (3, 2), (2, 3), (8191, 16383)]:
        assert geom(amd, w, h) == (0,) + render.geom(w, h), (w, h)
    for w, h in ((1, 4), (4, 1), (0, 0), (-4, 8), (8, -4), (1 << 14, 1 << 13), (1 << 27, 2)):
        assert geom(amd, w, h) == (lib.ERR_ARG, -7, -7) and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    one = C.c_int(5)
    assert amd.mlvfs_amd_rgb_geom(16, 16, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_rgb_geom(16, 16, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def lib_header(amd, pw, ph, cap=None):
    size = amd.mlvfs_amd_rgb_header_size()
    cap = size if cap is None else cap
    out = np.full(max(cap, 1) + 8, 0xA5, np.uint8)
    n = amd.mlvfs_amd_rgb_header(pw, ph, lib.ptr(out), cap)
    assert (out[cap:] == 0xA5).all(), "wrote past cap"
    return n, out[:cap]


def test_rgb_header_is_a_tiff_pil_reads(amd):
    from PIL import Image
    size = amd.mlvfs_amd_rgb_header_size()
    assert size == render.HEADER_BYTES and size % 16 == 0
    for pw, ph in ((1, 1), (3, 2), (32, 24), (209, 133), (1792, 660)):
        n, hdr = lib_header(amd, pw, ph)
        assert n == size and hdr.tobytes() == render.tiff_header(pw, ph), (pw, ph)
        pixels = np.random.default_rng(pw).integers(0, 256, (ph, pw, 3), dtype=np.uint8)
        with Image.open(io.BytesIO(hdr.tobytes() + pixels.tobytes())) as im:
            assert im.format == "TIFF" and im.mode == "RGB" and im.size == (pw, ph)
            t = dict(im.tag_v2)                                       # (loading the pixels consumes Orientation)
            assert np.array_equal(np.asarray(im), pixels), (pw, ph)
            assert (t[256], t[257], t[258], t[259], t[262], t[273], t[274], t[277], t[278], t[279], t[284], t[305]) == \
                (pw, ph, (8, 8, 8), 1, 2, (size,), 1, 3, ph, (3 * pw * ph,), 1, "MLVFS")
            assert sorted(t.keys()) == [256, 257, 258, 259, 262, 273, 274, 277, 278, 279, 284, 305]
    n, hdr = lib_header(amd, 4, 4, cap=size + 100)                    # more room: the header's size, nothing behind it
    assert n == size and (hdr[size:] == 0xA5).all()
    for pw, ph, cap in ((0, 4, size), (4, 0, size), (-1, 4, size), (1 << 13, 1 << 12, size), (4, 4, size - 1), (4, 4, 0)):
        n, hdr = lib_header(amd, pw, ph, cap)
        assert n == 0 and (hdr == 0xA5).all(), (pw, ph, cap)
    assert amd.mlvfs_amd_rgb_header(4, 4, None, size) == 0 and b"null" in amd.mlvfs_amd_last_error()


def test_render2_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    src, dst, par = np.full(4096, 7, np.uint16), np.full(8192, 9, np.uint8), np.zeros(64, np.int32)
    s, d, p = src.ctypes.data, dst.ctypes.data, par.ctypes.data
    vp = lambda a: C.c_void_p(a) if a else None
    r2 = lambda sp, st, w, h, pp, dp, ost, n: amd.mlvfs_amd_render2_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    for args in ((0, 512, 16, 16, p, d, 192, 1), (s, 512, 16, 16, 0, d, 192, 1), (s, 512, 16, 16, p, 0, 192, 1)):
        assert r2(*args) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error(), args
    for w, h in ((1, 16), (16, 1), (0, 16), (16, -1), (1 << 14, 1 << 13)):
        assert r2(s, 512, w, h, p, d, 192, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    assert r2(s, 512, 16, 16, p, d, 192, -1) == lib.ERR_ARG
    assert r2(s, 510, 16, 16, p, d, 192, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a frame
    assert r2(s, 512, 16, 16, p, d, 191, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a rendering
    assert r2(s, 513, 16, 16, p, d, 192, 2) == lib.ERR_ARG                                                   # an odd source stride
    assert r2(s + 1, 512, 16, 16, p, d, 192, 1) == lib.ERR_ARG and r2(s, 512, 16, 16, p + 2, d, 192, 1) == lib.ERR_ARG
    # overlap: in place, the destination inside the source, either end reaching the other, the destination on the parameters
    for dp, n in ((s, 1), (s + 256, 1), (s + 511, 1), (s + 1024 + 511, 3), (s - 191, 1), (s - 192 - 2 * 256 + 1, 3)):
        assert r2(s + 2048, 512, 16, 16, p, dp + 2048, 256, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - s, n)
    for dp, n in ((p, 1), (p + 51, 1), (p - 191, 1), (p + 2 * 52 + 51, 3)):
        assert r2(s, 512, 16, 16, p, dp, 192, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - p, n)
    assert r2(s, 512, 16, 16, p, d, 192, 0) == 0                                 # nothing to do
    assert (src == 7).all() and (dst == 9).all() and not par.any()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_rgb_refusals_and_sizes_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r:
        with Mount(r, MlvfsOptions()) as m:
            size = 256 + 32 * 24 * 3
            assert m.rgb_size() == m.rgb_size(1) == size == amd.mlvfs_amd_mount_rgb_size(m.h, 0)
            assert amd.mlvfs_amd_mount_rgb_size(m.h, 2) == 0 and amd.mlvfs_amd_mount_rgb_size(m.h, -1) == 0
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb_size(2)
            out = np.full(2 * size, 0xA5, np.uint8)
            rgb = lambda h, first, count, o, stride, gain: amd.mlvfs_amd_mount_rgb(h, first, count, o, stride, gain, 2, 1, None)
            # a file smaller than a .dng header is a stride like any other: one byte less than the file is refused
            assert rgb(m.h, 0, 2, lib.ptr(out), size - 1, 256) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
            for gain in (0, -256, 65536):
                assert rgb(m.h, 0, 2, lib.ptr(out), size, gain) == lib.ERR_ARG and b"gain" in amd.mlvfs_amd_last_error(), gain
            assert rgb(m.h, 0, 3, lib.ptr(out), size, 256) == lib.ERR_ARG and rgb(m.h, -1, 1, lib.ptr(out), size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 2, None, size, 256) == lib.ERR_ARG and rgb(None, 0, 2, lib.ptr(out), size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, -1, lib.ptr(out), size, 256) == lib.ERR_ARG
            assert rgb(m.h, 0, 0, lib.ptr(out), size, 256) == 0                  # nothing to do
            for gain in (0.0, -1.0, 256.0, 1 / 1024):
                with pytest.raises(ValueError):
                    m.rgb(0, 2, gain=gain)
            m.set_proxy(2)                                                       # nothing was served: a refusal serves nothing
            assert rgb(m.h, 0, 2, lib.ptr(out), size, 256) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb(0, 2)
            assert m.rgb_size() == size                                          # the size of a rendering does not depend on it
            assert (out == 0xA5).all()
    assert amd.mlvfs_amd_mount_rgb_size(None, 0) == 0
    with mlvfile.MlvReader(clips("B.MLV", 16, 1)) as r, Mount(r, MlvfsOptions()) as m:       # a frame below 2x2
        assert amd.mlvfs_amd_mount_rgb_size(m.h, 0) == 0 and b"2x2" in amd.mlvfs_amd_last_error()
        out = np.full(4096, 0xA5, np.uint8)
        assert amd.mlvfs_amd_mount_rgb(m.h, 0, 1, lib.ptr(out), 4096, 256, 1, 1, None) == lib.ERR_ARG and (out == 0xA5).all()
    with mlvfile.MlvReader(clips("C.MLV", 418, 267)) as r, Mount(r, MlvfsOptions()) as m:
        assert m.rgb_size() == 256 + 209 * 133 * 3


def test_rgb_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in RGB_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    p = inspect.signature(Mount.rgb).parameters
    assert list(p)[1:4] == ["first", "count", "gain"] and p["gain"].default == 1.0
    assert C.sizeof(abi.RgbParams) == 52


def test_the_same_through_a_sanitized_stand_alone_program(amd, tmp_path):
    """tests/render_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: mlvfs_amd_rgb_params writes exactly 13 integers and mlvfs_amd_rgb_header exactly its size (the program's buffers are
    that long and no longer), the 128-bit arithmetic overflows nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    records = 0
    with open(cases, "wb") as f:
        for label, fh, fps, base in param_cases():
            colour = render.header_colour(dng_header(amd, fh, fps, base))
            for gain in GAINS:
                blob = bytes(fh)
                f.write(struct.pack("<IIi", 1, len(blob), gain) + blob + struct.pack("<13i", *render.params(*colour, gain)))
                records += 1
        for pw, ph in ((1, 1), (32, 24), (209, 133), (1792, 660)):
            f.write(struct.pack("<IIi", 2, pw, ph) + render.tiff_header(pw, ph))
            records += 1
    exe = tmp_path / "render_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "render_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"render_host_check: {records} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
