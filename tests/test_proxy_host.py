"""Half-size Bayer proxies, the library's host code (no GPU): mlvfs_amd_proxy_geom, every refusal of the host and device entry points
(before any device work), mlvfs_amd_dng_header_proxy against the reference's dng_get_header_data on the same frame_headers with the
header rule of tests/proxy_cases.py applied, the export table and the Python binding -- and the same header cases once more through
a stand-alone C++ program (tests/proxy_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of the
host code (`make hostcheck`, built here if it is not yet).  The GPU side: tests/test_gpu_proxy.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import abi, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import proxy_cases as pc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
PROXY_SYMBOLS = ["mlvfs_amd_proxy_geom", "mlvfs_amd_bin2_dev", "mlvfs_amd_dng_header_proxy", "mlvfs_amd_mount_set_proxy",
                 "mlvfs_amd_mount_dng_size"]


def geom(amd, w, h, factor=2):
    pw, ph = C.c_int(-7), C.c_int(-7)
    rc = amd.mlvfs_amd_proxy_geom(w, h, factor, C.byref(pw), C.byref(ph))
    return rc, pw.value, ph.value


def test_proxy_geom(amd):
    for w, h in pc.BIN_SIZES + [(pc.BIG_W, pc.BIG_H), (pc.DROP_W, pc.DROP_H), (5, 4), (8191, 16383), (1 << 13, (1 << 14) - 1)]:
        assert geom(amd, w, h) == (0,) + pc.proxy_size(w, h), (w, h)
    for w, h in ((3, 4), (4, 3), (0, 0), (-4, 8), (8, -4), (1 << 14, 1 << 13), (1 << 27, 4)):
        assert geom(amd, w, h) == (lib.ERR_ARG, -7, -7) and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    for factor in (0, 1, 3, 4, -2):
        assert geom(amd, 16, 16, factor) == (lib.ERR_ARG, -7, -7) and b"factor" in amd.mlvfs_amd_last_error(), factor
    one = C.c_int(5)
    assert amd.mlvfs_amd_proxy_geom(16, 16, 2, None, C.byref(one)) == lib.ERR_ARG and one.value == 5
    assert amd.mlvfs_amd_proxy_geom(16, 16, 2, C.byref(one), None) == lib.ERR_ARG and one.value == 5


def test_bin2_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    src, dst = np.full(4096, 7, np.uint16), np.full(4096, 9, np.uint16)
    s, d = src.ctypes.data, dst.ctypes.data
    bin2 = lambda sp, st, w, h, dp, ost, n: amd.mlvfs_amd_bin2_dev(C.c_void_p(sp) if sp else None, st, w, h, C.c_void_p(dp) if dp else None, ost, n, None)
    assert bin2(0, 512, 16, 16, d, 128, 1) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error()
    assert bin2(s, 512, 16, 16, 0, 128, 1) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error()
    for w, h in ((3, 16), (16, 3), (0, 16), (16, -1), (1 << 14, 1 << 13)):
        assert bin2(s, 512, w, h, d, 128, 1) == lib.ERR_ARG and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    assert bin2(s, 512, 16, 16, d, 128, -1) == lib.ERR_ARG
    assert bin2(s, 510, 16, 16, d, 128, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a frame
    assert bin2(s, 512, 16, 16, d, 126, 2) == lib.ERR_ARG and b"stride" in amd.mlvfs_amd_last_error()      # smaller than a proxy frame
    assert bin2(s, 513, 16, 16, d, 128, 2) == lib.ERR_ARG and bin2(s, 512, 16, 16, d, 129, 2) == lib.ERR_ARG
    assert bin2(s + 1, 512, 16, 16, d, 128, 1) == lib.ERR_ARG and bin2(s, 512, 16, 16, d + 1, 128, 1) == lib.ERR_ARG
    # overlap: in place, the destination inside the source, the source's last frame reaching the destination, and the reverse
    for dp, n in ((s, 1), (s + 256, 1), (s + 510, 1), (s + 1024 + 510, 3), (s - 126, 1), (s - 128 - 2 * 256 + 2, 3)):
        st, ost = 512, 256
        assert bin2(s + 2048, st, 16, 16, dp + 2048, ost, n) == lib.ERR_ARG and b"overlap" in amd.mlvfs_amd_last_error(), (dp - s, n)
    assert bin2(s, 512, 16, 16, d, 128, 0) == 0                                # nothing to do
    assert (src == 7).all() and (dst == 9).all()


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_refusals_and_sizes_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r:
        with Mount(r, MlvfsOptions()) as m:
            full = 65536 + 64 * 48 * 2
            assert m.dng_size() == m.dng_size(1) == full == amd.mlvfs_amd_mount_dng_size(m.h, 0)
            for factor in (0, 3, -1, 4):
                assert amd.mlvfs_amd_mount_set_proxy(m.h, factor) == lib.ERR_ARG and b"factor" in amd.mlvfs_amd_last_error(), factor
                with pytest.raises(lib.MlvfsAmdError):
                    m.set_proxy(factor)
            assert m.proxy == 1 and m.dng_size() == full
            m.set_proxy(2)
            small = 65536 + 32 * 24 * 2
            assert m.proxy == 2 and m.dng_size() == m.dng_size(1) == small
            assert amd.mlvfs_amd_mount_dng_size(m.h, 2) == 0 and amd.mlvfs_amd_mount_dng_size(m.h, -1) == 0
            with pytest.raises(lib.MlvfsAmdError):
                m.dng_size(2)
            # an out_stride smaller than the PROXY file is refused, by both calls, before any device work
            out = np.full(2 * small, 0xA5, np.uint8)
            sizes, flags = np.zeros(2, np.uintp), np.zeros(2, np.int32)
            assert amd.mlvfs_amd_mount_dng(m.h, 0, 2, lib.ptr(out), small - 1, 2, 1, None) == lib.ERR_ARG
            assert b"out_stride" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_dng_lossless(m.h, 0, 2, lib.ptr(out), small - 1, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG
            assert (out == 0xA5).all()
            m.set_proxy(1)                                                   # nothing was served: it can still change
            assert m.dng_size() == full
            assert amd.mlvfs_amd_mount_dng(m.h, 0, 2, lib.ptr(out), full - 1, 2, 1, None) == lib.ERR_ARG and (out == 0xA5).all()
        with Mount(r, MlvfsOptions(), proxy=2) as m:
            assert m.proxy == 2 and m.dng_size() == 65536 + 32 * 24 * 2
        with pytest.raises(lib.MlvfsAmdError):
            Mount(r, MlvfsOptions(), proxy=3)
    assert amd.mlvfs_amd_mount_set_proxy(None, 2) == lib.ERR_ARG and amd.mlvfs_amd_mount_dng_size(None, 0) == 0
    with mlvfile.MlvReader(clips("B.MLV", 16, 2)) as r:                        # a first frame smaller than 4x4
        with Mount(r, MlvfsOptions()) as m:
            assert amd.mlvfs_amd_mount_set_proxy(m.h, 2) == lib.ERR_ARG and b"4x4" in amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_set_proxy(m.h, 1) == 0 and m.dng_size() == 65536 + 16 * 2 * 2
        with pytest.raises(lib.MlvfsAmdError):
            Mount(r, MlvfsOptions(), proxy=2)
    with mlvfile.MlvReader(clips("C.MLV", pc.DROP_W, pc.DROP_H)) as r, Mount(r, MlvfsOptions(), proxy=2) as m:
        assert m.dng_size() == 65536 + 208 * 132 * 2


def proxy_header(amd, blob, fps, base, offset=0, max_size=65536, stream=0, factor=2):
    fh = abi.FrameHeaders.from_buffer_copy(bytes(bytearray(blob)))
    out = np.full(max(max_size, 1) + 8, 0xA5, np.uint8)                     # 8 guard bytes behind the request
    n = amd.mlvfs_amd_dng_header_proxy(C.byref(fh), lib.ptr(out), offset, max_size, float(fps), base, factor, stream)
    assert (out[max_size:] == 0xA5).all(), "wrote past max_size"
    return n, out[:max_size], np.frombuffer(bytes(fh), np.uint8)


def check_case(amd, full_of, label, fh, fps, base):
    """full_of(blob, fps, base) -> (n, the full-size header, frame_headers after)"""
    blob = np.frombuffer(bytes(fh), np.uint8)
    n0, full, after0 = full_of(blob, fps, base)
    assert n0 == 65536
    for stream in (0, 1, 123457, 0xFFFFFFFF):
        want = pc.proxy_header(full, fh, stream)
        n1, got, after1 = proxy_header(amd, blob, fps, base, stream=stream)
        assert n1 == 65536 and np.array_equal(after0, after1), (label, stream)              # the same active-area rewrite
        if got.tobytes() != want:
            bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
            raise AssertionError(f"{label}, stream {stream}: {bad.size} bytes differ, first at {bad[0]}")
        # every byte outside the listed tags' value fields equals the full-size header's
        mask = np.ones(65536, bool)
        assert set(pc.proxy_tags(pc.header_tags(full), full, fh, stream)) - {259} == set(pc.PROXY_TAGS)
        for at, val in pc.proxy_tags(pc.header_tags(full), full, fh, stream).values():
            mask[at:at + len(val)] = False
        assert np.array_equal(got[mask], np.asarray(full)[mask]), label
        t, f = pc.header_tags(got), pc.header_tags(full)
        assert t.keys() == f.keys() and all(t[k][:2] == f[k][:2] and t[k][3] == f[k][3] for k in t)
        # DefaultScale and the focal-plane numerators: the full-size frame's
        a, b = t[50718][2], f[50718][2]
        assert a == b and got[a:a + 16].tobytes() == bytes(full[b:b + 16])
    want = pc.proxy_header(full, fh, 0)
    for offset, size in pc.WINDOWS:
        n1, got, _ = proxy_header(amd, blob, fps, base, offset, size)
        assert n1 == min(size, 65536), (label, offset, size)
        have = want[offset:offset + n1]
        assert got[:n1].tobytes() == have + bytes(n1 - len(have)), (label, offset, size)
    return want


def test_header_equals_the_reference_header_with_the_rule_applied(amd, reference):
    cases = pc.header_cases()
    for label, fh, fps, base in cases:
        check_case(amd, lambda blob, fps, base: reference.header_data(blob, 0, 65536, fps, base), label, fh, fps, base)
    # what the cases pin: a 5:3 frame keeps DefaultScale 1/1, 5/3 and the x3 / x5 denominators, doubled
    label, fh, fps, base = next(c for c in cases if c[0] == "5:3")
    want = pc.proxy_header(reference.header_data(np.frombuffer(bytes(fh), np.uint8), 0, 65536, fps, base)[1], fh)
    t = pc.header_tags(want)
    assert struct.unpack_from("<4i", want, t[50718][2]) == (1, 1, 5, 3)
    label, fh, fps, base = next(c for c in cases if c[0] == "below 2000 columns")
    full = reference.header_data(np.frombuffer(bytes(fh), np.uint8), 0, 65536, fps, base)[1]
    t, f = pc.header_tags(pc.proxy_header(full, fh)), pc.header_tags(full)
    for tag in (41486, 41487):
        (n1, d1), (n0, d0) = struct.unpack_from("<2i", pc.proxy_header(full, fh), t[tag][2]), struct.unpack_from("<2i", bytes(full), f[tag][2])
        assert n1 == n0 and d1 == 2 * d0 and d0 % 3 == 0


def test_header_equals_the_librarys_own_header_with_the_rule_applied(amd):
    """the same without the reference build: against dng_get_header_data of this library (tests/test_header.py holds that one to the
    reference's vectors)"""
    def full_of(blob, fps, base):
        fh = abi.FrameHeaders.from_buffer_copy(bytes(bytearray(blob)))
        out = np.zeros(65536, np.uint8)
        n = amd.dng_get_header_data(C.byref(fh), lib.ptr(out), 0, 65536, float(fps), base)
        return n, out, np.frombuffer(bytes(fh), np.uint8)
    for label, fh, fps, base in pc.header_cases():
        check_case(amd, full_of, label, fh, fps, base)


def test_header_refusals(amd):
    fh, fps, base = synth.header_case(3)
    blob = np.frombuffer(bytes(fh), np.uint8)
    for factor in (0, 1, 3, -2):
        n, got, after = proxy_header(amd, blob, fps, base, factor=factor)
        assert n == 0 and (got == 0xA5).all() and np.array_equal(after, blob) and b"factor" in amd.mlvfs_amd_last_error(), factor
    out = np.full(65536, 0xA5, np.uint8)
    assert amd.mlvfs_amd_dng_header_proxy(None, lib.ptr(out), 0, 65536, 0.0, base, 2, 0) == 0 and b"null" in amd.mlvfs_amd_last_error()
    assert amd.mlvfs_amd_dng_header_proxy(C.byref(fh), None, 0, 65536, 0.0, base, 2, 0) == 0 and (out == 0xA5).all()
    for size in ((3, 100), (100, 3), (0, 0)):
        small, _, _ = synth.header_case(3)
        small.rawi_hdr.xRes, small.rawi_hdr.yRes = size
        n, got, _ = proxy_header(amd, np.frombuffer(bytes(small), np.uint8), fps, base)
        assert n == 0 and (got == 0xA5).all(), size


def test_proxy_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in PROXY_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert inspect.signature(Mount.__init__).parameters["proxy"].default == 1 and hasattr(Mount, "set_proxy")


def test_the_same_headers_through_a_sanitized_stand_alone_program(amd, tmp_path):
    """tests/proxy_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: mlvfs_amd_dng_header_proxy writes exactly min(max_size, 65536) bytes (the program's buffers are that long and no
    longer) and mlvfs_amd_proxy_geom and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    records = 0
    with open(cases, "wb") as f:
        for label, fh, fps, base in pc.header_cases():
            blob = bytes(fh)
            full_fh = abi.FrameHeaders.from_buffer_copy(blob)
            full = np.zeros(65536, np.uint8)
            assert amd.dng_get_header_data(C.byref(full_fh), lib.ptr(full), 0, 65536, float(fps), base) == 65536
            for stream in (0, 123457):
                want = pc.proxy_header(full, fh, stream)
                for offset, size in pc.WINDOWS:
                    n = min(size, 65536)
                    have = want[offset:offset + n]
                    f.write(struct.pack("<IdqQIII", len(blob), float(fps), offset, size, stream, len(base), n))
                    f.write(blob + base + have + bytes(n - len(have)) + bytes(full_fh))
                    records += 1
    exe = tmp_path / "proxy_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "proxy_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"proxy_host_check: {records} headers" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
