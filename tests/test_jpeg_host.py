"""Rendered frames as baseline JPEG files, the library's host code (no GPU): mlvfs_amd_jpeg_header and mlvfs_amd_jpeg_qtables against the
definition of mlvfs_amd/jpeg.py for every quality and several sizes, the scratch size, every refusal of the host and device entry
points (before any device work), the export table and the Python binding -- and the same host code once more through a stand-alone C++
program (tests/jpeg_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of the host code
(`make hostcheck`, built here if it is not yet).  The GPU side: tests/test_gpu_jpeg.py."""
import ctypes as C
import inspect
import io
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
JPEG_SYMBOLS = ["mlvfs_amd_jpeg_header_size", "mlvfs_amd_jpeg_header", "mlvfs_amd_jpeg_qtables", "mlvfs_amd_jpeg_scratch_bytes",
                "mlvfs_amd_jpeg_encode_dev", "mlvfs_amd_mount_jpeg"]
SIZES = ((1, 1), (17, 17), (32, 24), (209, 133), (1792, 660), (65535, 1), (1, 65535))
PAD = 0xA5


def lib_header(amd, pw, ph, quality, cap=None):
    size = amd.mlvfs_amd_jpeg_header_size()
    cap = size if cap is None else cap
    out = np.full(max(cap, 1) + 8, PAD, np.uint8)
    n = amd.mlvfs_amd_jpeg_header(pw, ph, quality, lib.ptr(out), cap)
    assert (out[cap:] == PAD).all(), "wrote past cap"
    return n, out[:cap]


def test_header_is_the_definitions_for_every_quality(amd):
    size = amd.mlvfs_amd_jpeg_header_size()
    assert size == jpeg.HEADER_BYTES == 629
    for q in range(1, 101):
        for pw, ph in SIZES if q in (1, 50, 90, 100) else SIZES[2:3]:
            n, hdr = lib_header(amd, pw, ph, q)
            assert n == size and hdr.tobytes() == jpeg.header(pw, ph, q), (pw, ph, q)
    n, hdr = lib_header(amd, 4, 4, 90, cap=size + 100)                # more room: the header's size, nothing behind it
    assert n == size and (hdr[size:] == PAD).all()
    for pw, ph, q, cap in ((0, 4, 90, size), (4, 0, 90, size), (-1, 4, 90, size), (1 << 13, 1 << 12, 90, size), (65536, 1, 90, size),
                           (1, 65536, 90, size), (4, 4, 0, size), (4, 4, 101, size), (4, 4, -5, size), (4, 4, 90, size - 1), (4, 4, 90, 0)):
        n, hdr = lib_header(amd, pw, ph, q, cap)
        assert n == 0 and (hdr == PAD).all(), (pw, ph, q, cap)
    assert amd.mlvfs_amd_jpeg_header(4, 4, 90, None, size) == 0 and b"null" in amd.mlvfs_amd_last_error()


def test_header_and_the_oracles_stream_are_a_file_pil_opens(amd):
    from PIL import Image
    rgb = np.random.default_rng(3).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    n, hdr = lib_header(amd, 47, 33, 85)
    with Image.open(io.BytesIO(hdr.tobytes() + jpeg.encode(rgb, 85))) as im:
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (47, 33)
        im.load()


def test_qtables_are_the_definitions_for_every_quality(amd):
    for q in range(1, 101):
        out = np.full(128 + 8, PAD, np.uint8)
        assert amd.mlvfs_amd_jpeg_qtables(q, lib.ptr(out)) == 0
        assert np.array_equal(out[:128].reshape(2, 64), jpeg.qtables(q)) and (out[128:] == PAD).all(), q
    out = np.full(128, PAD, np.uint8)
    for q in (0, 101, -1):
        assert amd.mlvfs_amd_jpeg_qtables(q, lib.ptr(out)) == lib.ERR_ARG and b"quality" in amd.mlvfs_amd_last_error()
    assert amd.mlvfs_amd_jpeg_qtables(90, None) == lib.ERR_ARG and (out == PAD).all()


def test_scratch_bytes(amd):
    one, eight = amd.mlvfs_amd_jpeg_scratch_bytes(1792, 660, 1), amd.mlvfs_amd_jpeg_scratch_bytes(1792, 660, 8)
    assert one >= 112 * 42 * 768 and 7 * one < eight <= 8 * one                  # the coefficients at least; frames side by side
    assert amd.mlvfs_amd_jpeg_scratch_bytes(1, 1, 1) > 768 and amd.mlvfs_amd_jpeg_scratch_bytes(16, 16, 0) == 0
    for pw, ph, n in ((0, 4, 1), (4, 0, 1), (65536, 1, 1), (1 << 13, 1 << 12, 1), (4, 4, -1)):
        assert amd.mlvfs_amd_jpeg_scratch_bytes(pw, ph, n) == 0 and b"not supported" in amd.mlvfs_amd_last_error(), (pw, ph, n)


def test_encode_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    pw, ph = 16, 16
    need = amd.mlvfs_amd_jpeg_scratch_bytes(pw, ph, 2)
    buf = np.full(8192 + need + 4096 + 256, 7, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    s, d, sc = base, base + 2048, base + 8192
    lengths, status = np.full(2, 7, np.uint32), np.full(2, 7, np.int32)
    L, S = lib.ptr(lengths), lib.ptr(status)
    vp = lambda a: C.c_void_p(a) if a else None
    enc = lambda sp, st, w, h, q, dp, ost, room, scp, scb, lp, stp, n: amd.mlvfs_amd_jpeg_encode_dev(
        vp(sp), st, w, h, q, vp(dp), ost, room, vp(scp), scb, lp, stp, n, None)
    ok = dict(sp=s, st=1024, w=pw, h=ph, q=90, dp=d, ost=1024, room=1024, scp=sc, scb=need, lp=L, stp=S, n=2)
    bad = [(dict(sp=0), b"null"), (dict(dp=0), b"null"), (dict(scp=0), b"null"), (dict(lp=None), b"null"), (dict(stp=None), b"null"),
           (dict(w=0), b"not supported"), (dict(h=0), b"not supported"), (dict(w=65536, h=1), b"not supported"),
           (dict(w=1 << 13, h=1 << 12), b"not supported"), (dict(q=0), b"quality"), (dict(q=101), b"quality"),
           (dict(st=767), b"stride"), (dict(ost=1023), b"stride"), (dict(scb=need - 1), b"scratch"), (dict(scp=sc + 4), b"aligned"),
           (dict(n=-1), b"frames"), (dict(n=65536), b"frames"),
           (dict(dp=s + 1024), b"overlap"), (dict(dp=s - 1024 - 1023), b"overlap"), (dict(scp=d + 1024), b"overlap"),
           (dict(sp=sc + 256), b"overlap"), (dict(dp=sc + need - 16), b"overlap")]
    for change, why in bad:
        assert enc(**dict(ok, **change)) == lib.ERR_ARG and why in amd.mlvfs_amd_last_error(), change
    assert enc(**dict(ok, n=0)) == 0                                             # nothing to do
    assert (buf == 7).all() and list(lengths) == [7, 7] and list(status) == [7, 7]


@pytest.fixture()
def clips(tmp_path):
    def make(name, w, h, n=2):
        frames = [synth.normal_frame(w, h, seed=5, frame=k) for k in range(n)]
        return mlvfile.write_clip(str(tmp_path / name), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)[0]
    return make


def test_mount_jpeg_refusals_on_the_host(amd, clips):
    with mlvfile.MlvReader(clips("A.MLV", 64, 48)) as r, Mount(r, MlvfsOptions()) as m:
        size = m.rgb_size()
        out = np.full(2 * size, PAD, np.uint8)
        sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
        j = lambda h, first, count, o, stride, gain, q, s, f: amd.mlvfs_amd_mount_jpeg(h, first, count, o, stride, gain, q, s, f, 2, 1, None)
        assert j(m.h, 0, 2, O, size - 1, 256, 90, S, F) == lib.ERR_ARG and b"out_stride" in amd.mlvfs_amd_last_error()
        for gain in (0, -256, 65536):
            assert j(m.h, 0, 2, O, size, gain, 90, S, F) == lib.ERR_ARG and b"gain" in amd.mlvfs_amd_last_error(), gain
        for q in (0, -1, 101):
            assert j(m.h, 0, 2, O, size, 256, q, S, F) == lib.ERR_ARG and b"quality" in amd.mlvfs_amd_last_error(), q
        assert j(m.h, 0, 3, O, size, 256, 90, S, F) == lib.ERR_ARG and j(m.h, -1, 1, O, size, 256, 90, S, F) == lib.ERR_ARG
        assert j(m.h, 0, 2, None, size, 256, 90, S, F) == lib.ERR_ARG and j(None, 0, 2, O, size, 256, 90, S, F) == lib.ERR_ARG
        assert j(m.h, 0, 2, O, size, 256, 90, None, F) == lib.ERR_ARG and j(m.h, 0, 2, O, size, 256, 90, S, None) == lib.ERR_ARG
        assert j(m.h, 0, -1, O, size, 256, 90, S, F) == lib.ERR_ARG
        assert j(m.h, 0, 0, O, size, 256, 90, S, F) == 0                         # nothing to do
        for kw in (dict(gain=0.0), dict(gain=256.0), dict(quality=0), dict(quality=101)):
            with pytest.raises(ValueError):
                m.jpeg(0, 2, **kw)
        m.set_proxy(2)                                                           # nothing was served: a refusal serves nothing
        assert j(m.h, 0, 2, O, size, 256, 90, S, F) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
        with pytest.raises(lib.MlvfsAmdError):
            m.jpeg(0, 2)
        assert (out == PAD).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
    with mlvfile.MlvReader(clips("B.MLV", 16, 1)) as r, Mount(r, MlvfsOptions()) as m:       # a frame below 2x2
        out = np.full(4096, PAD, np.uint8)
        assert amd.mlvfs_amd_mount_jpeg(m.h, 0, 1, lib.ptr(out), 4096, 256, 90, S, F, 1, 1, None) == lib.ERR_ARG and (out == PAD).all()


def test_jpeg_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in JPEG_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    p = inspect.signature(Mount.jpeg).parameters
    assert list(p)[1:5] == ["first", "count", "gain", "quality"] and p["gain"].default == 1.0 and p["quality"].default == 90


def test_the_same_through_a_sanitized_stand_alone_program(amd, tmp_path):
    """tests/jpeg_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: mlvfs_amd_jpeg_header writes exactly its size and mlvfs_amd_jpeg_qtables exactly 128 bytes (the program's buffers are
    that long and no longer), the layout arithmetic of the largest input overflows nowhere, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    records = 0
    with open(cases, "wb") as f:
        for q in (1, 25, 49, 50, 75, 90, 100):
            for pw, ph in SIZES:
                f.write(struct.pack("<Iiii", 1, pw, ph, q) + jpeg.header(pw, ph, q))
                records += 1
        for q in range(1, 101):
            f.write(struct.pack("<Iiii", 2, 0, 0, q) + jpeg.qtables(q).tobytes())
            records += 1
    exe = tmp_path / "jpeg_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "jpeg_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"jpeg_host_check: {records} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
