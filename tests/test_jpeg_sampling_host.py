"""The chroma samplings of the rendered JPEG files, the library's host code (no GPU): mlvfs_amd_jpeg_header_sampled and
mlvfs_amd_jpeg_mcus against the definition of mlvfs_amd/jpeg.py, the scratch sizes, every refusal of the host and device entry points
and of the mount's setter (before any device work), the export table and the Python binding -- and the same host code once more through
a stand-alone C++ program (tests/jpeg_sampling_host_check.cpp) built with -fsanitize=address,undefined against the sanitizer build of
the host code (`make hostcheck`, built here if it is not yet).  The GPU side: tests/test_gpu_jpeg_sampling.py."""
import ctypes as C
import inspect
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
SYMBOLS = ["mlvfs_amd_jpeg_header_sampled", "mlvfs_amd_jpeg_scratch_bytes_sampled", "mlvfs_amd_jpeg_mcus", "mlvfs_amd_jpeg_encode_sampled_dev",
           "mlvfs_amd_mount_set_jpeg_sampling"]
SIZES = ((1, 1), (8, 8), (9, 9), (17, 17), (32, 24), (209, 133), (1792, 660), (65535, 1), (1, 65535))
CODES = ((420, 0), (422, 1), (444, 2))
BAD = (-1, 3, 4, 420, 422, 444, -2 ** 31, 2 ** 31 - 1)
PAD = 0xA5


def lib_header(amd, pw, ph, quality, code, cap=None):
    size = amd.mlvfs_amd_jpeg_header_size()
    cap = size if cap is None else cap
    out = np.full(max(cap, 1) + 8, PAD, np.uint8)
    n = amd.mlvfs_amd_jpeg_header_sampled(pw, ph, quality, code, lib.ptr(out), cap)
    assert (out[cap:] == PAD).all(), "wrote past cap"
    return n, out[:cap]


def test_header_is_the_definitions_at_every_sampling(amd):
    size = amd.mlvfs_amd_jpeg_header_size()
    assert size == jpeg.HEADER_BYTES == 629
    for sampling, code in CODES:
        for q in (1, 25, 50, 75, 90, 100):
            for pw, ph in SIZES:
                n, hdr = lib_header(amd, pw, ph, q, code)
                assert n == size and hdr.tobytes() == jpeg.header(pw, ph, q, sampling), (pw, ph, q, sampling)
        n, hdr = lib_header(amd, 4, 4, 90, code, cap=size + 100)              # more room: the header's size, nothing behind it
        assert n == size and (hdr[size:] == PAD).all()
        for pw, ph, q, cap in ((0, 4, 90, size), (4, 0, 90, size), (-1, 4, 90, size), (1 << 13, 1 << 12, 90, size), (65536, 1, 90, size),
                               (1, 65536, 90, size), (4, 4, 0, size), (4, 4, 101, size), (4, 4, -5, size), (4, 4, 90, size - 1), (4, 4, 90, 0)):
            n, hdr = lib_header(amd, pw, ph, q, code, cap)
            assert n == 0 and (hdr == PAD).all(), (pw, ph, q, cap)
        assert amd.mlvfs_amd_jpeg_header_sampled(4, 4, 90, code, None, size) == 0 and b"null" in amd.mlvfs_amd_last_error()
    for bad in BAD:
        n, hdr = lib_header(amd, 16, 16, 90, bad)
        assert n == 0 and (hdr == PAD).all() and b"sampling" in amd.mlvfs_amd_last_error(), bad
    # the call without a sampling is what it was
    out = np.full(size, PAD, np.uint8)
    assert amd.mlvfs_amd_jpeg_header(209, 133, 85, lib.ptr(out), size) == size and out.tobytes() == jpeg.header(209, 133, 85)


def test_header_and_the_definitions_stream_are_a_file_pil_opens(amd):
    import io
    from PIL import Image
    rgb = np.random.default_rng(3).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    for sampling, code in CODES:
        n, hdr = lib_header(amd, 47, 33, 85, code)
        with Image.open(io.BytesIO(hdr.tobytes() + jpeg.encode(rgb, 85, None, sampling))) as im:
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == (47, 33)
            im.load()


def test_mcus(amd):
    for sampling, code in CODES:
        for pw, ph in SIZES + ((16, 16), (4112, 8), (8, 8200), (8191, 4096)):
            mw, mh = C.c_int(-7), C.c_int(-7)
            assert amd.mlvfs_amd_jpeg_mcus(pw, ph, code, C.byref(mw), C.byref(mh)) == 0
            assert (mw.value, mh.value) == jpeg.mcus(pw, ph, sampling), (pw, ph, sampling)
    mw, mh = C.c_int(-7), C.c_int(-7)
    for pw, ph, code in ((0, 4, 2), (4, 0, 1), (65536, 1, 2), (1 << 13, 1 << 12, 0)) + tuple((16, 16, b) for b in BAD):
        assert amd.mlvfs_amd_jpeg_mcus(pw, ph, code, C.byref(mw), C.byref(mh)) == lib.ERR_ARG, (pw, ph, code)
    assert amd.mlvfs_amd_jpeg_mcus(4, 4, 2, None, C.byref(mh)) == lib.ERR_ARG and amd.mlvfs_amd_jpeg_mcus(4, 4, 2, C.byref(mw), None) == lib.ERR_ARG
    assert (mw.value, mh.value) == (-7, -7)


def test_scratch_bytes_per_sampling(amd):
    f = amd.mlvfs_amd_jpeg_scratch_bytes_sampled
    for pw, ph in ((1, 1), (17, 17), (209, 133), (1792, 660)):
        sizes = {}
        for sampling, code in CODES:
            mw, mh = jpeg.mcus(pw, ph, sampling)
            blocks = mw * mh * (jpeg.SAMPLINGS[sampling][2] + 2)
            got = [f(pw, ph, code, n) for n in range(0, 10)]
            assert got[0] == 0 and got[1] >= blocks * 128, (pw, ph, sampling)                # the coefficients at least
            steps = {b - a for a, b in zip(got[1:], got[2:])}
            assert len(steps) == 1 and min(steps) >= blocks * 128, "monotone in the frame count, frames side by side"
            sizes[sampling] = got[8]
        assert sizes[420] == amd.mlvfs_amd_jpeg_scratch_bytes(pw, ph, 8)
        if pw >= 209:                                      # (a single pixel is six blocks at 4:2:0 and three at 4:4:4)
            assert sizes[420] < sizes[422] < sizes[444]
    assert 1.9 * f(1792, 660, 0, 1) < f(1792, 660, 2, 1) < 3 * f(1792, 660, 0, 1)       # twice the coefficient bytes per pixel
    for code in range(3):
        for pw, ph, n in ((0, 4, 1), (4, 0, 1), (65536, 1, 1), (1 << 13, 1 << 12, 1), (4, 4, -1)):
            assert f(pw, ph, code, n) == 0 and b"not supported" in amd.mlvfs_amd_last_error(), (pw, ph, n)
        assert f(65535, 511, code, 65535) > 0 and f(1, 65535, code, 2) > 0
    for bad in BAD:
        assert f(16, 16, bad, 1) == 0 and b"sampling" in amd.mlvfs_amd_last_error(), bad


def test_encode_sampled_dev_refuses_on_the_host(amd):
    """every check happens before any device work: the pointers are never followed (they are host memory here)"""
    pw, ph = 16, 16
    need = amd.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, 2, 2)
    buf = np.full(8192 + need + 4096 + 256, 7, np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    s, d, sc = base, base + 2048, base + 8192
    lengths, status = np.full(2, 7, np.uint32), np.full(2, 7, np.int32)
    L, S = lib.ptr(lengths), lib.ptr(status)
    vp = lambda a: C.c_void_p(a) if a else None
    enc = lambda sp, st, w, h, q, smp, dp, ost, room, scp, scb, lp, stp, n: amd.mlvfs_amd_jpeg_encode_sampled_dev(
        vp(sp), st, w, h, q, smp, vp(dp), ost, room, vp(scp), scb, lp, stp, n, None)
    for smp in range(3):
        exact = amd.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, smp, 2)
        ok = dict(sp=s, st=1024, w=pw, h=ph, q=90, smp=smp, dp=d, ost=1024, room=1024, scp=sc, scb=exact, lp=L, stp=S, n=2)
        bad = [(dict(sp=0), b"null"), (dict(dp=0), b"null"), (dict(scp=0), b"null"), (dict(lp=None), b"null"), (dict(stp=None), b"null"),
               (dict(w=0), b"not supported"), (dict(h=0), b"not supported"), (dict(w=65536, h=1), b"not supported"),
               (dict(w=1 << 13, h=1 << 12), b"not supported"), (dict(q=0), b"quality"), (dict(q=101), b"quality"),
               (dict(st=767), b"stride"), (dict(ost=1023), b"stride"), (dict(scb=exact - 1), b"scratch"), (dict(scp=sc + 4), b"aligned"),
               (dict(n=-1), b"frames"), (dict(n=65536), b"frames"),
               (dict(dp=s + 1024), b"overlap"), (dict(dp=s - 1024 - 1023), b"overlap"), (dict(scp=d + 1024), b"overlap"),
               (dict(sp=sc + 256), b"overlap"), (dict(dp=sc + exact - 16), b"overlap")]
        bad += [(dict(smp=b), b"sampling") for b in BAD]
        for change, why in bad:
            assert enc(**dict(ok, **change)) == lib.ERR_ARG and why in amd.mlvfs_amd_last_error(), (smp, change)
        assert enc(**dict(ok, n=0)) == 0                                         # nothing to do
    assert (buf == 7).all() and list(lengths) == [7, 7] and list(status) == [7, 7]


def test_mount_set_jpeg_sampling_on_the_host(amd, tmp_path):
    frames = [synth.normal_frame(64, 48, seed=5, frame=k) for k in range(2)]
    path = mlvfile.write_clip(str(tmp_path / "A.MLV"), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], 64, 48)[0]
    assert amd.mlvfs_amd_mount_set_jpeg_sampling(None, 0) == lib.ERR_ARG and b"null" in amd.mlvfs_amd_last_error()
    with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions()) as m:
        assert m.jpeg_sampling == "4:2:0"
        for bad in BAD:
            assert amd.mlvfs_amd_mount_set_jpeg_sampling(m.h, bad) == lib.ERR_ARG and b"sampling" in amd.mlvfs_amd_last_error(), bad
        for name, code in Mount.SAMPLINGS.items():
            assert amd.mlvfs_amd_mount_set_jpeg_sampling(m.h, code) == 0
            m.set_jpeg_sampling(name)
            assert m.jpeg_sampling == name
        assert Mount.SAMPLINGS == {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}
        for bad in ("444", "4:1:1", 444, None):
            with pytest.raises(ValueError):
                m.set_jpeg_sampling(bad)
        with pytest.raises(ValueError):
            m.jpeg(0, 1, sampling="4:4:0")
        assert m.jpeg_sampling == "4:4:4"


def test_symbols_are_exported_declared_and_bound(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    p = inspect.signature(Mount.jpeg).parameters
    assert list(p)[1:5] == ["first", "count", "gain", "quality"] and p["sampling"].default is None and list(p)[-1] == "resample"
    for f in (jpeg.mcus, jpeg.header, jpeg.coefficients, jpeg.encode):
        q = inspect.signature(f).parameters
        assert list(q)[-1] == "sampling" and q["sampling"].default == 420, f.__name__


def test_the_same_through_a_sanitized_stand_alone_program(amd, tmp_path):
    """tests/jpeg_sampling_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and
    run directly: mlvfs_amd_jpeg_header_sampled writes exactly its size (the program's buffers are that long and no longer), the layout
    arithmetic of the largest input overflows nowhere at any sampling, and the refusals follow no pointer."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    records = 0
    with open(cases, "wb") as f:
        for sampling, code in CODES:
            for pw, ph in SIZES + ((4112, 8), (8, 8200)):
                for q in (1, 50, 90, 100):
                    f.write(struct.pack("<Iiiii", 1, pw, ph, q, code) + jpeg.header(pw, ph, q, sampling))
                    records += 1
                f.write(struct.pack("<Iiiii", 2, pw, ph, 0, code) + struct.pack("<ii", *jpeg.mcus(pw, ph, sampling)))
                records += 1
    exe = tmp_path / "jpeg_sampling_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "jpeg_sampling_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"jpeg_sampling_host_check: {records} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
