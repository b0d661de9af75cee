"""The tensor route's host code (csrc/tensor.cpp, csrc/mount.cpp; no GPU): every refusal of mlvfs_amd_tensor_rgb_dev,
mlvfs_amd_tensor_bayer_dev, mlvfs_amd_mount_tensor and mlvfs_amd_mount_tensor_bytes that happens before any device work, with nothing
written; mlvfs_amd_tensor_bayer_params against Python integers; the sizes mlvfs_amd_mount_tensor_bytes answers; the export table and the
Python binding -- and the same once more through a stand-alone C++ program (tests/tensor_host_check.cpp) built with
-fsanitize=address,undefined against the sanitizer build of the host code (`make hostcheck`, built here if it is not yet).  Nothing is
loaded into Python under a sanitizer.  The GPU side: tests/test_gpu_tensor.py, tests/test_gpu_mount_tensor.py."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from mlvfs_amd import abi, lib, mlvfile, synth, tensor as T
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import tensor_cases as tc
from test_cabi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK_SO = os.path.join(ROOT, "mlvfs_amd", "libmlvfs_amd_hostcheck.so")
TENSOR_SYMBOLS = ["mlvfs_amd_tensor_rgb_dev", "mlvfs_amd_tensor_bayer_params", "mlvfs_amd_tensor_bayer_dev", "mlvfs_amd_mount_tensor",
                  "mlvfs_amd_mount_tensor_bytes"]
W, H = 64, 48
# (black, white) -> the helper's answer; refused beyond |black| = 2^30
LEVEL_CASES = tc.LEVELS + [(0, 0), (0, 1), (5, 3), (0, 65535), (1 << 30, (1 << 31) - 1), (-(1 << 30), (1 << 31) - 1), (-(1 << 30), -(1 << 30)),
                           ((1 << 30) + 1, (1 << 31) - 1), (-(1 << 30) - 1, 0), ((1 << 31) - 1, 0), (-(1 << 31), 0)]


def unit_bits(rng):
    return struct.unpack("<i", struct.pack("<f", 1.0 / rng))[0]          # the double quotient, rounded once by the pack


def level_answer(black, white):
    if abs(black) > 1 << 30:
        return None
    rng = max(white - black, 1)
    return [black, min(rng, (1 << 31) - 1), unit_bits(rng), 0]          # the range is reported as an int32; unit is of the range itself


def spec(kind=T.RGB, dtype=T.F16, layout=T.NCHW, scale=1.0, bias=0.0, **more):
    sp = lib.TensorSpec(kind=kind, dtype=dtype, layout=layout, gain_q8=256, **more)
    sp.scale[:], sp.bias[:] = [scale] * 4, [bias] * 4
    return sp


def write_clip(tmp_path):
    path = str(tmp_path / "T.MLV")
    frames = [synth.normal_frame(W, H, seed=3, frame=k) for k in range(2)]
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], W, H)
    return path


def test_bayer_params_against_python_integers(amd):
    for black, white in LEVEL_CASES:
        fh = abi.make_frame_headers(W, H, black=black, white=white)
        out = np.full(4, -7, np.int32)
        rc = amd.mlvfs_amd_tensor_bayer_params(C.byref(fh), lib.ptr(out))
        want = level_answer(black, white)
        if want is None:
            assert rc == lib.ERR_ARG and (out == -7).all() and b"2^30" in amd.mlvfs_amd_last_error(), (black, white)
            with pytest.raises(ValueError):
                T.bayer_levels(black, white)
        else:
            assert rc == 0 and out.tolist() == want, (black, white)
            b, r, u = T.bayer_levels(black, white)
            assert [b, min(r, (1 << 31) - 1), int(np.array([u], np.float32).view(np.int32)[0]), 0] == want
    out = np.full(4, -7, np.int32)
    fh = abi.make_frame_headers(W, H)
    assert amd.mlvfs_amd_tensor_bayer_params(None, lib.ptr(out)) == lib.ERR_ARG and amd.mlvfs_amd_tensor_bayer_params(C.byref(fh), None) == lib.ERR_ARG
    assert (out == -7).all()


def test_the_device_calls_refuse_on_the_host(amd):
    """every check happens before any device work: no pointer is followed (they are host memory here)"""
    src, dst, lv = np.full(1024, 7, np.uint8), np.full(1024, 9, np.uint8), np.zeros(8, np.int32)
    s, d, p = src.ctypes.data, dst.ctypes.data, lv.ctypes.data
    vp = lambda a: C.c_void_p(a) if a else None
    rgb = lambda sp_, st, w, h, bits, spec_, dp, ost, n: amd.mlvfs_amd_tensor_rgb_dev(vp(sp_), st, w, h, bits, C.byref(spec_) if spec_ else None, vp(dp), ost, n, None)
    bay = lambda sp_, st, w, h, lp, spec_, dp, ost, n: amd.mlvfs_amd_tensor_bayer_dev(vp(sp_), st, w, h, vp(lp), C.byref(spec_) if spec_ else None, vp(dp), ost, n, None)
    ok = spec()
    for args, word in (((0, 192, 8, 8, 8, ok, d, 384, 1), b"null"), ((s, 192, 8, 8, 8, None, d, 384, 1), b"null"), ((s, 192, 8, 8, 8, ok, 0, 384, 1), b"null"),
                       ((s, 192, 0, 8, 8, ok, d, 384, 1), b"not supported"), ((s, 192, 8, -1, 8, ok, d, 384, 1), b"not supported"),
                       ((s, 192, 1 << 14, 1 << 14, 8, ok, d, 384, 1), b"not supported"), ((s, 192, 8, 8, 12, ok, d, 384, 1), b"bits"),
                       ((s, 192, 8, 8, 8, ok, d, 384, -1), b"negative"), ((s, 191, 8, 8, 8, ok, d, 384, 2), b"stride"), ((s, 192, 8, 8, 8, ok, d, 382, 2), b"stride"),
                       ((s, 192, 8, 8, 8, ok, d, 385, 2), b"stride"), ((s, 192, 8, 8, 8, ok, d, 382, 1), b"stride"), ((s, 192, 8, 8, 8, ok, d + 1, 384, 1), b"boundary"),
                       ((s + 1, 384, 8, 8, 16, ok, d, 384, 1), b"boundary"), ((s, 385, 8, 8, 16, ok, d, 384, 2), b"stride"),
                       ((s, 192, 8, 8, 8, ok, s, 384, 1), b"overlap"), ((s, 192, 8, 8, 8, ok, s + 190, 384, 1), b"overlap"), ((s + 400, 192, 8, 8, 8, ok, s + 18, 384, 1), b"overlap"),
                       ((s, 192, 8, 8, 8, spec(dtype=T.U16), d, 384, 1), b"illegal"), ((s, 384, 8, 8, 16, spec(dtype=T.U8), d, 192, 1), b"illegal"),
                       ((s, 192, 8, 8, 8, spec(dtype=5), d, 384, 1), b"dtype"), ((s, 192, 8, 8, 8, spec(dtype=-1), d, 384, 1), b"dtype"),
                       ((s, 192, 8, 8, 8, spec(layout=2), d, 384, 1), b"layout"), ((s, 192, 8, 8, 8, spec(scale=float("inf")), d, 384, 1), b"range"),
                       ((s, 192, 8, 8, 8, spec(bias=float("nan")), d, 384, 1), b"range"), ((s, 192, 8, 8, 8, spec(scale=2.0 ** 65), d, 384, 1), b"range"),
                       ((s, 192, 8, 8, 8, spec(scale=-2.0 ** -65), d, 384, 1), b"range"), ((s, 192, 8, 8, 8, spec(bias=2.0 ** -65), d, 384, 1), b"range")):
        assert rgb(*args) == lib.ERR_ARG and word in amd.mlvfs_amd_last_error(), (args[:5] + args[6:], amd.mlvfs_amd_last_error())
    for args, word in (((0, 512, 16, 16, p, ok, d, 512, 1), b"null"), ((s, 512, 16, 16, 0, ok, d, 512, 1), b"null"), ((s, 512, 16, 16, p, None, d, 512, 1), b"null"),
                       ((s, 512, 16, 16, p, ok, 0, 512, 1), b"null"), ((s, 512, 1, 16, p, ok, d, 512, 1), b"not supported"), ((s, 512, 16, 1, p, ok, d, 512, 1), b"not supported"),
                       ((s, 512, 1 << 14, 1 << 14, p, ok, d, 512, 1), b"not supported"), ((s, 512, 16, 16, p, ok, d, 512, -1), b"negative"),
                       ((s, 510, 16, 16, p, ok, d, 512, 2), b"stride"), ((s, 513, 16, 16, p, ok, d, 512, 2), b"stride"), ((s, 512, 16, 16, p, ok, d, 510, 2), b"stride"),
                       ((s + 1, 512, 16, 16, p, ok, d, 512, 1), b"boundary"), ((s, 512, 16, 16, p + 2, ok, d, 512, 1), b"4-byte"), ((s, 512, 16, 16, p, ok, d + 1, 512, 1), b"boundary"),
                       ((s, 512, 16, 16, p, spec(dtype=T.U8), d, 512, 1), b"illegal"), ((s, 512, 16, 16, p, spec(scale=float("-inf")), d, 512, 1), b"range"),
                       ((s, 512, 16, 16, p, ok, s + 510, 512, 1), b"overlap"), ((s, 512, 16, 16, d + 64, ok, d, 512, 1), b"overlap")):
        assert bay(*args) == lib.ERR_ARG and word in amd.mlvfs_amd_last_error(), (args[:4] + args[6:], amd.mlvfs_amd_last_error())
    # the fourth channel of an RGB spec is not read; an integer dtype reads neither scale nor bias; nothing to do is no error
    sp3 = spec()
    sp3.scale[3] = float("nan")
    assert rgb(s, 192, 8, 8, 8, sp3, d, 384, 0) == 0 and bay(s, 512, 16, 16, p, sp3, d, 512, 0) == lib.ERR_ARG
    assert rgb(s, 192, 8, 8, 8, spec(dtype=T.U8, scale=float("nan")), d, 192, 0) == 0 and bay(s, 512, 16, 16, p, spec(dtype=T.U16, bias=float("inf")), d, 512, 0) == 0
    assert (src == 7).all() and (dst == 9).all() and not lv.any()


def test_mount_tensor_bytes_and_the_mounts_refusals(amd, tmp_path):
    path = write_clip(tmp_path)
    dst = np.full(1024, 9, np.uint8)
    d = dst.ctypes.data
    with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions()) as m:
        size = lambda sp_: amd.mlvfs_amd_mount_tensor_bytes(m.h, 0, C.byref(sp_))
        pw, ph = W // 2, H // 2
        for dtype, es in T.ELEM.items():
            if T.legal(dtype, 8):
                assert size(spec(dtype=dtype)) == 3 * pw * ph * es == m.tensor_bytes(0, spec(dtype=dtype))
                assert size(spec(dtype=dtype, size=T.FULL, layout=T.NHWC)) == 3 * W * H * es
                assert size(spec(dtype=dtype, size=T.SCALED, ow=5, oh=3)) == 45 * es
                assert size(spec(dtype=dtype, size=T.RESAMPLED, ow=W, oh=H - 1)) == 3 * W * (H - 1) * es
            if T.legal(dtype, 16):
                assert size(spec(kind=T.BAYER, dtype=dtype)) == 4 * pw * ph * es
        m.set_demosaic("amaze")                          # the handle's route decides: the resampled calls have a route of their own
        assert size(spec(size=T.FULL)) == 3 * W * H * 2
        m.set_resample_demosaic("amaze")
        assert size(spec(size=T.RESAMPLED, ow=W, oh=H)) == 3 * W * H * 2
        m.set_demosaic("linear")
        m.set_resample_demosaic("linear")
        refused = [(spec(size=T.SCALED, ow=pw + 1, oh=1), b"not supported"), (spec(size=T.RESAMPLED, ow=1, oh=H + 1), b"not supported"), (spec(size=4), b"size kind"),
                   (spec(size=-1), b"size kind"), (spec(size=T.SCALED), b"scaled rendering"), (spec(dtype=T.U16), b"illegal"), (spec(kind=2), b"kind"),
                   (spec(kind=T.BAYER, dtype=T.U8), b"illegal"), (spec(dtype=7), b"dtype"), (spec(layout=3), b"layout"), (spec(scale=float("inf")), b"range"),
                   (spec(kind=T.BAYER, bias=2.0 ** 70), b"range")]
        sp0 = spec()
        sp0.gain_q8 = 0
        refused.append((sp0, b"gain_q8"))
        for sp_, word in refused:
            assert size(sp_) == 0 and word in amd.mlvfs_amd_last_error(), amd.mlvfs_amd_last_error()
            assert amd.mlvfs_amd_mount_tensor(m.h, 0, 1, C.c_void_p(d), 1 << 20, C.byref(sp_), 2, 0, None) == lib.ERR_ARG and word in amd.mlvfs_amd_last_error()
            with pytest.raises(lib.MlvfsAmdError):
                m.tensor_bytes(0, sp_)
        ok = spec()
        assert amd.mlvfs_amd_mount_tensor_bytes(None, 0, C.byref(ok)) == 0 and amd.mlvfs_amd_mount_tensor_bytes(m.h, 0, None) == 0
        assert amd.mlvfs_amd_mount_tensor_bytes(m.h, -1, C.byref(ok)) == 0 and amd.mlvfs_amd_mount_tensor_bytes(m.h, 2, C.byref(ok)) == 0
        need = 3 * pw * ph * 2
        call = lambda mh, first, count, dp, stride, sp_: amd.mlvfs_amd_mount_tensor(mh, first, count, C.c_void_p(dp) if dp else None, stride, C.byref(sp_) if sp_ else None, 2, 0, None)
        for args in ((None, 0, 1, d, need, ok), (m.h, 0, 1, 0, need, ok), (m.h, 0, 1, d, need, None), (m.h, 0, -1, d, need, ok), (m.h, 2, 1, d, need, ok), (m.h, 1, 2, d, need, ok),
                     (m.h, 0, 1, d, need - 2, ok), (m.h, 0, 1, d, need + 1, ok), (m.h, 0, 1, d + 1, need, ok)):
            assert call(*args) == lib.ERR_ARG, args[1:5]
        assert call(m.h, 0, 0, d, need, ok) == 0
    with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions(), proxy=2) as m:
        for sp_, need in ((spec(), 3 * (W // 2) * (H // 2) * 2), (spec(kind=T.BAYER), 4 * (W // 2) * (H // 2) * 2)):
            assert amd.mlvfs_amd_mount_tensor(m.h, 0, 1, C.c_void_p(d), need, C.byref(sp_), 2, 0, None) == lib.ERR_ARG and b"prox" in amd.mlvfs_amd_last_error()
    assert (dst == 9).all()


def test_the_python_side_refuses_what_it_must(amd, tmp_path):
    path = write_clip(tmp_path)
    with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions()) as m:
        for kw in (dict(kind="yuv"), dict(dtype="int8"), dict(layout="CHWN"), dict(gain=0.0), dict(full=True, size=(4, 4)), dict(resample=True),
                   dict(mean=(1, 2), std=1.0)):
            with pytest.raises(ValueError):
                m._tensor_spec(**{**dict(kind="rgb", dtype="float16", layout="NCHW", mean=None, std=None, gain=1.0, full=False, size=None, resample=False, look16=None), **kw})
        sp_, channels = m._tensor_spec("bayer", "bfloat16", "NHWC", 0.5, 0.25, 1.0, False, None, False, None)
        assert (sp_.kind, sp_.dtype, sp_.layout, channels) == (T.BAYER, T.BF16, T.NHWC, 4) and list(sp_.scale) == [4.0] * 4 and list(sp_.bias) == [-2.0] * 4
        sp_, channels = m._tensor_spec("rgb", "float32", "NCHW", (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 1.5, False, (20, 13), True, None)
        assert (sp_.size, sp_.ow, sp_.oh, sp_.gain_q8, channels) == (T.RESAMPLED, 20, 13, 384, 3) and sp_.scale[0] == np.float32(1.0 / 0.229) and sp_.scale[3] == 1.0
    doc = inspect.getdoc(Mount.tensor)
    assert "synchronises torch's current stream" in doc and list(inspect.signature(Mount.tensor).parameters)[1:5] == ["first", "count", "kind", "dtype"]
    assert inspect.isgeneratorfunction(Mount.tensors)


def test_tensor_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in TENSOR_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    header = open(os.path.join(ROOT, "include", "mlvfs_amd.h")).read()
    for name, value in (("RGB", T.RGB), ("BAYER", T.BAYER), ("HALF", T.HALF), ("FULL", T.FULL), ("SCALED", T.SCALED), ("RESAMPLED", T.RESAMPLED), ("F32", T.F32),
                        ("F16", T.F16), ("BF16", T.BF16), ("U8", T.U8), ("U16", T.U16), ("NCHW", T.NCHW), ("NHWC", T.NHWC)):
        assert f"#define MLVFS_AMD_TENSOR_{name:<9} {value}" in header, name
    assert C.sizeof(lib.TensorSpec) == 72 and lib.TensorSpec.look16.offset == 32 and lib.TensorSpec.scale.offset == 40 and lib.TensorSpec.bias.offset == 56


def test_the_same_through_a_sanitized_stand_alone_program(tmp_path):
    """tests/tensor_host_check.cpp, compiled and linked with -fsanitize=address,undefined against libmlvfs_amd_hostcheck.so and run
    directly: the helper writes exactly its four words, and the refusals follow no pointer and write nothing."""
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "mlvfs_amd", "csrc"), "hostcheck", "-j8"], capture_output=True, text=True)     # (as tests/test_hostcheck.py does)
    assert m.returncode == 0 and os.path.exists(HOSTCHECK_SO), m.stdout[-2000:] + m.stderr[-2000:]
    cases = tmp_path / "cases.bin"
    with open(cases, "wb") as f:
        for black, white in LEVEL_CASES:
            f.write(struct.pack("<2i4i", black, white, *(level_answer(black, white) or [0, 0, 0, 0])))
    clip = write_clip(tmp_path)
    exe = tmp_path / "tensor_host_check"
    so_dir = os.path.dirname(HOSTCHECK_SO)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "tensor_host_check.cpp"), "-o", str(exe), "-L", so_dir, "-l:libmlvfs_amd_hostcheck.so",
                        "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe), str(cases), clip, str(W), str(H)], capture_output=True, text=True, timeout=300, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and f"tensor_host_check: {len(LEVEL_CASES)} records" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
