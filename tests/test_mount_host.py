"""The mount API and the batched stages without a GPU: argument checks that refuse before any device work, and the options
struct as ctypes sees it against the header (csrc/mount.cpp, include/mlvfs_amd.h)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_mount_options_layout_matches_the_header(tmp_path):
    fields = [f for f, _ in lib.MountOpts._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlvfs_amd.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mlvfs_amd_mount_opts_t));\n' +
                   "".join(f'  printf(" %zu", offsetof(mlvfs_amd_mount_opts_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(lib.MountOpts)] + [getattr(lib.MountOpts, f).offset for f in fields]


@pytest.fixture()
def clip(tmp_path):
    w, h = 256, 130
    pl = [synth.pack_bits(synth.normal_frame(w, h, frame=k)).tobytes() for k in range(3)]
    names = mlvfile.write_clip(str(tmp_path / "C.MLV"), pl, w, h)
    r = mlvfile.MlvReader(names[0])
    yield r, w, h
    r.close()


def _err(L):
    return L.mlvfs_amd_last_error().decode()


def test_mount_open_refuses_bad_arguments(clip):
    L = lib.load()
    r, _, _ = clip
    ok = lib.MountOpts(chroma_smooth=5, rand_mode=1)
    assert not L.mlvfs_amd_mount_open(None, C.byref(ok), b"/C.MLV") and "null" in _err(L)
    assert not L.mlvfs_amd_mount_open(r.h, None, b"/C.MLV") and "null" in _err(L)
    for bad in (dict(dual_iso=3), dict(fix_bad_pixels=3), dict(rand_mode=2), dict(hdr_interpolation_method=2), dict(deflicker=-1),
                dict(fps=-1.0)):
        o = lib.MountOpts(**bad)
        assert not L.mlvfs_amd_mount_open(r.h, C.byref(o), b"/C.MLV"), bad
        assert "out of range" in _err(L)
    m = L.mlvfs_amd_mount_open(r.h, C.byref(ok), None)                   # no basename: an empty one
    assert m
    L.mlvfs_amd_mount_close(m)
    L.mlvfs_amd_mount_close(None)


def test_mount_dng_refuses_bad_arguments_before_device_work(clip):
    L = lib.load()
    r, w, h = clip
    o = lib.MountOpts(chroma_smooth=5, fix_stripes=1, rand_mode=1)
    m = L.mlvfs_amd_mount_open(r.h, C.byref(o), b"/C.MLV")
    size = 65536 + w * h * 2
    out = np.zeros((3, size), np.uint8)
    try:
        assert L.mlvfs_amd_mount_dng(None, 0, 1, lib.ptr(out), size, 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert L.mlvfs_amd_mount_dng(m, 0, 1, None, size, 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert L.mlvfs_amd_mount_dng(m, 0, -1, lib.ptr(out), size, 2, 1, None) == lib.ERR_ARG and "negative" in _err(L)
        for first, count in ((-1, 1), (2, 2), (3, 1), (0, 4)):
            assert L.mlvfs_amd_mount_dng(m, first, count, lib.ptr(out), size, 2, 1, None) == lib.ERR_ARG, (first, count)
            assert "outside the clip" in _err(L)
        assert L.mlvfs_amd_mount_dng(m, 0, 2, lib.ptr(out), size - 1, 2, 1, None) == lib.ERR_ARG and "out_stride" in _err(L)
        assert L.mlvfs_amd_mount_dng(m, 1, 0, lib.ptr(out), size, 2, 1, None) == lib.OK     # nothing to serve
        assert not out.any()
    finally:
        L.mlvfs_amd_mount_close(m)


def test_batched_stages_refuse_bad_arguments_before_device_work():
    L = lib.load()
    g = lib.Geom(256, 130, 14, synth.BLACK, synth.WHITE, 0, 0)
    eb = np.zeros(4, np.int32)
    res = np.zeros(2, np.int32)
    fake = C.c_void_p(0x1000)                                            # never dereferenced: every call below is refused first
    assert L.mlvfs_amd_fix_pattern_noise_dev(None, fake, 0, 1, None) == lib.ERR_ARG and "null" in _err(L)
    assert L.mlvfs_amd_fix_pattern_noise_dev(C.byref(g), None, 0, 1, None) == lib.ERR_ARG
    for bad in (lib.Geom(255, 130, 14, 0, 0, 0, 0), lib.Geom(256, 131, 14, 0, 0, 0, 0), lib.Geom(0, 0, 14, 0, 0, 0, 0)):
        assert L.mlvfs_amd_fix_pattern_noise_dev(C.byref(bad), fake, 0, 1, None) == lib.ERR_ARG and "not supported" in _err(L)
    assert L.mlvfs_amd_fix_pattern_noise_dev(C.byref(g), fake, 256 * 130 * 2 - 2, 2, None) == lib.ERR_ARG and "stride" in _err(L)
    assert L.mlvfs_amd_fix_pattern_noise_dev(C.byref(g), fake, 0, -1, None) == lib.ERR_ARG
    assert L.mlvfs_amd_deflicker_batch_dev(C.byref(g), fake, 0, 1, 256 * 130 * 2, 3000, None, None) == lib.ERR_ARG and "null" in _err(L)
    for bpp, size in ((0, 256 * 130 * 2), (16, 256 * 130 * 2), (14, 1), (14, 256 * 130 * 2 + 2)):
        g2 = lib.Geom(256, 130, bpp, synth.BLACK, synth.WHITE, 0, 0)
        assert L.mlvfs_amd_deflicker_batch_dev(C.byref(g2), fake, 0, 1, size, 3000, lib.ptr(eb), None) == lib.ERR_ARG, (bpp, size)
    assert L.mlvfs_amd_deflicker_batch_dev(C.byref(g), fake, 100, 2, 256 * 130 * 2, 3000, lib.ptr(eb), None) == lib.ERR_ARG
    assert L.mlvfs_amd_hdr_preview_batch_dev(C.byref(g), fake, 0, 1, 256 * 130 * 2, None, None) == lib.ERR_ARG and "null" in _err(L)
    assert L.mlvfs_amd_hdr_preview_batch_dev(None, fake, 0, 1, 256 * 130 * 2, lib.ptr(res), None) == lib.ERR_ARG
    assert L.mlvfs_amd_hdr_preview_batch_dev(C.byref(g), fake, 7, 2, 256 * 130 * 2, lib.ptr(res), None) == lib.ERR_ARG and "stride" in _err(L)
    # zero frames: nothing to do, nothing touched
    assert L.mlvfs_amd_fix_pattern_noise_dev(C.byref(g), fake, 0, 0, None) == lib.OK
    assert L.mlvfs_amd_hdr_preview_batch_dev(C.byref(g), fake, 0, 0, 256 * 130 * 2, lib.ptr(res), None) == lib.OK


def test_mount_python_wrapper_checks_the_results_array(clip):
    from mlvfs_amd.mount import Mount
    from mlvfs_amd.pipeline import MlvfsOptions
    r, _, _ = clip
    with Mount(r, MlvfsOptions(chroma_smooth=5)) as m:
        for bad in (np.zeros(1, np.int32), np.zeros(3, np.int64), np.zeros(6, np.int32)[::2], [0, 0, 0]):
            with pytest.raises(ValueError, match="int32"):
                m.dng(0, 3, results=bad)


def test_pattern_noise_scratch_cap_hook():
    L = lib.load()
    before = L.mlvfs_amd_test_pn_scratch_cap(12345)
    try:
        assert before > 0
        assert L.mlvfs_amd_test_pn_scratch_cap(0) == 12345
        assert L.mlvfs_amd_test_pn_scratch_cap(0) == before                # 0: the default again
    finally:
        L.mlvfs_amd_test_pn_scratch_cap(0)
