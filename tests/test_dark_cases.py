"""Dark frames, the part that needs no GPU: the cases of tests/dark_cases.py really exercise both clamps and the rounding, the
pre-subtracted clips really differ from their sources, and the host-only entry points (mlvfs_amd_dark_create / _info / _plane, the
argument checks of the device entry points) with the export table and the Python binding.  The GPU side: tests/test_gpu_dark.py."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import dark_cases as dc
from test_cabi import declared_functions

DARK_SYMBOLS = ["mlvfs_amd_dark_create", "mlvfs_amd_dark_from_clip", "mlvfs_amd_dark_info", "mlvfs_amd_dark_plane", "mlvfs_amd_dark_destroy",
                "mlvfs_amd_dark_subtract_dev", "mlvfs_amd_mount_set_dark", "mlvfs_amd_mlv_transcode_dark"]


@pytest.mark.parametrize("w,h,bpp,n,off", dc.SUB_CASES, ids=lambda v: str(v))
def test_every_subtraction_case_clamps_both_ways_and_not_at_all(w, h, bpp, n, off):
    black_d = dc.clip_black(bpp) + off
    frames, dark, want = dc.sub_case(w, h, bpp, n, black_d)
    assert len(frames) == n and dark.shape == (h, w)
    for f, o in zip(frames, want):
        lo, hi, mid = dc.clamp_classes(f, dark, black_d, bpp)
        assert lo > 0 and hi > 0 and mid > 0, (lo, hi, mid)
        assert int(o.max()) == (1 << bpp) - 1 and int(o.min()) == 0
        assert int(f.max()) < (1 << bpp)
    assert {off for *_, off in dc.SUB_CASES} == {0, -37}                 # black_d equal to the clip's black level and different from it


@pytest.mark.parametrize("kind,black_d", [("plain", dc.BLACK), ("plain", dc.BLACK - 48), ("dual_iso", dc.BLACK)])
def test_every_clip_case_clamps_both_ways_and_the_subtracted_clip_differs(oracle, kind, black_d):
    frames, dark, pre = dc.clip_case(kind, black_d=black_d)
    for f, p in zip(frames, pre):
        lo, hi, mid = dc.clamp_classes(f, dark, black_d, 14)
        assert lo >= len(dc.ZERO_AT) and hi >= len(dc.TOP_AT) and mid > f.size * 9 // 10, (lo, hi, mid)
        assert int(f.max()) < 16384 and p[0, 0] != 0
        assert not np.array_equal(f, p) and (f != p).mean() > 0.5          # the subtraction changes most of the frame
    # ... and what the stages behind it give: the equalities of test_gpu_dark.py cannot hold for a stage-0 that does nothing
    a, b = oracle.chroma_smooth(frames[0], dc.BLACK, 5), oracle.chroma_smooth(pre[0], dc.BLACK, 5)
    assert not np.array_equal(a, b)
    assert not np.array_equal(b, dc.subtract(a, dark, black_d, 14))         # nor for a subtraction behind the stages instead of in front


@pytest.mark.parametrize("w,h,bpp", dc.DEPTH_CASES, ids=lambda v: str(v))
def test_every_depth_case_clamps_both_ways_and_takes_the_path_it_is_there_for(w, h, bpp):
    frames, dark, black_d, pre = dc.depth_case(w, h, bpp)
    top = (1 << bpp) - 1
    for f, p in zip(frames, pre):
        lo, hi, mid = dc.clamp_classes(f, dark, black_d, bpp)
        assert lo > 0 and hi > 0 and mid > f.size // 2, (lo, hi, mid)
        assert int(f.max()) <= top and int(p.max()) == top and int(p.min()) == 0 and not np.array_equal(f, p)
    assert (w * h * bpp) % 16 == 0                                        # the clip's frame_size holds every pixel
    fused = bpp in (10, 12, 14) and (w * h) % 16 == 0                      # launch_cal_unpack's choice (csrc/k_cal.hip)
    assert fused == ((w, h, bpp) in [(dc.W, dc.H, 12), (dc.W, dc.H, 10)])
    assert {b for _, _, b in dc.DEPTH_CASES if b != 14} == {10, 12, 16}


def test_averaging_cases_hit_the_rounding_boundary():
    assert 1 in dc.AVG_COUNTS and any(n % 2 == 0 for n in dc.AVG_COUNTS) and any(n > 3 for n in dc.AVG_COUNTS)
    for w, h in dc.AVG_GEOMETRIES:
        for n in dc.AVG_COUNTS:
            frames, want = dc.avg_case(w, h, n)
            sums = sum(f.astype(np.int64) for f in frames)
            assert np.array_equal(want, np.floor(sums / n + 0.5).astype(np.uint16))      # round half up, in exact arithmetic
            if n == 1:
                assert np.array_equal(want, frames[0])
                continue
            v = dc.BLACK + 13
            assert int(sums[0, 0]) % n == n // 2 and int(sums[0, 1]) % n == n // 2 - 1
            assert int(want[0, 1]) == v and int(want[0, 2]) == v + 1
            if n % 2 == 0:
                assert int(sums[0, 0]) * 2 == (2 * v + 1) * n and int(want[0, 0]) == v + 1     # exactly half way: up
            else:
                assert int(want[0, 0]) == v
            assert len({int(s) % n for s in sums.reshape(-1)}) == n                     # every remainder occurs
    assert (dc.AVG_GEOMETRIES[0][0] * dc.AVG_GEOMETRIES[0][1]) % 16 == 0 and (dc.AVG_GEOMETRIES[1][0] * dc.AVG_GEOMETRIES[1][1]) % 16 == 8


# ---- host-only entry points ------------------------------------------------------------------------------------------
def test_create_info_plane_round_trip(amd):
    rng = np.random.default_rng(4)
    for w, h, bpp, black in ((16, 2, 14, 2048), (3, 5, 10, 0), (30, 10, 16, 65535), (1, 1, 1, 1)):
        plane = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        with Dark.from_plane(plane, bpp, black) as d:
            assert d.info() == dict(width=w, height=h, bpp=bpp, black=black, frames_averaged=0)
            assert np.array_equal(d.plane(), plane)
            plane[0, 0] ^= 1                                               # the handle keeps its own copy
            assert not np.array_equal(d.plane(), plane)
            big = np.full(w * h + 3, 0xABCD, np.uint16)
            assert amd.mlvfs_amd_dark_plane(d.h, lib.ptr(big), big.size) == 0 and (big[w * h:] == 0xABCD).all()
            assert amd.mlvfs_amd_dark_info(d.h, None, None) == 0
        assert d.h is None


def test_host_refusals(amd):
    plane = np.zeros((4, 16), np.uint16)

    def create(w, h, bpp, black, p=plane):
        g = lib.Geom(w, h, bpp, black, 0, 0, 0)
        return amd.mlvfs_amd_dark_create(C.byref(g), None if p is None else lib.ptr(p))

    assert create(16, 4, 14, 2048, None) is None and b"null" in amd.mlvfs_amd_last_error()
    assert amd.mlvfs_amd_dark_create(None, lib.ptr(plane)) is None
    for bpp in (0, 17, -1, 32):
        assert create(16, 4, bpp, 2048) is None and b"bits_per_pixel" in amd.mlvfs_amd_last_error(), bpp
    for w, h in ((0, 4), (16, 0), (-16, 4), (16, -4), (1 << 14, 1 << 13)):
        assert create(w, h, 14, 2048) is None and b"not supported" in amd.mlvfs_amd_last_error(), (w, h)
    for black in (-1, 65536):
        assert create(16, 4, 14, black) is None, black
    h = create(16, 4, 14, 2048)
    assert h
    try:
        out = np.full(64, 7, np.uint16)
        assert amd.mlvfs_amd_dark_plane(h, lib.ptr(out), 63) == lib.ERR_ARG and (out == 7).all()          # cap_pixels too small
        assert amd.mlvfs_amd_dark_plane(h, None, 64) == lib.ERR_ARG and amd.mlvfs_amd_dark_plane(None, lib.ptr(out), 64) == lib.ERR_ARG
        assert amd.mlvfs_amd_dark_info(None, None, None) == lib.ERR_ARG
        # the device entry point refuses on the host, before any device work: the pointers are never followed
        sub, buf = amd.mlvfs_amd_dark_subtract_dev, lib.ptr(out)
        g = lambda w, hh, bpp: C.byref(lib.Geom(w, hh, bpp, 0, 0, 0, 0))
        for w, hh, bpp in ((16, 2, 14), (8, 4, 14), (16, 4, 12)):
            assert sub(h, g(w, hh, bpp), buf, 128, 1, None) == lib.ERR_ARG, (w, hh, bpp)
        assert sub(None, g(16, 4, 14), buf, 128, 1, None) == lib.ERR_ARG and sub(h, None, buf, 128, 1, None) == lib.ERR_ARG
        assert sub(h, g(16, 4, 14), None, 128, 1, None) == lib.ERR_ARG and sub(h, g(16, 4, 14), buf, 128, -1, None) == lib.ERR_ARG
        assert sub(h, g(16, 4, 14), buf, 126, 2, None) == lib.ERR_ARG and sub(h, g(16, 4, 14), buf, 129, 2, None) == lib.ERR_ARG
        assert sub(h, g(16, 4, 14), C.c_void_p(out.ctypes.data + 1), 128, 1, None) == lib.ERR_ARG
        assert sub(h, g(16, 4, 14), buf, 128, 0, None) == 0
        assert (out == 7).all()
    finally:
        amd.mlvfs_amd_dark_destroy(h)
    amd.mlvfs_amd_dark_destroy(None)
    with pytest.raises(ValueError):
        Dark.from_plane(np.zeros((4, 16), np.int32), 14, 2048)


def test_from_clip_and_the_users_refuse_on_the_host(amd, tmp_path):
    """Frames outside the clip, too many frames, a dark frame of another geometry: refused before any device work and before any
    output file exists."""
    frames = [synth.normal_frame(64, 48, seed=3, frame=k) for k in range(3)]
    names = mlvfile.write_clip(str(tmp_path / "A.MLV"), [synth.pack_bits(f).tobytes() for f in frames], 64, 48)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        for first, count in ((0, 4), (2, 2), (3, 1), (-1, 2), (0, 0), (0, -1), (0, 65537), (0, 1 << 20)):
            assert amd.mlvfs_amd_dark_from_clip(r.h, first, count, 3, 2) is None, (first, count)
        assert amd.mlvfs_amd_dark_from_clip(None, 0, 1, 3, 2) is None
        for shape, bpp in (((48, 32), 14), ((24, 64), 14), ((48, 64), 12)):
            with Dark.from_plane(np.zeros(shape, np.uint16), bpp, 2048) as d:
                with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                    Mount(r, MlvfsOptions(), dark=d)
                for lj92 in (False, True):
                    with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                        r.transcode(str(out / "B.MLV"), lj92=lj92, dark=d)
                    assert list(out.iterdir()) == []
        # without a dark frame mlvfs_amd_mlv_transcode_dark is mlvfs_amd_mlv_transcode, the host-only route included
        stats = (C.c_longlong * 4)()
        assert amd.mlvfs_amd_mlv_transcode_dark(r.h, str(out / "C.MLV").encode(), lib.MLV_PLAIN, None, 2, 2, stats) == 0
        assert r.transcode(str(out / "D.MLV"), lj92=False, batch=2, io_threads=2) == dict(frames=int(stats[0]), bytes_in=int(stats[1]),
                                                                                        bytes_out=int(stats[2]), files=int(stats[3]))
        assert (out / "C.MLV").read_bytes() == (out / "D.MLV").read_bytes() and stats[0] == 3


# ---- export and binding ----------------------------------------------------------------------------------------------
def test_dark_symbols_are_exported_and_declared(amd):
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = declared_functions()
    for s in DARK_SYMBOLS:
        assert s in exported and s in declared and s in lib.DEVICE_SYMBOLS and hasattr(amd, s), s
    assert {s for s in exported if s.startswith("mlvfs_amd_dark_")} == {s for s in DARK_SYMBOLS if s.startswith("mlvfs_amd_dark_")}


def test_mount_without_a_dark_frame_constructs_as_before(amd, tmp_path):
    assert inspect.signature(Mount.__init__).parameters["dark"].default is None
    frames = [synth.normal_frame(64, 48, seed=3, frame=k) for k in range(2)]
    names = mlvfile.write_clip(str(tmp_path / "A.MLV"), [synth.pack_bits(f).tobytes() for f in frames], 64, 48)
    with mlvfile.MlvReader(names[0]) as r:
        with Mount(r, MlvfsOptions(chroma_smooth=5), deflicker=3000, basename="/A.MLV") as a, \
                Mount(r, MlvfsOptions(chroma_smooth=5), deflicker=3000, basename="/A.MLV", dark=None) as b:
            assert a.h and b.h and a._dark is None and b._dark is None
            assert bytes(a.opts) == bytes(b.opts) and a.frame_count == b.frame_count == 2 and a.dng_size() == b.dng_size()
            with Dark.from_plane(np.zeros((48, 64), np.uint16), 14, 2048) as d:
                b.set_dark(d)
                b.set_dark(None)                                            # NULL clears
                assert b._dark is None
