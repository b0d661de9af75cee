"""Rendered full-size frames demosaiced by AMaZE through the mount (csrc/mount.cpp, csrc/amaze_render.cpp): with
mlvfs_amd_mount_set_demosaic(1) the three full-size calls serve the definition of mlvfs_amd/amaze_render.py (the checker's AMaZE) applied
to the pixels of the .dng file of the same clip and options, byte for byte -- TIFF, JPEG and 16-bit TIFF, with the handle's look too --
and PIL opens every file at W x H; the linear filter afterwards serves the linear files; the calls interleave with dng() and the
half-size calls; a clip whose frames go through the dual-ISO conversion's AMaZE first; the refusals.  The helpers are those of
tests/mount_harness.py."""
import os

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib, look, mlvfile, render, synth

import deep_cases as dc
import look_cases as lc
from mount_harness import (GAIN_A, GAIN_B, HDR, NAME, ORDER, QUALITY, check_jpegs, check_tiffs, fresh, load_tool, make_clip, open_mount, payloads,
                           renderings, run_tool, serve)

pytestmark = pytest.mark.gpu
OPTS = dict(cs=5, badpix=1, stripes=1)
SIZES = [(64, 48), (148, 40)]            # a width the fast forms take, and one they do not
LOOK, LOOK16 = lc.look_of("random17"), dc.look_of("random3")
FULL = dict(full=True)


def amaze(lk=None):
    """the setup of a handle that serves AMaZE at full size, with a look where one is given"""
    def setup(m):
        m.set_demosaic("amaze")
        if lk is not None:
            m.set_look(lk)
    return setup


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_mount_amaze_serves_the_definitions_files(gpu, oracle, tmp_path, w, h):
    label = f"amaze {w}x{h}"
    path = make_clip(tmp_path, "plain", w, h)
    full, _, res_full, _ = serve(gpu, path, OPTS, "dng")
    tiffs, _, res_rgb, gains = serve(gpu, path, OPTS, "rgb", FULL, setup=amaze())
    jpgs, flags, res_jpg, _ = serve(gpu, path, OPTS, "jpeg", FULL, setup=amaze())
    with look.Look16(*LOOK16) as lk16:
        deep, _, res_deep, _ = serve(gpu, path, OPTS, "rgb", dict(FULL, look16=lk16), setup=amaze())
    assert res_rgb == res_full == res_jpg == res_deep
    want = renderings(full, gains, w, h, "full+amaze", amaze=oracle.amaze_demosaic)
    check_tiffs(want, tiffs, (w, h), label)
    check_jpegs(want, jpgs, flags, (w, h), label, QUALITY)
    check_tiffs(renderings(full, gains, w, h, "full+amaze", amaze=oracle.amaze_demosaic, look16=LOOK16), deep, (w, h), label, bits=16)
    assert len(set(tiffs)) == len(tiffs)
    # another rendering than the linear filter's, which the same handle serves again once it is set back
    linear, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=ORDER)
    assert all(a != b for a, b in zip(linear, tiffs))
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        m.set_demosaic("amaze")
        first = [f.tobytes() for f in m.rgb(2, 3, gain=GAIN_A, batch=2, full=True)]
        m.set_demosaic("linear")
        second = [f.tobytes() for f in m.rgb(0, 2, gain=GAIN_B, batch=2, full=True)]
        m.set_demosaic("amaze")
        third, fl = m.jpeg(0, 2, gain=GAIN_B, quality=QUALITY, batch=2, full=True)
    assert first == tiffs[:3] and second == linear[3:] and third == jpgs[3:] and fl == flags[3:]


def test_mount_amaze_with_a_look(gpu, oracle, tmp_path):
    w, h = SIZES[0]
    path = make_clip(tmp_path, "plain", w, h)
    full, _, _, _ = serve(gpu, path, OPTS, "dng")
    with look.Look(*LOOK) as lk:
        tiffs, _, _, gains = serve(gpu, path, OPTS, "rgb", FULL, setup=amaze(lk))
        jpgs, flags, _, _ = serve(gpu, path, OPTS, "jpeg", FULL, setup=amaze(lk))
    want = renderings(full, gains, w, h, "full+amaze", amaze=oracle.amaze_demosaic, look=LOOK)
    check_tiffs(want, tiffs, (w, h), "amaze with a look")
    check_jpegs(want, jpgs, flags, (w, h), "amaze with a look", QUALITY)
    plain, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, setup=amaze())
    assert all(a != b for a, b in zip(plain, tiffs))


def test_amaze_calls_interleave_with_the_other_calls(gpu, oracle, tmp_path):
    w, h = SIZES[0]
    path = make_clip(tmp_path, "plain", w, h, n=8)
    order = ((0, 8, GAIN_A),)
    want_dng, _, _, _ = serve(gpu, path, OPTS, "dng", order=order, batch=4)
    want_half, _, _, _ = serve(gpu, path, OPTS, "rgb", order=order, batch=4)
    want_tiff, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=order, batch=4, setup=amaze())
    want_jpg, _, _, _ = serve(gpu, path, OPTS, "jpeg", FULL, order=order, batch=4, setup=amaze())
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*LOOK16) as lk16:
        m.set_demosaic("amaze")
        a = m.rgb(0, 1, batch=2)                                             # half size: the linear superpixels, as ever
        b = m.rgb(1, 2, batch=2, full=True)
        c = m.dng(3, 1, batch=2)
        d, _ = m.jpeg(4, 1, quality=QUALITY, batch=2, full=True)
        e, efl = m.dng_lossless(5, 1, batch=2)
        f, _ = m.jpeg(6, 1, quality=QUALITY, batch=2)                        # half size
        g = m.rgb(7, 1, batch=2, full=True, look16=lk16)
        s = m.rgb(7, 1, batch=2, size=(20, 10))                              # the scaled route does not know
    assert a[0].tobytes() == want_half[0] and [x.tobytes() for x in b] == want_tiff[1:3] and c[0].tobytes() == want_dng[3]
    assert d == want_jpg[4:5] and efl == [0] and len(e[0]) < len(want_dng[5])
    half = jpeg.header(w // 2, h // 2, QUALITY) + jpeg.encode(render.split_file(want_half[6], w // 2, h // 2), QUALITY)
    assert f == [half]
    check_tiffs(renderings(want_dng[7:], [GAIN_A], w, h, "full+amaze", amaze=oracle.amaze_demosaic, look16=LOOK16), [g[0].tobytes()], (w, h), "interleaved", bits=16)
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        m.dng(0, 7, batch=4)
        assert m.rgb(7, 1, batch=2, size=(20, 10)).tobytes() == s.tobytes()


def test_mount_amaze_behind_a_dual_iso_conversion(gpu, oracle, tmp_path):
    """the conversion's AMaZE and the rendering's run on one thread, batch after batch, at one geometry: each has tile planes of its own"""
    w, h = 416, 264
    path = make_clip(tmp_path, "plain", w, h, dual=True, n=3)
    opts = dict(dual_iso=2, hdr_interp=0)
    order = ((0, 3, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, opts, "dng", order=order)
    tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", FULL, order=order, setup=amaze())
    assert res_rgb == res_full == [1, 1, 1]
    check_tiffs(renderings(full, gains, w, h, "full+amaze", amaze=oracle.amaze_demosaic), tiffs, (w, h), "dual ISO")
    again, _, _, _ = serve(gpu, path, opts, "dng", order=order)
    assert again == full


def test_the_render_tool_with_amaze(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --full --demosaic amaze (its main(), in this process): TIFF, --jpeg, --bits 16 and --lut files are the mount's"""
    from PIL import Image
    tool = load_tool("mlv_render")
    w, h = SIZES[0]
    path = make_clip(tmp_path, "plain", w, h, n=3)
    order = ((0, 3, 1.5),)
    want, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=order, setup=amaze())
    want_jpg, _, _, _ = serve(gpu, path, OPTS, "jpeg", FULL, order=order, setup=amaze())
    with look.Look16(look.shaper16("srgb")) as lk16:
        want16, _, _, _ = serve(gpu, path, OPTS, "rgb", dict(FULL, look16=lk16), order=order, setup=amaze())
    cube = tmp_path / "t.cube"
    cube.write_text(lc.cube_text(3, lc.random_table(3)))
    with look.Look(look.shaper("srgb"), *look.read_cube(str(cube))) as lk:
        want_lut, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=order, setup=amaze(lk))

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--bad-pix", "1", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)

    def files(out, ext):
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.%s" % (k, ext) for k in range(3)]
        return [open(out / n, "rb").read() for n in names]

    assert run(tmp_path / "a", ["--full", "--demosaic", "amaze"]) == 0 and files(tmp_path / "a", "tif") == want
    with Image.open(tmp_path / "a" / "M07-1234_000000.tif") as im:
        assert im.mode == "RGB" and im.size == (w, h)
    assert run(tmp_path / "b", ["--full", "--demosaic", "amaze", "--jpeg", str(QUALITY)]) == 0 and files(tmp_path / "b", "jpg") == want_jpg
    assert run(tmp_path / "c", ["--full", "--demosaic", "amaze", "--bits", "16"]) == 0 and files(tmp_path / "c", "tif") == want16
    assert run(tmp_path / "d", ["--full", "--demosaic", "amaze", "--lut", str(cube)]) == 0 and files(tmp_path / "d", "tif") == want_lut
    assert want_lut != want and want16 != want
    linear, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=order)
    assert run(tmp_path / "e", ["--full"]) == 0 and files(tmp_path / "e", "tif") == linear
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run(tmp_path / "f", ["--demosaic", "amaze"])
    assert "--full" in capsys.readouterr().err


def test_mount_amaze_refusals(gpu, tmp_path):
    w, h = SIZES[0]
    path = make_clip(tmp_path, "plain", w, h, n=4)
    size = HDR + w * h * 3
    want, _, _, _ = serve(gpu, path, OPTS, "rgb", FULL, order=((0, 4, GAIN_A),), setup=amaze())
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*LOOK16) as lk16:
        m.set_demosaic("amaze")
        out = np.full(2 * size, 0xA5, np.uint8)
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), size, 256, 40, 30, 2, 0, None) == lib.ERR_ARG and b"resampled" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), size, 256, 90, 40, 30, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert gpu.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, lib.ptr(out), size, 256, 20, 10, lk16.h, 2, 0, None) == lib.ERR_ARG
        assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, size=(40, 30), resample=True)
        assert gpu.mlvfs_amd_mount_set_demosaic(m.h, 2) == lib.ERR_ARG
        assert [f.tobytes() for f in m.rgb(0, 2, batch=2, full=True)] == want[:2]      # the refusals served nothing and spoilt nothing
        m.set_demosaic("linear")
        assert m.rgb(2, 2, batch=2, size=(40, 30), resample=True).shape == (2, HDR + 3600)
        m.set_demosaic("amaze")
        assert [f.tobytes() for f in m.rgb(2, 2, batch=2, full=True)] == want[2:]
    fresh(gpu)
    r, m = open_mount(path, OPTS, proxy=2)
    with r, m:
        m.set_demosaic("amaze")
        out[:] = 0xA5
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_full(m.h, 0, 2, lib.ptr(out), size, 256, 90, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert (out == 0xA5).all()
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + (w // 2) * (h // 2) * 2)
    # 34 pixels wide: the linear filter serves the clip, AMaZE does not, and it is not served by the linear filter in silence
    d = tmp_path / "narrow"
    d.mkdir()
    frames = [synth.normal_frame(34, 40, seed=5, frame=k) for k in range(2)]
    narrow = mlvfile.write_clip(str(d / NAME), payloads(frames, "plain")[0], 34, 40)[0]
    fresh(gpu)
    r, m = open_mount(narrow, {})
    with r, m:
        nsize = HDR + 34 * 40 * 3
        linear = m.rgb(0, 2, full=True)
        assert linear.shape == (2, nsize)
        m.set_demosaic("amaze")
        assert gpu.mlvfs_amd_mount_rgb_full_size(m.h, 0) == 0 and gpu.mlvfs_amd_mount_rgb16_full_size(m.h, 0) == 0
        buf = np.full(2 * nsize, 0xA5, np.uint8)
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 2, lib.ptr(buf), nsize, 256, 2, 0, None) == lib.ERR_ARG and b"36x36" in gpu.mlvfs_amd_last_error()
        assert (buf == 0xA5).all()
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, full=True)
        assert m.rgb(0, 2).shape == (2, HDR + 17 * 20 * 3)                   # the half-size call serves it as before
        m.set_demosaic("linear")
        assert m.rgb(0, 2, full=True).tobytes() == linear.tobytes()
