"""Resampled rendered frames demosaiced by AMaZE through the mount (csrc/mount.cpp, csrc/amaze_render.cpp, csrc/k_amaze_resample.hip;
DESIGN.md 3.20): with mlvfs_amd_mount_set_resample_demosaic(1) the three resampled calls serve the definition of
mlvfs_amd/amaze_resample.py (the checker's AMaZE) applied to the pixels of the .dng file of the same clip and options, byte for byte --
TIFF, JPEG and 16-bit TIFF, with the handle's look too -- and PIL opens every file at ow x oh; results[], sizes[] and flags[]; the
linear files come back when the setter returns to 0; every kind of call interleaves on one handle; a handle that never calls the setter
serves what it served; a clip whose frames go through the dual-ISO conversion's AMaZE first; the refusals; the tool.  The helpers are
those of tests/mount_harness.py."""
import os

import numpy as np
import pytest

from mlvfs_amd import amaze_resample, lib, look, mlvfile, synth

import deep_cases as dc
import look_cases as lc
from mount_harness import (GAIN_A, GAIN_B, HDR, NAME, ORDER, QUALITY, check_jpegs, check_tiffs, fresh, load_tool, make_clip, open_mount, payloads,
                           renderings, run_tool, serve)

pytestmark = pytest.mark.gpu
OPTS = dict(cs=5, badpix=1, stripes=1)
LOOK, LOOK16 = lc.look_of("random17"), dc.look_of("random3")
# payload, frame, size: a width the fast form takes at a ratio it takes, one it does not (148 is no multiple of 8), and the fast width
# at a ratio below a half (the generic form)
CASES = [("plain", 64, 48, (48, 36)), ("lzma", 148, 40, (111, 27)), ("lj92", 64, 48, (63, 47)), ("plain", 64, 48, (30, 48))]


def resampled(size, **more):
    return dict(size=size, resample=True, **more)


def amaze(lk=None, full_demosaic=None):
    """the setup of a handle that serves AMaZE in the resampled calls, with a look and a full-size demosaic where they are given"""
    def setup(m):
        assert m.resample_demosaic == "linear"
        m.set_resample_demosaic("amaze")
        assert m.resample_demosaic == "amaze"
        if full_demosaic is not None:
            m.set_demosaic(full_demosaic)
        if lk is not None:
            m.set_look(lk)
    return setup


@pytest.mark.parametrize("payload,w,h,size", CASES, ids=lambda v: str(v))
def test_mount_serves_the_definitions_files(gpu, oracle, reference, tmp_path, payload, w, h, size):
    label = f"amaze {payload} {w}x{h}->{size}"
    path = make_clip(tmp_path, payload, w, h, reference=reference)
    full, _, res_full, _ = serve(gpu, path, OPTS, "dng")
    tiffs, _, res_rgb, gains = serve(gpu, path, OPTS, "rgb", resampled(size), setup=amaze())
    jpgs, flags, res_jpg, _ = serve(gpu, path, OPTS, "jpeg", resampled(size), setup=amaze())
    with look.Look16(*LOOK16) as lk16:
        deep, _, res_deep, _ = serve(gpu, path, OPTS, "rgb", resampled(size, look16=lk16), setup=amaze())
    assert res_rgb == res_full == res_jpg == res_deep and all(r in (0, 1) for r in res_full)
    want = renderings(full, gains, w, h, "resampled+amaze", size, oracle.amaze_demosaic)
    check_tiffs(want, tiffs, size, label)
    check_jpegs(want, jpgs, flags, size, label, QUALITY)
    check_tiffs(renderings(full, gains, w, h, "resampled+amaze", size, oracle.amaze_demosaic, look16=LOOK16), deep, size, label, bits=16)
    assert len(set(tiffs)) == len(tiffs)
    # whatever set_demosaic says
    again, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), setup=amaze(full_demosaic="amaze"))
    assert again == tiffs
    # another rendering than the linear filter's, which the same handle serves again once the setter is back at 0
    linear, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), order=ORDER)
    assert all(a != b for a, b in zip(linear, tiffs))
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        m.set_resample_demosaic("amaze")
        first = [f.tobytes() for f in m.rgb(2, 3, gain=GAIN_A, batch=2, size=size, resample=True)]
        m.set_resample_demosaic("linear")
        second = [f.tobytes() for f in m.rgb(0, 2, gain=GAIN_B, batch=2, size=size, resample=True)]
        m.set_resample_demosaic("amaze")
        third, fl = m.jpeg(0, 2, gain=GAIN_B, quality=QUALITY, batch=2, size=size, resample=True)
    assert first == tiffs[:3] and second == linear[3:] and third == jpgs[3:] and fl == flags[3:]


def test_mount_with_a_look(gpu, oracle, tmp_path):
    w, h, size = 64, 48, (48, 36)
    path = make_clip(tmp_path, "plain", w, h)
    full, _, _, _ = serve(gpu, path, OPTS, "dng")
    with look.Look(*LOOK) as lk:
        tiffs, _, _, gains = serve(gpu, path, OPTS, "rgb", resampled(size), setup=amaze(lk))
        jpgs, flags, _, _ = serve(gpu, path, OPTS, "jpeg", resampled(size), setup=amaze(lk))
    want = renderings(full, gains, w, h, "resampled+amaze", size, oracle.amaze_demosaic, look=LOOK)
    check_tiffs(want, tiffs, size, "amaze resampled with a look")
    check_jpegs(want, jpgs, flags, size, "amaze resampled with a look", QUALITY)
    plain, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), setup=amaze())
    assert all(a != b for a, b in zip(plain, tiffs))


def test_sizes_and_flags_as_the_c_call_reports_them(gpu, tmp_path):
    w, h, size = 64, 48, (48, 36)
    path = make_clip(tmp_path, "plain", w, h, n=4)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), order=order, setup=amaze())
    want_jpg, want_fl, _, _ = serve(gpu, path, OPTS, "jpeg", resampled(size), order=order, setup=amaze())
    nbytes = HDR + 48 * 36 * 3
    st = nbytes + 37
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        m.set_resample_demosaic("amaze")
        out = np.full(4 * st + 64, 0xA5, np.uint8)
        sizes, fl, res = np.full(4, 7, np.uintp), np.full(4, 7, np.int32), np.full(4, -1, np.int32)
        lib.check(gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), st, 256, 48, 36, 2, 0, lib.ptr(res)), "mount_rgb_resampled")
        assert [out[k * st:k * st + nbytes].tobytes() for k in range(2)] == want[:2]
        assert (out[nbytes:st] == 0xA5).all() and (out[st + nbytes:] == 0xA5).all() and list(res[:2]) == [0, 0]
        out[:] = 0xA5
        lib.check(gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 2, 2, lib.ptr(out), st, 256, QUALITY, 48, 36, lib.ptr(sizes), lib.ptr(fl), 2, 0, lib.ptr(res)), "mount_jpeg_resampled")
        assert list(sizes[:2]) == [len(f) for f in want_jpg[2:]] and list(fl[:2]) == want_fl[2:] and list(sizes[2:]) == [7, 7]
        for k in range(2):
            assert out[k * st:k * st + int(sizes[k])].tobytes() == want_jpg[2 + k] and (out[k * st + int(sizes[k]):(k + 1) * st] == 0xA5).all(), k
        # a failed growth of the work memory's first buffer serves nothing; the call after it serves
        gpu.mlvfs_amd_dualiso_trim()
        out[:] = 0xA5
        gpu.mlvfs_amd_test_fail_next(3)
        rc = gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 1, lib.ptr(out), st, 256, 48, 36, 1, 0, None)
        assert rc == lib.ERR_HIP and b"injected" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all()
        assert [f.tobytes() for f in m.rgb(0, 2, batch=2, size=size, resample=True)] == want[:2]


def test_every_kind_of_call_interleaves(gpu, oracle, tmp_path):
    w, h = 64, 48
    A, B = (48, 36), (64, 16)
    path = make_clip(tmp_path, "plain", w, h, n=8)
    order = ((0, 8, GAIN_A),)
    want_dng, _, _, _ = serve(gpu, path, OPTS, "dng", order=order, batch=4)
    want_half, _, _, _ = serve(gpu, path, OPTS, "rgb", order=order, batch=4)
    want_a, _, _, gains = serve(gpu, path, OPTS, "rgb", resampled(A), order=order, batch=4, setup=amaze())
    want_b, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(B), order=order, batch=4, setup=amaze())
    jpg_b, flags, _, _ = serve(gpu, path, OPTS, "jpeg", resampled(B), order=order, batch=4, setup=amaze())
    check_tiffs(renderings(want_dng, gains, w, h, "resampled+amaze", A, oracle.amaze_demosaic), want_a, A, "one size")
    check_tiffs(renderings(want_dng, gains, w, h, "resampled+amaze", B, oracle.amaze_demosaic), want_b, B, "another")
    ident, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled((w, h)), order=((0, 2, GAIN_A),), batch=2, setup=amaze())
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*LOOK16) as lk16:
        m.set_resample_demosaic("amaze")
        a = m.rgb(0, 1, batch=2)                                             # half size: the linear superpixels, as ever
        b = m.rgb(1, 2, batch=2, size=A, resample=True)
        c = m.dng(3, 1, batch=2)
        d, _ = m.jpeg(4, 1, quality=QUALITY, batch=2, size=B, resample=True)
        e = m.rgb(5, 1, batch=2, full=True)                                  # the linear full-size rendering: set_demosaic was not called
        f = m.rgb(6, 1, batch=2, size=(20, 10))                              # the scaled route does not know
        g = m.rgb(7, 1, batch=2, size=B, resample=True, look16=lk16)
        m.set_demosaic("amaze")
        i2 = [x.tobytes() for x in m.rgb(0, 2, batch=2, full=True)]          # the AMaZE full-size rendering is the identity size
    assert a[0].tobytes() == want_half[0] and [x.tobytes() for x in b] == want_a[1:3] and c[0].tobytes() == want_dng[3]
    assert d == jpg_b[4:5] and i2 == ident
    check_tiffs(renderings(want_dng[7:], [GAIN_A], w, h, "resampled+amaze", B, oracle.amaze_demosaic, look16=LOOK16), [g[0].tobytes()], B, "interleaved", bits=16)
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        m.dng(0, 5, batch=4)
        assert m.rgb(5, 1, batch=2, full=True).tobytes() == e.tobytes()
        assert m.rgb(6, 1, batch=2, size=(20, 10)).tobytes() == f.tobytes()


def test_a_handle_that_never_calls_the_setter_serves_what_it_served(gpu, tmp_path):
    """and one with the setter at 0 does too, the refusal under set_demosaic("amaze") included"""
    path = make_clip(tmp_path, "plain", 64, 48, n=6)
    size = (50, 40)

    def run(setter):
        fresh(gpu)
        r, m = open_mount(path, OPTS)
        out = []
        with r, m:
            if setter:
                m.set_resample_demosaic("amaze")
                m.set_resample_demosaic("linear")
            out.append(m.dng(0, 2, batch=2).tobytes())
            out.append(m.rgb(0, 2, batch=2, size=size, resample=True).tobytes())
            out.append(b"".join(m.jpeg(2, 2, batch=2, size=(64, 16), resample=True)[0]))
            out.append(m.rgb(4, 1, batch=2, full=True).tobytes())
            m.set_demosaic("amaze")
            with pytest.raises(lib.MlvfsAmdError):
                m.rgb(4, 1, batch=2, size=size, resample=True)
            out.append(m.rgb(5, 1, batch=2, full=True).tobytes())
        return out

    linear, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), order=((0, 2, GAIN_A),))
    a = run(False)
    assert a == run(True) and a[1] == b"".join(linear)


def test_behind_a_dual_iso_conversion(gpu, oracle, tmp_path):
    """the conversion's AMaZE and the rendering's run on one thread, batch after batch, at one geometry: each has tile planes of its own"""
    w, h, size = 416, 264, (300, 190)
    path = make_clip(tmp_path, "plain", w, h, dual=True, n=3)
    opts = dict(dual_iso=2, hdr_interp=0)
    order = ((0, 3, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, opts, "dng", order=order)
    tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", resampled(size), order=order, setup=amaze())
    assert res_rgb == res_full == [1, 1, 1]
    check_tiffs(renderings(full, gains, w, h, "resampled+amaze", size, oracle.amaze_demosaic), tiffs, size, "dual ISO")
    again, _, _, _ = serve(gpu, path, opts, "dng", order=order)
    assert again == full


def test_refusals(gpu, tmp_path):
    w, h, size = 64, 48, (48, 36)
    path = make_clip(tmp_path, "plain", w, h, n=4)
    nbytes = HDR + 48 * 36 * 3
    want, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(size), order=((0, 4, GAIN_A),), setup=amaze())
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*LOOK16) as lk16:
        for which in (2, -1, 256):
            assert gpu.mlvfs_amd_mount_set_resample_demosaic(m.h, which) == lib.ERR_ARG and b"demosaic" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_set_resample_demosaic(None, 1) == lib.ERR_ARG
        with pytest.raises(ValueError):
            m.set_resample_demosaic("bilinear")
        m.set_resample_demosaic("amaze")
        out = np.full(2 * 65536, 0xA5, np.uint8)
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        call = lambda first, count, stride, ow=48, oh=36: gpu.mlvfs_amd_mount_rgb_resampled(m.h, first, count, lib.ptr(out), stride, 256, ow, oh, 2, 0, None)
        assert call(0, 2, nbytes - 1) == lib.ERR_ARG and b"out_stride" in gpu.mlvfs_amd_last_error()
        for ow, oh in ((65, 48), (64, 49), (0, 15), (20, -1)):
            assert call(0, 2, 65536, ow, oh) == lib.ERR_ARG and b"resampled" in gpu.mlvfs_amd_last_error(), (ow, oh)
            assert gpu.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, ow, oh) == 0 and gpu.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, ow, oh) == 0
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), 65536, 0, 48, 36, 2, 0, None) == lib.ERR_ARG          # the gain
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 3, 2, lib.ptr(out), 65536, 256, 48, 36, 2, 0, None) == lib.ERR_ARG        # past the clip
        assert gpu.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 48, 36, None, 2, 0, None) == lib.ERR_ARG  # no deep look
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 0, 48, 36, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 90, 48, 36, None, lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        assert [f.tobytes() for f in m.rgb(0, 4, batch=2, size=size, resample=True)] == want      # the refusals served nothing and spoilt nothing
    fresh(gpu)
    r, m = open_mount(path, OPTS, proxy=2)
    with r, m:
        m.set_resample_demosaic("amaze")
        out[:] = 0xA5
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 48, 36, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 90, 48, 36, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
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
        nsize = HDR + 20 * 30 * 3
        linear = m.rgb(0, 2, size=(20, 30), resample=True)
        assert linear.shape == (2, nsize)
        m.set_resample_demosaic("amaze")
        assert gpu.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, 20, 30) == 0 and gpu.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, 20, 30) == 0
        buf = np.full(2 * nsize, 0xA5, np.uint8)
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(buf), nsize, 256, 20, 30, 2, 0, None) == lib.ERR_ARG and b"36x36" in gpu.mlvfs_amd_last_error()
        assert (buf == 0xA5).all()
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, size=(20, 30), resample=True)
        assert m.rgb(0, 2, full=True).shape == (2, HDR + 34 * 40 * 3)        # the linear full-size call serves it as before
        m.set_resample_demosaic("linear")
        assert m.rgb(0, 2, size=(20, 30), resample=True).tobytes() == linear.tobytes()


def test_the_render_tool(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --resample (--size | --fit) --demosaic amaze (its main(), in this process): TIFF, --jpeg, --bits 16 and --lut
    files are the mount's"""
    from PIL import Image
    tool = load_tool("mlv_render")
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=3)
    order = ((0, 3, 1.5),)
    fit = amaze_resample.fit(w, h, 60, 36)
    assert fit == (48, 36)
    want, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(fit), order=order, setup=amaze())
    want_jpg, _, _, _ = serve(gpu, path, OPTS, "jpeg", resampled(fit), order=order, quality=QUALITY, setup=amaze())
    want_size, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled((50, 40)), order=order, setup=amaze())
    with look.Look16(look.shaper16("srgb")) as lk16:
        want16, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(fit, look16=lk16), order=order, setup=amaze())
    cube = tmp_path / "t.cube"
    cube.write_text(lc.cube_text(3, lc.random_table(3)))
    with look.Look(look.shaper("srgb"), *look.read_cube(str(cube))) as lk:
        want_lut, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(fit), order=order, setup=amaze(lk))

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--bad-pix", "1", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)

    def files(out, ext):
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.%s" % (k, ext) for k in range(3)]
        return [open(out / n, "rb").read() for n in names]

    argv = ["--resample", "--fit", "60x36", "--demosaic", "amaze"]
    assert run(tmp_path / "a", argv) == 0 and files(tmp_path / "a", "tif") == want
    with Image.open(tmp_path / "a" / "M07-1234_000000.tif") as im:
        assert im.mode == "RGB" and im.size == fit
    assert run(tmp_path / "b", argv + ["--jpeg", str(QUALITY)]) == 0 and files(tmp_path / "b", "jpg") == want_jpg
    assert run(tmp_path / "c", argv + ["--bits", "16"]) == 0 and files(tmp_path / "c", "tif") == want16
    assert run(tmp_path / "d", argv + ["--lut", str(cube)]) == 0 and files(tmp_path / "d", "tif") == want_lut
    assert run(tmp_path / "e", ["--resample", "--size", "50x40", "--demosaic", "amaze"]) == 0 and files(tmp_path / "e", "tif") == want_size
    assert want_lut != want and want16 != want
    linear, _, _, _ = serve(gpu, path, OPTS, "rgb", resampled(fit), order=order)
    assert run(tmp_path / "f", ["--resample", "--fit", "60x36"]) == 0 and files(tmp_path / "f", "tif") == linear and linear != want
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run(tmp_path / "g", ["--demosaic", "amaze"])
    assert "--full" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(tmp_path / "g", ["--size", "20x10", "--demosaic", "amaze"])
    assert not os.path.exists(tmp_path / "g")
