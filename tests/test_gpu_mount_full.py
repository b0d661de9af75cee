"""Rendered full-size sRGB frames through the mount (csrc/mount.cpp, csrc/k_demosaic.hip): mlvfs_amd_mount_rgb_full
against a full-size .dng mount of the same clip and options -- the TIFF's pixels are the definition of mlvfs_amd/demosaic.py applied to
the pixels of the .dng file, with the parameters the tags of that file's header give -- and mlvfs_amd_mount_jpeg_full against
mlvfs_amd/jpeg.py's encoding of that rendering; results[], sizes[] and flags[]; PIL opens every file at W x H; the calls interleave with
the other four on one handle and leave a handle that never makes them as it was; the refusals; a failed growth of the new buffer; the
tool.  The clips and option sets are those of tests/test_gpu_render.py.  All comparisons are for equality."""
import io
import os

import numpy as np
import pytest

from mlvfs_amd import demosaic, jpeg, lib, mlvfile, render, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.flat import Flat

import dark_cases as dc
import demosaic_cases as dm
import flat_cases as fc
from test_gpu_render import GAIN_A, GAIN_B, NAME, OPTION_SETS, ORDER, PAYLOADS, fresh, make_clip, open_mount, serve

pytestmark = pytest.mark.gpu
HDR = render.HEADER_BYTES
JHDR = jpeg.HEADER_BYTES
QUALITY = 85


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def serve_full(gpu, path, opts, kind, dark=None, flat=None, order=ORDER, batch=2, quality=QUALITY):
    """frames 2..4, then 0..1 (at another gain), in batches of 2, through one fresh handle -> (files, flags, results, gains)"""
    fresh(gpu)
    r, m = open_mount(path, opts, dark, flat)
    files, flags, results, gains = [], [], [], []
    with r, m:
        for first, count, gain in order:
            res = np.full(count, -1, np.int32)
            if kind == "jpeg":
                a, fl = m.jpeg(first, count, gain=gain, quality=quality, batch=batch, results=res, full=True)
            else:
                a = m.rgb(first, count, gain=gain, batch=batch, results=res, full=True)
                assert a.shape == (count, m.rgb_size(full=True)) and m.rgb_size(full=True) == gpu.mlvfs_amd_mount_rgb_full_size(m.h, first)
                a, fl = [f.tobytes() for f in a], [None] * count
            files += a
            flags += fl
            results += list(res)
            gains += [gain] * count
    return files, flags, results, gains


def renderings(full, gains, w, h, lut):
    """the definition applied to every full-size .dng file"""
    out = []
    for f, gain in zip(full, gains):
        assert len(f) == 65536 + w * h * 2
        p = render.params_from_header(f[:65536], int(round(256 * gain)))
        out.append(demosaic.render(np.frombuffer(f, "<u2", offset=65536).reshape(h, w), p, lut))
    return out


def check_tiffs(want, tiffs, w, h, label):
    from PIL import Image
    assert len(want) == len(tiffs)
    for k, (px, t) in enumerate(zip(want, tiffs)):
        assert len(t) == HDR + w * h * 3, (label, k)
        got = demosaic.split_file(t, w, h)
        assert np.array_equal(got, px), f"{label} frame {k}: {(got != px).sum()} bytes are not the definition's of the full-size .dng file"
        assert t[:HDR] == render.tiff_header(w, h), (label, k)
        with Image.open(io.BytesIO(t)) as im:
            assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.asarray(im), px), (label, k)


def check_jpegs(want, files, flags, w, h, label, quality=QUALITY):
    """each file: the definition's JPEG file of the rendering, or, where that is the larger, the TIFF with flag bit 0"""
    from PIL import Image
    assert len(want) == len(files) == len(flags)
    for k, (px, j, fl) in enumerate(zip(want, files, flags)):
        file = jpeg.header(w, h, quality) + jpeg.encode(px, quality)
        tiff = render.tiff_header(w, h) + px.tobytes()
        fallback = len(file) > len(tiff)
        assert fl == int(fallback), (label, k, fl, len(file), len(tiff))
        assert j == (tiff if fallback else file), f"{label} frame {k}: not the definition's file of the rendering"
        with Image.open(io.BytesIO(j)) as im:
            assert im.format == ("TIFF" if fallback else "JPEG") and im.mode == "RGB" and im.size == (w, h)
            im.load()


CASES = [(p, w, h, name, opts, cal) for p in PAYLOADS for w, h in dm.MOUNT_SIZES for name, opts, cal in OPTION_SETS]


@pytest.mark.parametrize("payload,w,h,name,opts,cal", CASES, ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _, _ in CASES])
def test_mount_full_is_the_full_size_file_demosaiced(gpu, reference, lut, tmp_path, payload, w, h, name, opts, cal):
    label = f"{payload}:{w}x{h}:{name}"
    path = make_clip(tmp_path, payload, w, h, dual=bool(opts.get("dual_iso")), reference=reference)
    with Dark.from_plane(dc.dark_plane(w, h) if cal else np.zeros((1, 1), np.uint16), 14, synth.BLACK) as dark, \
            Flat.from_plane(fc.clip_flat(w, h) if cal else np.full((1, 1), 3000, np.uint16), 14, synth.BLACK) as flat:
        cal_args = dict(dark=dark, flat=flat) if cal else {}
        full, res_full, _ = serve(gpu, path, opts, "dng", **cal_args)
        tiffs, _, res_rgb, gains = serve_full(gpu, path, opts, "rgb", **cal_args)
        jpgs, flags, res_jpg, _ = serve_full(gpu, path, opts, "jpeg", **cal_args)
    assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full)
    want = renderings(full, gains, w, h, lut)
    check_tiffs(want, tiffs, w, h, label)
    check_jpegs(want, jpgs, flags, w, h, label)
    assert flags == [0] * 5 and all(JHDR < len(j) < len(t) for j, t in zip(jpgs, tiffs))
    assert len(set(tiffs)) == len(tiffs) and len(set(jpgs)) == len(jpgs), "two frames rendered alike"


def test_mount_full_uses_the_x4_levels_of_a_converted_frame(gpu, lut, tmp_path):
    """416x264, the size the dual-ISO tests convert at (and one the fast kernel takes): a mixed clip, frames 1 and 3 are not dual ISO
    and keep their levels"""
    from test_gpu_mount import dual_clip
    path = str(dual_clip(tmp_path, "plain", normal_at=(1, 3)) / NAME)
    opts = dict(dual_iso=2, hdr_interp=1, cs=2)
    order = ((0, 5, GAIN_A),)
    full, res_full, _ = serve(gpu, path, opts, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve_full(gpu, path, opts, "rgb", order=order, batch=3)
    jpgs, flags, res_jpg, _ = serve_full(gpu, path, opts, "jpeg", order=order, batch=3)
    assert res_full == res_rgb == res_jpg == [1, 0, 1, 0, 1]
    levels = [render.header_colour(f[:65536])[:2] for f in full]
    assert levels[0] == (4 * 2048, 4 * 15000) and levels[1] == (2048, 15000)
    want = renderings(full, gains, 416, 264, lut)
    check_tiffs(want, tiffs, 416, 264, "mixed dual ISO")
    check_jpegs(want, jpgs, flags, 416, 264, "mixed dual ISO")


def noise_clip(tmp_path, w, h, flat_at=(1,)):
    """frames of noise from black to white; those in flat_at one grey level"""
    g = np.random.default_rng(11)
    frames = [np.full((h, w), 6000, np.uint16) if k in flat_at else g.integers(synth.BLACK, 15000, (h, w)).astype(np.uint16) for k in range(3)]
    path = str(tmp_path / NAME)
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)
    return path


def test_mount_jpeg_full_serves_the_tiff_where_that_is_smaller(gpu, lut, tmp_path):
    """20 x 20 of noise at quality 100: 629 bytes of header and the stream are more than the TIFF's 1456 bytes (some 1900 through the
    definition); the flat frame between the two noise frames stays a JPEG file"""
    w, h = 20, 20
    path = noise_clip(tmp_path, w, h)
    order = ((0, 3, GAIN_A),)
    full, res_full, _ = serve(gpu, path, {}, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve_full(gpu, path, {}, "rgb", order=order, batch=3)
    files, flags, res_jpg, _ = serve_full(gpu, path, {}, "jpeg", order=order, batch=3, quality=100)
    want = renderings(full, gains, w, h, lut)
    check_tiffs(want, tiffs, w, h, "noise")
    check_jpegs(want, files, flags, w, h, "noise", quality=100)
    assert flags == [1, 0, 1] and files[0] == tiffs[0] and files[2] == tiffs[2] and len(files[0]) == HDR + 1200 and res_jpg == res_rgb == res_full
    assert JHDR < len(files[1]) < len(tiffs[1])
    # sizes[] as the C call reports them, and nothing behind a file is touched
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        size = m.rgb_size(full=True)
        out = np.full(3 * (size + 9), 0xA5, np.uint8)
        sizes, fl = np.full(3, 7, np.uintp), np.full(3, 7, np.int32)
        lib.check(gpu.mlvfs_amd_mount_jpeg_full(m.h, 0, 3, lib.ptr(out), size + 9, 256, 100, lib.ptr(sizes), lib.ptr(fl), 2, 0, None), "mount_jpeg_full")
        assert list(sizes) == [len(f) for f in files] and list(fl) == flags
        for k in range(3):
            at = k * (size + 9)
            assert out[at:at + int(sizes[k])].tobytes() == files[k] and (out[at + int(sizes[k]):at + size + 9] == 0xA5).all(), k


def test_full_size_calls_interleave_with_the_other_four(gpu, lut, tmp_path):
    path = make_clip(tmp_path, "plain", 416, 264, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, GAIN_A),)
    want_dng, _, _ = serve(gpu, path, opts, "dng", order=order, batch=4)
    want_half, _, _ = serve(gpu, path, opts, "rgb", order=order, batch=4)
    want_tiff, _, _, gains = serve_full(gpu, path, opts, "rgb", order=order, batch=4)
    want_jpg, flags, _, _ = serve_full(gpu, path, opts, "jpeg", order=order, batch=4)
    px = renderings(want_dng, gains, 416, 264, lut)
    check_tiffs(px, want_tiff, 416, 264, "one kind")
    check_jpegs(px, want_jpg, flags, 416, 264, "one kind")
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a = m.rgb(0, 1, batch=2)                                             # half size
        b = m.rgb(1, 2, batch=2, full=True)
        c = m.dng(3, 1, batch=2)
        d, _ = m.jpeg(4, 1, quality=QUALITY, batch=2, full=True)
        e, efl = m.dng_lossless(5, 1, batch=2)
        f, _ = m.jpeg(6, 1, quality=QUALITY, batch=2)                        # half size
        g = m.rgb(7, 1, batch=2, full=True)
    assert a[0].tobytes() == want_half[0] and [x.tobytes() for x in b] == want_tiff[1:3] and c[0].tobytes() == want_dng[3]
    assert d == want_jpg[4:5] and efl == [0] and len(e[0]) < len(want_dng[5]) and g[0].tobytes() == want_tiff[7]
    half = jpeg.header(208, 132, QUALITY) + jpeg.encode(render.split_file(want_half[6], 208, 132), QUALITY)
    assert f == [half]


def test_a_handle_without_full_size_calls_serves_what_a_fresh_one_does(gpu, tmp_path):
    """the same calls on two handles, one of which made full-size calls in between on other frames' turn: the other four calls serve
    the same bytes; and the full-size calls on a handle that also serves half size equal a handle's that serves nothing else"""
    path = make_clip(tmp_path, "plain", 64, 48, n=6)
    opts = dict(cs=5, stripes=1)

    def run(with_full):
        fresh(gpu)
        r, m = open_mount(path, opts)
        out = []
        with r, m:
            out.append(m.dng(0, 2, batch=2).tobytes())
            if with_full:
                m.rgb(0, 2, batch=2, full=True)
                m.jpeg(2, 2, batch=2, full=True)
            out.append(m.rgb(2, 2, batch=2).tobytes())
            out.append(b"".join(m.jpeg(4, 1, batch=2)[0]))
            out.append(b"".join(m.dng_lossless(5, 1, batch=2)[0]))
        return out

    assert run(False) == run(True)


def test_mount_full_refusals_and_strides(gpu, lut, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve_full(gpu, path, opts, "rgb", order=order)
    size = HDR + w * h * 3
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        out = np.full(4 * (size + 37) + 64, 0xA5, np.uint8)
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 4, lib.ptr(out), size - 1, 256, 2, 0, None) == lib.ERR_ARG and (out == 0xA5).all()
        lib.check(gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None), "mount_rgb_full")     # exactly the file's size
        assert [out[k * size:(k + 1) * size].tobytes() for k in range(2)] == want[:2] and (out[2 * size:] == 0xA5).all()
        out[:] = 0xA5
        st = size + 37                                            # and anything above; the bytes between the files stay
        lib.check(gpu.mlvfs_amd_mount_rgb_full(m.h, 2, 2, lib.ptr(out), st, 256, 2, 0, None), "mount_rgb_full")
        assert [out[k * st:k * st + size].tobytes() for k in range(2)] == want[2:]
        assert (out[size:st] == 0xA5).all() and (out[st + size:] == 0xA5).all()
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        out[:] = 0xA5
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_full(m.h, 0, 2, lib.ptr(out), size, 256, 90, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert b"prox" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, full=True)
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)        # the refusal served nothing and spoilt nothing
    # below 4x4: the half-size call serves the clip, the full-size call does not
    d = tmp_path / "small"
    d.mkdir()
    frames = [synth.normal_frame(16, 3, seed=5, frame=k) for k in range(2)]
    small = mlvfile.write_clip(str(d / NAME), [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], 16, 3)[0]
    fresh(gpu)
    r, m = open_mount(small, {})
    with r, m:
        out[:] = 0xA5
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 1, lib.ptr(out), 4096, 256, 1, 0, None) == lib.ERR_ARG and b"4x4" in gpu.mlvfs_amd_last_error()
        assert (out == 0xA5).all() and m.rgb(0, 1).shape == (1, HDR + 8 * 1 * 3)


def test_a_failed_growth_of_the_full_size_buffer(gpu, lut, tmp_path):
    """mlvfs_amd_test_fail_next(3) fails the next growth of a device buffer: on a handle whose other buffers are large enough already
    that is the full-size one.  The call returns MLVFS_AMD_ERR_HIP and serves nothing; the next call serves correctly."""
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve_full(gpu, path, opts, "rgb", order=((0, 4, GAIN_A),))
    want_jpg, _, _, _ = serve_full(gpu, path, opts, "jpeg", order=((0, 4, GAIN_A),))
    size = HDR + w * h * 3
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        m.rgb(0, 2, batch=2)                                                 # every other buffer has its size now
        out = np.full(2 * size, 0xA5, np.uint8)
        gpu.mlvfs_amd_test_fail_next(3)
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None) == lib.ERR_HIP
        assert b"injected" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all()
        assert [f.tobytes() for f in m.rgb(0, 2, batch=2, full=True)] == want[:2]
        # a JPEG call wants more scratch and the streams' room behind the renderings: the first of these growths fails in the same way
        gpu.mlvfs_amd_test_fail_next(3)
        with pytest.raises(lib.MlvfsAmdError):
            m.jpeg(2, 2, quality=QUALITY, batch=2, full=True)
        assert m.jpeg(2, 2, quality=QUALITY, batch=2, full=True)[0] == want_jpg[2:]
        assert [f.tobytes() for f in m.rgb(2, 2, batch=2, full=True)] == want[2:]


def test_mount_full_at_3584x1320(gpu, lut, tmp_path):
    from PIL import Image
    w, h = dm.BIG_W, dm.BIG_H
    frames = [synth.normal_frame(w, h, seed=1, frame=k) for k in range(2)]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)
    opts = dict(cs=5, stripes=1)
    order = ((0, 2, GAIN_A),)
    full, _, _ = serve(gpu, path, opts, "dng", order=order)
    tiffs, _, _, gains = serve_full(gpu, path, opts, "rgb", order=order)
    assert len(tiffs[0]) == HDR + 3584 * 1320 * 3
    want = renderings(full, gains, w, h, lut)
    check_tiffs(want, tiffs, w, h, "3584x1320")
    # the JPEG route at that size (its bytes are held to the definition at the smaller sizes): the header, and a file PIL decodes
    jpgs, flags, _, _ = serve_full(gpu, path, opts, "jpeg", order=((0, 1, GAIN_A),), batch=1)
    assert flags == [0] and jpgs[0][:JHDR] == jpeg.header(w, h, QUALITY) and JHDR < len(jpgs[0]) < len(tiffs[0])
    with Image.open(io.BytesIO(jpgs[0])) as im:
        assert im.format == "JPEG" and im.size == (w, h)
        im.load()


def test_the_render_tool_full(gpu, lut, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --full (its main(), in this process): the files are mlvfs_amd_mount_rgb_full's and mlvfs_amd_mount_jpeg_full's"""
    import importlib.util
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mlv_render_tool", os.path.join(root, "tools", "mlv_render.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve_full(gpu, path, opts, "rgb", order=((0, 3, 1.5),))
    want_jpg, _, _, _ = serve_full(gpu, path, opts, "jpeg", order=((0, 3, 1.5),), quality=80)

    def run(out, extra):
        fresh(gpu)
        monkeypatch.setattr(sys, "argv", ["mlv_render.py", path, str(out), "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
        return tool.main()

    out = tmp_path / "out"
    assert run(out, ["--full"]) == 0
    names = sorted(os.listdir(out))
    assert names == ["M07-1234_%06d.tif" % k for k in range(3)]
    assert [open(out / n, "rb").read() for n in names] == want
    with Image.open(out / names[0]) as im:
        assert im.mode == "RGB" and im.size == (64, 48)
    capsys.readouterr()
    assert run(out, ["--full"]) == 1 and "nothing is overwritten" in capsys.readouterr().err
    out2 = tmp_path / "out2"
    assert run(out2, ["--full", "--jpeg", "80"]) == 0
    names = sorted(os.listdir(out2))
    assert names == ["M07-1234_%06d.jpg" % k for k in range(3)] and [open(out2 / n, "rb").read() for n in names] == want_jpg
