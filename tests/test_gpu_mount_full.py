"""Rendered full-size sRGB frames through the mount (csrc/mount.cpp, csrc/k_demosaic.hip): mlvfs_amd_mount_rgb_full
against a full-size .dng mount of the same clip and options -- the TIFF's pixels are the definition of mlvfs_amd/demosaic.py applied to
the pixels of the .dng file, with the parameters the tags of that file's header give -- and mlvfs_amd_mount_jpeg_full against
mlvfs_amd/jpeg.py's encoding of that rendering; results[], sizes[] and flags[]; PIL opens every file at W x H; the calls interleave with
the other four on one handle and leave a handle that never makes them as it was; the refusals; a failed growth of the new buffer; the
tool.  The clips, option sets and helpers are those of tests/mount_harness.py.  All comparisons are for equality."""
import io
import os

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib, mlvfile, render, synth

import demosaic_cases as dm
from mount_harness import (GAIN_A, HDR, NAME, OPTION_SETS, PAYLOADS, QUALITY, calibration, check_jpegs, check_tiffs, fresh, load_tool, make_clip,
                           noise_clip, open_mount, payloads, renderings, run_tool, serve)

pytestmark = pytest.mark.gpu
JHDR = jpeg.HEADER_BYTES
FULL = dict(full=True)


CASES = [(p, w, h, name, opts, cal) for p in PAYLOADS for w, h in dm.MOUNT_SIZES for name, opts, cal in OPTION_SETS]


@pytest.mark.parametrize("payload,w,h,name,opts,cal", CASES, ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _, _ in CASES])
def test_mount_full_is_the_full_size_file_demosaiced(gpu, reference, tmp_path, payload, w, h, name, opts, cal):
    label = f"{payload}:{w}x{h}:{name}"
    path = make_clip(tmp_path, payload, w, h, dual=bool(opts.get("dual_iso")), reference=reference)
    with calibration(cal, w, h) as cal_args:
        full, _, res_full, _ = serve(gpu, path, opts, "dng", **cal_args)
        tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", FULL, **cal_args)
        jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", FULL, **cal_args)
    assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full)
    want = renderings(full, gains, w, h, "full")
    check_tiffs(want, tiffs, (w, h), label)
    check_jpegs(want, jpgs, flags, (w, h), label, QUALITY)
    assert flags == [0] * 5 and all(JHDR < len(j) < len(t) for j, t in zip(jpgs, tiffs))
    assert len(set(tiffs)) == len(tiffs) and len(set(jpgs)) == len(jpgs), "two frames rendered alike"


def test_mount_full_uses_the_x4_levels_of_a_converted_frame(gpu, tmp_path):
    """416x264, the size the dual-ISO tests convert at (and one the fast kernel takes): a mixed clip, frames 1 and 3 are not dual ISO
    and keep their levels"""
    path = make_clip(tmp_path, "plain", 416, 264, normal_at=(1, 3))
    opts = dict(dual_iso=2, hdr_interp=1, cs=2)
    order = ((0, 5, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, opts, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", FULL, order=order, batch=3)
    jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", FULL, order=order, batch=3)
    assert res_full == res_rgb == res_jpg == [1, 0, 1, 0, 1]
    levels = [render.header_colour(f[:65536])[:2] for f in full]
    assert levels[0] == (4 * 2048, 4 * 15000) and levels[1] == (2048, 15000)
    want = renderings(full, gains, 416, 264, "full")
    check_tiffs(want, tiffs, (416, 264), "mixed dual ISO")
    check_jpegs(want, jpgs, flags, (416, 264), "mixed dual ISO", QUALITY)


def test_mount_jpeg_full_serves_the_tiff_where_that_is_smaller(gpu, tmp_path):
    """20 x 20 of noise at quality 100: 629 bytes of header and the stream are more than the TIFF's 1456 bytes (some 1900 through the
    definition); the flat frame between the two noise frames stays a JPEG file"""
    w, h = 20, 20
    path = noise_clip(tmp_path, w, h)
    order = ((0, 3, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, {}, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve(gpu, path, {}, "rgb", FULL, order=order, batch=3)
    files, flags, res_jpg, _ = serve(gpu, path, {}, "jpeg", FULL, order=order, batch=3, quality=100)
    want = renderings(full, gains, w, h, "full")
    check_tiffs(want, tiffs, (w, h), "noise")
    check_jpegs(want, files, flags, (w, h), "noise", 100)
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


def test_full_size_calls_interleave_with_the_other_four(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 416, 264, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, GAIN_A),)
    want_dng, _, _, _ = serve(gpu, path, opts, "dng", order=order, batch=4)
    want_half, _, _, _ = serve(gpu, path, opts, "rgb", order=order, batch=4)
    want_tiff, _, _, gains = serve(gpu, path, opts, "rgb", FULL, order=order, batch=4)
    want_jpg, flags, _, _ = serve(gpu, path, opts, "jpeg", FULL, order=order, batch=4)
    px = renderings(want_dng, gains, 416, 264, "full")
    check_tiffs(px, want_tiff, (416, 264), "one kind")
    check_jpegs(px, want_jpg, flags, (416, 264), "one kind", QUALITY)
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


def test_mount_full_refusals_and_strides(gpu, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve(gpu, path, opts, "rgb", FULL, order=order)
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
    small = mlvfile.write_clip(str(d / NAME), payloads(frames, "plain")[0], 16, 3)[0]
    fresh(gpu)
    r, m = open_mount(small, {})
    with r, m:
        out[:] = 0xA5
        assert gpu.mlvfs_amd_mount_rgb_full(m.h, 0, 1, lib.ptr(out), 4096, 256, 1, 0, None) == lib.ERR_ARG and b"4x4" in gpu.mlvfs_amd_last_error()
        assert (out == 0xA5).all() and m.rgb(0, 1).shape == (1, HDR + 8 * 1 * 3)


def test_a_failed_growth_of_the_full_size_buffer(gpu, tmp_path):
    """mlvfs_amd_test_fail_next(3) fails the next growth of a device buffer: on a handle whose other buffers are large enough already
    that is the full-size one.  The call returns MLVFS_AMD_ERR_HIP and serves nothing; the next call serves correctly."""
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, "rgb", FULL, order=((0, 4, GAIN_A),))
    want_jpg, _, _, _ = serve(gpu, path, opts, "jpeg", FULL, order=((0, 4, GAIN_A),))
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


def test_mount_full_at_3584x1320(gpu, tmp_path):
    from PIL import Image
    w, h = dm.BIG_W, dm.BIG_H
    frames = [synth.normal_frame(w, h, seed=1, frame=k) for k in range(2)]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, payloads(frames, "plain")[0], w, h)
    opts = dict(cs=5, stripes=1)
    order = ((0, 2, GAIN_A),)
    full, _, _, _ = serve(gpu, path, opts, "dng", order=order)
    tiffs, _, _, gains = serve(gpu, path, opts, "rgb", FULL, order=order)
    assert len(tiffs[0]) == HDR + 3584 * 1320 * 3
    want = renderings(full, gains, w, h, "full")
    check_tiffs(want, tiffs, (w, h), "3584x1320")
    # the JPEG route at that size (its bytes are held to the definition at the smaller sizes): the header, and a file PIL decodes
    jpgs, flags, _, _ = serve(gpu, path, opts, "jpeg", FULL, order=((0, 1, GAIN_A),), batch=1)
    assert flags == [0] and jpgs[0][:JHDR] == jpeg.header(w, h, QUALITY) and JHDR < len(jpgs[0]) < len(tiffs[0])
    with Image.open(io.BytesIO(jpgs[0])) as im:
        assert im.format == "JPEG" and im.size == (w, h)
        im.load()


def test_the_render_tool_full(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --full (its main(), in this process): the files are mlvfs_amd_mount_rgb_full's and mlvfs_amd_mount_jpeg_full's"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, "rgb", FULL, order=((0, 3, 1.5),))
    want_jpg, _, _, _ = serve(gpu, path, opts, "jpeg", FULL, order=((0, 3, 1.5),), quality=80)

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
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
