"""Rendered frames at any smaller size through the mount (csrc/mount.cpp, csrc/k_scale.hip): mlvfs_amd_mount_rgb_scaled
against a full-size .dng mount of the same clip and options -- the TIFF's pixels are the definition of mlvfs_amd/scale.py applied to
the pixels of the .dng file, with the parameters the tags of that file's header give -- and mlvfs_amd_mount_jpeg_scaled against
mlvfs_amd/jpeg.py's encoding of that rendering; results[], sizes[] and flags[]; PIL opens every file at ow x oh; calls at two sizes
interleave with the half-size call and the others on one handle and leave a handle that never makes them as it was; the refusals; the
tool.  The clips, option sets and helpers are those of tests/mount_harness.py.  All comparisons are for equality."""
import io
import os

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib, mlvfile, render, scale, synth

import scale_cases as sc
from mount_harness import (GAIN_A, HDR, OPTION_SETS, QUALITY, calibration, check_jpegs, check_tiffs, fresh, load_tool, make_clip, noise_clip,
                           open_mount, payloads, renderings, run_tool, serve)

pytestmark = pytest.mark.gpu
JHDR = jpeg.HEADER_BYTES


# one payload kind -- the scaling sits behind every stage that depends on it --, both of the mount tests' frame sizes (the fast and the
# generic form), every option set, each at a size of its own: a ratio that is no integer, a thumbnail, a ratio of exactly 2, 3 a side,
# one pixel less a side
SIZES_OF = {(64, 48): [(21, 16), (7, 5), (16, 12), (32, 8), (31, 23)], (418, 266): [(140, 89), (9, 6), (104, 66), (209, 44), (208, 132)]}
CASES = [(w, h, SIZES_OF[(w, h)][k], name, opts, cal) for w, h in sc.MOUNT_SIZES for k, (name, opts, cal) in enumerate(OPTION_SETS)]


@pytest.mark.parametrize("w,h,size,name,opts,cal", CASES, ids=[f"{w}x{h}->{s[0]}x{s[1]}:{name}" for w, h, s, name, _, _ in CASES])
def test_mount_scaled_is_the_full_size_file_scaled(gpu, tmp_path, w, h, size, name, opts, cal):
    label = f"{w}x{h}->{size}:{name}"
    path = make_clip(tmp_path, "plain", w, h, dual=bool(opts.get("dual_iso")))
    with calibration(cal, w, h) as cal_args:
        full, _, res_full, _ = serve(gpu, path, opts, "dng", **cal_args)
        tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", dict(size=size), **cal_args)
        jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", dict(size=size), **cal_args)
    assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full)
    want = renderings(full, gains, w, h, "scaled", size)
    check_tiffs(want, tiffs, size, label)
    check_jpegs(want, jpgs, flags, size, label, QUALITY)
    assert len(set(tiffs)) == len(tiffs), "two frames rendered alike"


def test_mount_scaled_uses_the_x4_levels_of_a_converted_frame(gpu, tmp_path):
    """416x264, the size the dual-ISO tests convert at (and one the fast kernel takes): a mixed clip, frames 1 and 3 are not dual ISO
    and keep their levels"""
    path = make_clip(tmp_path, "plain", 416, 264, normal_at=(1, 3))
    opts = dict(dual_iso=2, hdr_interp=1, cs=2)
    order = ((0, 5, GAIN_A),)
    size = scale.fit(416, 264, 100, 100)
    assert size == (100, 63)
    full, _, res_full, _ = serve(gpu, path, opts, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", dict(size=size), order=order, batch=3)
    jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", dict(size=size), order=order, batch=3)
    assert res_full == res_rgb == res_jpg == [1, 0, 1, 0, 1]
    levels = [render.header_colour(f[:65536])[:2] for f in full]
    assert levels[0] == (4 * 2048, 4 * 15000) and levels[1] == (2048, 15000)
    want = renderings(full, gains, 416, 264, "scaled", size)
    check_tiffs(want, tiffs, size, "mixed dual ISO")
    check_jpegs(want, jpgs, flags, size, "mixed dual ISO", QUALITY)
    assert flags == [0] * 5 and all(JHDR < len(j) < len(t) for j, t in zip(jpgs, tiffs))


def test_mount_jpeg_scaled_serves_the_tiff_where_that_is_smaller(gpu, tmp_path):
    """noise at quality 100 at 13 x 11: 629 bytes of header and the stream are more than the TIFF's 685 bytes; the flat frame between
    the two noise frames stays a JPEG file"""
    w, h, size = 64, 48, (13, 11)
    path = noise_clip(tmp_path, w, h)
    order = ((0, 3, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, {}, "dng", order=order, batch=3)
    tiffs, _, res_rgb, gains = serve(gpu, path, {}, "rgb", dict(size=size), order=order, batch=3)
    files, flags, res_jpg, _ = serve(gpu, path, {}, "jpeg", dict(size=size), order=order, batch=3, quality=100)
    want = renderings(full, gains, w, h, "scaled", size)
    check_tiffs(want, tiffs, size, "noise")
    check_jpegs(want, files, flags, size, "noise", 100)
    assert flags == [1, 0, 1] and files[0] == tiffs[0] and files[2] == tiffs[2] and len(files[0]) == HDR + 13 * 11 * 3 and res_jpg == res_rgb == res_full
    assert JHDR < len(files[1]) < len(tiffs[1])
    # sizes[] as the C call reports them, and nothing behind a file is touched
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        stride = m.rgb_size(size=size) + 9
        out = np.full(3 * stride, 0xA5, np.uint8)
        sizes, fl = np.full(3, 7, np.uintp), np.full(3, 7, np.int32)
        lib.check(gpu.mlvfs_amd_mount_jpeg_scaled(m.h, 0, 3, lib.ptr(out), stride, 256, 100, size[0], size[1], lib.ptr(sizes), lib.ptr(fl), 2, 0, None),
                  "mount_jpeg_scaled")
        assert list(sizes) == [len(f) for f in files] and list(fl) == flags
        for k in range(3):
            at = k * stride
            assert out[at:at + int(sizes[k])].tobytes() == files[k] and (out[at + int(sizes[k]):at + stride] == 0xA5).all(), k


def test_scaled_calls_of_two_sizes_interleave_with_the_others(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 416, 264, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, GAIN_A),)
    A, B = (160, 101), (52, 33)
    want_dng, _, _, _ = serve(gpu, path, opts, "dng", order=order, batch=4)
    want_half, _, _, _ = serve(gpu, path, opts, "rgb", order=order, batch=4)
    want_a, _, _, gains = serve(gpu, path, opts, "rgb", dict(size=A), order=order, batch=4)
    want_b, _, _, _ = serve(gpu, path, opts, "rgb", dict(size=B), order=order, batch=4)
    jpg_b, flags, _, _ = serve(gpu, path, opts, "jpeg", dict(size=B), order=order, batch=4)
    check_tiffs(renderings(want_dng, gains, 416, 264, "scaled", A), want_a, A, "one size")
    check_tiffs(renderings(want_dng, gains, 416, 264, "scaled", B), want_b, B, "another")
    check_jpegs(renderings(want_dng, gains, 416, 264, "scaled", B), jpg_b, flags, B, "another", QUALITY)
    # the identity size is the half-size call's file
    ident, _, _, _ = serve(gpu, path, opts, "rgb", dict(size=(208, 132)), order=order, batch=4)
    assert ident == want_half
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a = m.rgb(0, 1, batch=2)                                             # half size
        b = m.rgb(1, 2, batch=2, size=A)
        c = m.dng(3, 1, batch=2)
        d, _ = m.jpeg(4, 1, quality=QUALITY, batch=2, size=B)
        e = m.rgb(5, 1, batch=2, size=B)
        f, _ = m.jpeg(6, 1, quality=QUALITY, batch=2)                        # half size
        g = m.rgb(7, 1, batch=2, size=A)
    assert a[0].tobytes() == want_half[0] and [x.tobytes() for x in b] == want_a[1:3] and c[0].tobytes() == want_dng[3]
    assert d == jpg_b[4:5] and e[0].tobytes() == want_b[5] and g[0].tobytes() == want_a[7]
    half = jpeg.header(208, 132, QUALITY) + jpeg.encode(render.split_file(want_half[6], 208, 132), QUALITY)
    assert f == [half]


def test_a_handle_without_scaled_calls_serves_what_a_fresh_one_does(gpu, tmp_path):
    """the same calls on two handles, one of which made scaled calls in between on other frames' turn: the other calls serve the same
    bytes"""
    path = make_clip(tmp_path, "plain", 64, 48, n=6)
    opts = dict(cs=5, stripes=1)

    def run(with_scaled):
        fresh(gpu)
        r, m = open_mount(path, opts)
        out = []
        with r, m:
            out.append(m.dng(0, 2, batch=2).tobytes())
            if with_scaled:
                m.rgb(0, 2, batch=2, size=(20, 15))
                m.jpeg(2, 2, batch=2, size=(5, 3))
            out.append(m.rgb(2, 2, batch=2).tobytes())
            out.append(b"".join(m.jpeg(4, 1, batch=2)[0]))
            out.append(m.rgb(4, 1, batch=2, full=True).tobytes())
            out.append(b"".join(m.dng_lossless(5, 1, batch=2)[0]))
        return out

    assert run(False) == run(True)


def test_mount_scaled_refusals_and_strides(gpu, tmp_path):
    w, h, size = 64, 48, (20, 15)
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve(gpu, path, opts, "rgb", dict(size=size), order=order)
    nbytes = HDR + 20 * 15 * 3
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        out = np.full(4 * (nbytes + 37) + 64, 0xA5, np.uint8)
        call = lambda first, count, stride, ow=20, oh=15: gpu.mlvfs_amd_mount_rgb_scaled(m.h, first, count, lib.ptr(out), stride, 256, ow, oh, 2, 0, None)
        assert call(0, 4, nbytes - 1) == lib.ERR_ARG and (out == 0xA5).all()
        for ow, oh in ((33, 24), (32, 25), (0, 15), (20, -1)):
            assert call(0, 4, 65536, ow, oh) == lib.ERR_ARG and b"scaled" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all(), (ow, oh)
        lib.check(call(0, 2, nbytes), "mount_rgb_scaled")                    # exactly the file's size
        assert [out[k * nbytes:(k + 1) * nbytes].tobytes() for k in range(2)] == want[:2] and (out[2 * nbytes:] == 0xA5).all()
        out[:] = 0xA5
        st = nbytes + 37                                          # and anything above; the bytes between the files stay
        lib.check(call(2, 2, st), "mount_rgb_scaled")
        assert [out[k * st:k * st + nbytes].tobytes() for k in range(2)] == want[2:]
        assert (out[nbytes:st] == 0xA5).all() and (out[st + nbytes:] == 0xA5).all()
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        out[:] = 0xA5
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        assert gpu.mlvfs_amd_mount_rgb_scaled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 20, 15, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_scaled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 90, 20, 15, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert b"prox" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, size=size)
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)        # the refusal served nothing and spoilt nothing


def test_mount_scaled_at_3584x1320(gpu, tmp_path):
    from PIL import Image
    w, h = sc.BIG_W, sc.BIG_H
    frames = [synth.normal_frame(w, h, seed=1, frame=k) for k in range(2)]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, payloads(frames, "plain")[0], w, h)
    opts = dict(cs=5, stripes=1)
    order = ((0, 2, GAIN_A),)
    size = scale.fit(w, h, 1280, 720)
    assert size == (1280, 471)
    full, _, _, _ = serve(gpu, path, opts, "dng", order=order)
    tiffs, _, _, gains = serve(gpu, path, opts, "rgb", dict(size=size), order=order)
    want = renderings(full, gains, w, h, "scaled", size)
    check_tiffs(want, tiffs, size, "3584x1320")
    jpgs, flags, _, _ = serve(gpu, path, opts, "jpeg", dict(size=(160, 59)), order=((0, 1, GAIN_A),), batch=1)
    check_jpegs(renderings(full[:1], gains[:1], w, h, "scaled", (160, 59)), jpgs, flags, (160, 59), "thumbnail", QUALITY)
    with Image.open(io.BytesIO(jpgs[0])) as im:
        assert im.format == "JPEG" and im.size == (160, 59)


def test_the_render_tool_scaled(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --size and --fit (its main(), in this process): the files are mlvfs_amd_mount_rgb_scaled's and
    mlvfs_amd_mount_jpeg_scaled's; the two options exclude each other and --full"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, "rgb", dict(size=(20, 15)), order=((0, 3, 1.5),))
    want_jpg, _, _, _ = serve(gpu, path, opts, "jpeg", dict(size=(16, 12)), order=((0, 3, 1.5),), quality=80)

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    out = tmp_path / "out"
    assert run(out, ["--size", "20x15"]) == 0
    names = sorted(os.listdir(out))
    assert names == ["M07-1234_%06d.tif" % k for k in range(3)]
    assert [open(out / n, "rb").read() for n in names] == want
    with Image.open(out / names[0]) as im:
        assert im.mode == "RGB" and im.size == (20, 15)
    capsys.readouterr()
    assert run(out, ["--size", "20x15"]) == 1 and "nothing is overwritten" in capsys.readouterr().err
    out2 = tmp_path / "out2"
    assert run(out2, ["--fit", "16x16", "--jpeg", "80"]) == 0                  # 32 x 24 in a box of 16 x 16: 16 x 12
    names = sorted(os.listdir(out2))
    assert names == ["M07-1234_%06d.jpg" % k for k in range(3)] and [open(out2 / n, "rb").read() for n in names] == want_jpg
    for extra in (["--size", "20x15", "--fit", "16x16"], ["--size", "20x15", "--full"], ["--fit", "16x16", "--full"], ["--size", "20"]):
        with pytest.raises(SystemExit):
            run(tmp_path / "out3", extra)
    assert not os.path.exists(tmp_path / "out3")
