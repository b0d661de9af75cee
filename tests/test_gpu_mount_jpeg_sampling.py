"""The mount's JPEG calls at a chroma sampling (mlvfs_amd_mount_set_jpeg_sampling; csrc/mount.cpp): every file is the
header and stream mlvfs_amd/jpeg.py gives, at the sampling set, for the numpy rendering of the route that served it -- the half-size
and the resampled route on plain and LJ92 clips, the full-size route with AMaZE --; samplings interleave on one handle and with the
other serving calls; a handle that never sets one serves 4:2:0; the TIFF is served where the JPEG file would be larger; and
tools/mlv_render.py --sampling.  All comparisons are for equality."""
import os

import pytest

from mlvfs_amd import jpeg, lib, render, synth

from mount_harness import GAIN_A, HDR as TIFF, QUALITY, check_jpegs, fresh, load_tool, make_clip, noise_clip, open_mount, renderings, run_tool, serve

pytestmark = pytest.mark.gpu
HDR = jpeg.HEADER_BYTES
NAMES = {"4:2:0": 420, "4:2:2": 422, "4:4:4": 444}
OPTS = dict(cs=5, badpix=1, stripes=1)


def sampled(sampling, amaze=False):
    """the setup of a handle that serves JPEG files at `sampling` (None: never set)"""
    def setup(m):
        if amaze:
            m.set_demosaic("amaze")
        if sampling is not None:
            m.set_jpeg_sampling(sampling)
    return setup


def check_files(want, files, flags, size, sampling, quality, label):
    """every file is the definition's at `sampling`, which PIL opens at the rendering's size, and none is the TIFF"""
    check_jpegs(want, files, flags, size, label, quality, NAMES[sampling])
    assert flags == [0] * len(files) and all(len(j) <= TIFF + 3 * size[0] * size[1] for j in files), label


CASES = [(p, w, h, size) for p in ("plain", "lj92") for (w, h), size in (((64, 48), (33, 25)), ((418, 266), (280, 178)))]


@pytest.mark.parametrize("payload,w,h,size", CASES, ids=[f"{p}:{w}x{h}" for p, w, h, _ in CASES])
def test_half_size_and_resampled_files_at_both_samplings(gpu, tmp_path, payload, w, h, size):
    path = make_clip(tmp_path, payload, w, h)
    full, _, res_full, gains = serve(gpu, path, OPTS, "dng")
    half = renderings(full, gains, w, h, "half")
    resampled = renderings(full, gains, w, h, "resampled", size)
    for sampling in ("4:2:2", "4:4:4"):
        files, flags, res, _ = serve(gpu, path, OPTS, "jpeg", setup=sampled(sampling))
        assert res == res_full
        check_files(half, files, flags, render.geom(w, h), sampling, QUALITY, f"{payload}:{w}x{h} half {sampling}")
        assert len(set(files)) == len(files), "two frames encoded alike"
        files, flags, res, _ = serve(gpu, path, OPTS, "jpeg", dict(size=size, resample=True), setup=sampled(sampling))
        assert res == res_full
        check_files(resampled, files, flags, size, sampling, QUALITY, f"{payload}:{w}x{h} resampled {sampling}")


def test_full_size_amaze_files_at_both_samplings(gpu, oracle, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h)
    full, _, res_full, gains = serve(gpu, path, OPTS, "dng")
    want = renderings(full, gains, w, h, "full+amaze", amaze=oracle.amaze_demosaic)
    for sampling in ("4:2:2", "4:4:4"):
        files, flags, res, _ = serve(gpu, path, OPTS, "jpeg", dict(full=True), setup=sampled(sampling, amaze=True))
        assert res == res_full
        check_files(want, files, flags, (w, h), sampling, QUALITY, f"amaze {sampling}")


def test_samplings_interleave_on_one_handle_and_with_rgb_and_dng(gpu, tmp_path):
    w, h, q = 416, 264, 75
    path = make_clip(tmp_path, "plain", w, h, n=8)
    order = ((0, 8, GAIN_A),)
    full, _, _, gains = serve(gpu, path, OPTS, "dng", order=order, batch=4)
    want_rgb, _, _, _ = serve(gpu, path, OPTS, "rgb", order=order, batch=4)
    half = renderings(full, gains, w, h, "half")
    size = (300, 190)
    resampled = {k: renderings(full[k:k + 1], gains[k:k + 1], w, h, "resampled", size)[0] for k in (4, 7)}
    file = lambda px, s: jpeg.header(px.shape[1], px.shape[0], q, s) + jpeg.encode(px, q, None, s)
    # a handle that never calls the setter: the files of the call as it was, which are the definition's without a sampling
    never, flags, _, _ = serve(gpu, path, OPTS, "jpeg", order=order, batch=4, quality=q)
    assert flags == [0] * 8 and never == [jpeg.header(w // 2, h // 2, q) + jpeg.encode(px, q) for px in half]
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m:
        assert m.jpeg_sampling == "4:2:0"
        a, fa = m.jpeg(0, 2, quality=q, batch=2, sampling="4:4:4")
        b, fb = m.jpeg(2, 1, quality=q, batch=2, sampling="4:2:2")
        c = m.dng(3, 1, batch=2)
        d, fd = m.jpeg(4, 1, quality=q, batch=2, size=size, resample=True)          # 4:2:2 stays set
        e = m.rgb(5, 1, batch=2)
        assert m.jpeg_sampling == "4:2:2"
        f, ff = m.jpeg(6, 1, quality=q, batch=2, sampling="4:2:0")
        g, fg = m.jpeg(7, 1, quality=q, batch=2, sampling="4:4:4", size=size, resample=True)
    assert fa + fb + fd + ff + fg == [0] * 6
    assert a == [file(px, 444) for px in half[:2]] and b == [file(half[2], 422)]
    assert c[0].tobytes() == full[3] and e[0].tobytes() == want_rgb[5]
    assert d == [file(resampled[4], 422)]
    assert f == never[6:7]
    assert g == [file(resampled[7], 444)]


def test_the_tiff_is_served_where_the_444_file_would_be_larger(gpu, tmp_path):
    """noise at quality 100: the definition's 4:4:4 stream does not fit beside 629 bytes of header in the TIFF's 256 + 3 W' H', so the
    TIFF is served with flag bit 0; every sampling follows the one rule"""
    w, h, q = 64, 48, 100
    path = noise_clip(tmp_path, w, h, n=2, flat_at=(), top=synth.WHITE + 1)
    order = ((0, 2, GAIN_A),)
    tiffs, _, _, _ = serve(gpu, path, {}, "rgb", order=order)
    pw, ph = render.geom(w, h)
    pixels = [render.split_file(t, pw, ph) for t in tiffs]
    for sampling, code in NAMES.items():
        streams = [jpeg.encode(px, q, None, code) for px in pixels]
        larger = [HDR + len(s) > len(t) for s, t in zip(streams, tiffs)]
        if code == 444:
            assert larger == [True, True], "the case does not reach the rule: " + str([len(s) for s in streams])
        files, flags, _, _ = serve(gpu, path, {}, "jpeg", order=order, quality=q, setup=sampled(sampling))
        assert flags == [int(x) for x in larger], sampling
        for k in range(2):
            assert files[k] == (tiffs[k] if larger[k] else jpeg.header(pw, ph, q, code) + streams[k]), (sampling, k)


def test_set_jpeg_sampling_refusals(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 64, 48, n=2)
    assert gpu.mlvfs_amd_mount_set_jpeg_sampling(None, 0) == lib.ERR_ARG
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        want, _ = m.jpeg(0, 1, batch=2, sampling="4:2:2")
        for bad in (-1, 3, 422, 444):
            assert gpu.mlvfs_amd_mount_set_jpeg_sampling(m.h, bad) == lib.ERR_ARG and b"sampling" in gpu.mlvfs_amd_last_error()
        with pytest.raises(ValueError):
            m.set_jpeg_sampling("4:1:1")
        with pytest.raises(ValueError):
            m.jpeg(0, 1, sampling=444)
        assert m.jpeg_sampling == "4:2:2" and m.jpeg(0, 1, batch=2)[0] == want, "a refused value changed the handle"
        assert jpeg.file_sampling(want[0]) == 422


def test_the_render_tool_takes_a_sampling(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --jpeg Q --sampling (its main(), in this process): the files are the mount's at that sampling, and PIL opens them"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    names = ["M07-1234_%06d.jpg" % k for k in range(3)]
    for arg, sampling in (("444", "4:4:4"), ("422", "4:2:2"), ("420", "4:2:0")):
        want, flags, _, _ = serve(gpu, path, opts, "jpeg", order=((0, 3, 1.5),), quality=80, setup=sampled(sampling))
        out = tmp_path / ("out" + arg)
        assert run(out, ["--jpeg", "80", "--sampling", arg]) == 0 and flags == [0, 0, 0]
        assert sorted(os.listdir(out)) == names and [open(out / n, "rb").read() for n in names] == want
        for n in names:
            with Image.open(out / n) as im:
                assert im.format == "JPEG" and im.mode == "RGB" and im.size == (32, 24)
                im.load()
            assert jpeg.file_sampling(open(out / n, "rb").read()) == NAMES[sampling]
    plain, _, _, _ = serve(gpu, path, opts, "jpeg", order=((0, 3, 1.5),), quality=80)
    assert run(tmp_path / "plain", ["--jpeg", "80"]) == 0 and [open(tmp_path / "plain" / n, "rb").read() for n in names] == plain == want
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run(tmp_path / "none", ["--sampling", "444"])
    assert "--sampling takes --jpeg" in capsys.readouterr().err
