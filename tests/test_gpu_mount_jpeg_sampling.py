"""The mount's JPEG calls at a chroma sampling (mlvfs_amd_mount_set_jpeg_sampling; csrc/mount.cpp): every file is the
header and stream mlvfs_amd/jpeg.py gives, at the sampling set, for the numpy rendering of the route that served it -- the half-size
and the resampled route on plain and LJ92 clips, the full-size route with AMaZE --; samplings interleave on one handle and with the
other serving calls; a handle that never sets one serves 4:2:0; the TIFF is served where the JPEG file would be larger; and
tools/mlv_render.py --sampling.  All comparisons are for equality."""
import io
import os

import numpy as np
import pytest

from mlvfs_amd import amaze_render, jpeg, lib, mlvfile, render, resample, synth

from test_gpu_render import GAIN_A, GAIN_B, NAME, fresh, make_clip, open_mount, serve

pytestmark = pytest.mark.gpu
HDR = jpeg.HEADER_BYTES
TIFF = render.HEADER_BYTES
NAMES = {"4:2:0": 420, "4:2:2": 422, "4:4:4": 444}
OPTS = dict(cs=5, badpix=1, stripes=1)
ORDER = ((2, 3, GAIN_A), (0, 2, GAIN_B))
QUALITY = 85


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def serve_jpeg(gpu, path, opts, sampling, order=ORDER, batch=2, quality=QUALITY, amaze=False, **route):
    """the clip through one fresh handle at `sampling` (None: never set) -> (files, flags, results, gains)"""
    fresh(gpu)
    r, m = open_mount(path, opts)
    files, flags, results, gains = [], [], [], []
    with r, m:
        if amaze:
            m.set_demosaic("amaze")
        if sampling is not None:
            m.set_jpeg_sampling(sampling)
        for first, count, gain in order:
            res = np.full(count, -1, np.int32)
            a, fl = m.jpeg(first, count, gain=gain, quality=quality, batch=batch, results=res, **route)
            files += a
            flags += fl
            results += list(res)
            gains += [gain] * count
    return files, flags, results, gains


def raw_of(full, w, h, gains):
    """[(the frame, its rendering parameters)] of full-size .dng files"""
    out = []
    for f, gain in zip(full, gains):
        assert len(f) == 65536 + w * h * 2
        out.append((np.frombuffer(f, "<u2", offset=65536).reshape(h, w), render.params_from_header(f[:65536], int(round(256 * gain)))))
    return out


def check_files(want, files, flags, sampling, quality, label):
    """want: the numpy renderings; every file is the definition's at `sampling`, and PIL opens it at the rendering's size"""
    from PIL import Image
    assert len(want) == len(files) == len(flags)
    for k, (px, j, fl) in enumerate(zip(want, files, flags)):
        ph, pw = px.shape[:2]
        file = jpeg.header(pw, ph, quality, NAMES[sampling]) + jpeg.encode(px, quality, None, NAMES[sampling])
        assert len(file) <= TIFF + 3 * pw * ph and fl == 0, (label, k)
        assert j == file, f"{label} frame {k}: not the definition's {sampling} file of the route's rendering"
        assert jpeg.file_sampling(j) == NAMES[sampling]
        with Image.open(io.BytesIO(j)) as im:
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == (pw, ph)
            im.load()


CASES = [(p, w, h, size) for p in ("plain", "lj92") for (w, h), size in (((64, 48), (33, 25)), ((418, 266), (280, 178)))]


@pytest.mark.parametrize("payload,w,h,size", CASES, ids=[f"{p}:{w}x{h}" for p, w, h, _ in CASES])
def test_half_size_and_resampled_files_at_both_samplings(gpu, lut, tmp_path, payload, w, h, size):
    path = make_clip(tmp_path, payload, w, h)
    full, res_full, gains = serve(gpu, path, OPTS, "dng")
    raws = raw_of(full, w, h, gains)
    half = [render.render(f, p, lut) for f, p in raws]
    resampled = [resample.render(f, p, size[0], size[1], lut) for f, p in raws]
    for sampling in ("4:2:2", "4:4:4"):
        files, flags, res, _ = serve_jpeg(gpu, path, OPTS, sampling)
        assert res == res_full
        check_files(half, files, flags, sampling, QUALITY, f"{payload}:{w}x{h} half {sampling}")
        assert len(set(files)) == len(files), "two frames encoded alike"
        files, flags, res, _ = serve_jpeg(gpu, path, OPTS, sampling, size=size, resample=True)
        assert res == res_full
        check_files(resampled, files, flags, sampling, QUALITY, f"{payload}:{w}x{h} resampled {sampling}")


def test_full_size_amaze_files_at_both_samplings(gpu, oracle, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h)
    full, res_full, gains = serve(gpu, path, OPTS, "dng")
    want = [amaze_render.render(f, p, oracle.amaze_demosaic) for f, p in raw_of(full, w, h, gains)]
    for sampling in ("4:2:2", "4:4:4"):
        files, flags, res, _ = serve_jpeg(gpu, path, OPTS, sampling, amaze=True, full=True)
        assert res == res_full
        check_files(want, files, flags, sampling, QUALITY, f"amaze {sampling}")


def test_samplings_interleave_on_one_handle_and_with_rgb_and_dng(gpu, lut, tmp_path):
    w, h, q = 416, 264, 75
    path = make_clip(tmp_path, "plain", w, h, n=8)
    order = ((0, 8, GAIN_A),)
    full, _, gains = serve(gpu, path, OPTS, "dng", order=order, batch=4)
    want_rgb, _, _ = serve(gpu, path, OPTS, "rgb", order=order, batch=4)
    raws = raw_of(full, w, h, gains)
    half = [render.render(f, p, lut) for f, p in raws]
    size = (300, 190)
    file = lambda px, s: jpeg.header(px.shape[1], px.shape[0], q, s) + jpeg.encode(px, q, None, s)
    # a handle that never calls the setter: the files of the call as it was, which are the definition's without a sampling
    never, flags, _, _ = serve_jpeg(gpu, path, OPTS, None, order=order, batch=4, quality=q)
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
    assert d == [file(resample.render(*raws[4], size[0], size[1], lut), 422)]
    assert f == never[6:7]
    assert g == [file(resample.render(*raws[7], size[0], size[1], lut), 444)]


def noise_clip(tmp_path, w, h, n=2):
    rng = np.random.default_rng(11)
    frames = [rng.integers(synth.BLACK, synth.WHITE + 1, (h, w)).astype(np.uint16) for _ in range(n)]
    path = str(tmp_path / NAME)
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)
    return path


def test_the_tiff_is_served_where_the_444_file_would_be_larger(gpu, tmp_path):
    """noise at quality 100: the definition's 4:4:4 stream does not fit beside 629 bytes of header in the TIFF's 256 + 3 W' H', so the
    TIFF is served with flag bit 0; every sampling follows the one rule"""
    w, h, q = 64, 48, 100
    path = noise_clip(tmp_path, w, h)
    order = ((0, 2, GAIN_A),)
    tiffs, _, _ = serve(gpu, path, {}, "rgb", order=order)
    pw, ph = render.geom(w, h)
    pixels = [render.split_file(t, pw, ph) for t in tiffs]
    for sampling, code in NAMES.items():
        streams = [jpeg.encode(px, q, None, code) for px in pixels]
        larger = [HDR + len(s) > len(t) for s, t in zip(streams, tiffs)]
        if code == 444:
            assert larger == [True, True], "the case does not reach the rule: " + str([len(s) for s in streams])
        files, flags, _, _ = serve_jpeg(gpu, path, {}, sampling, order=order, quality=q)
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
    import importlib.util
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mlv_render_tool", os.path.join(root, "tools", "mlv_render.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)

    def run(out, extra):
        fresh(gpu)
        monkeypatch.setattr(sys, "argv", ["mlv_render.py", path, str(out), "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
        return tool.main()

    names = ["M07-1234_%06d.jpg" % k for k in range(3)]
    for arg, sampling in (("444", "4:4:4"), ("422", "4:2:2"), ("420", "4:2:0")):
        want, flags, _, _ = serve_jpeg(gpu, path, opts, sampling, order=((0, 3, 1.5),), quality=80)
        out = tmp_path / ("out" + arg)
        assert run(out, ["--jpeg", "80", "--sampling", arg]) == 0 and flags == [0, 0, 0]
        assert sorted(os.listdir(out)) == names and [open(out / n, "rb").read() for n in names] == want
        for n in names:
            with Image.open(out / n) as im:
                assert im.format == "JPEG" and im.mode == "RGB" and im.size == (32, 24)
                im.load()
            assert jpeg.file_sampling(open(out / n, "rb").read()) == NAMES[sampling]
    plain, _, _, _ = serve_jpeg(gpu, path, opts, None, order=((0, 3, 1.5),), quality=80)
    assert run(tmp_path / "plain", ["--jpeg", "80"]) == 0 and [open(tmp_path / "plain" / n, "rb").read() for n in names] == plain == want
    capsys.readouterr()
    with pytest.raises(SystemExit):
        run(tmp_path / "none", ["--sampling", "444"])
    assert "--sampling takes --jpeg" in capsys.readouterr().err
