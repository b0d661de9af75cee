"""A look through the mount (csrc/mount.cpp, csrc/k_tone_dev.h): with mlvfs_amd_mount_set_look every rendered route --
TIFF and JPEG, at half size, at full size and at a smaller size -- serves the definition of mlvfs_amd/look.py applied to the pixels of
the .dng the same options serve (for JPEG: mlvfs_amd/jpeg.py's encoding of that), on plain and LJ92 clips whose sizes take the fast
and the generic kernels; a look is set, changed and cleared between calls on one handle while the .dng calls in between serve what a
handle without a look serves; a handle that set and cleared a look serves what one that never did serves; and tools/mlv_render.py
--lut writes those files from a .cube text.  All comparisons are for equality."""
import io
import os

import numpy as np
import pytest

from mlvfs_amd import demosaic, jpeg, look, render, scale

import look_cases as lc
import render_cases as rc
from test_gpu_render import ORDER, fresh, make_clip, open_mount, serve

pytestmark = pytest.mark.gpu
HDR = render.HEADER_BYTES
QUALITY = 85
LOOKS = {name: (S, n, T) for name, S, n, T in lc.looks()}
OPTION_SETS = [("none", dict()), ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1))]
SIZE_OF = {(64, 48): (21, 16), (418, 266): (140, 89)}
ROUTES = [("half", dict()), ("full", dict(full=True)), ("scaled", None)]           # scaled: size=SIZE_OF[(w, h)]


def route_args(route, w, h):
    return dict(size=SIZE_OF[(w, h)]) if route == "scaled" else dict(ROUTES)[route]


def out_size(route, w, h):
    return (w // 2, h // 2) if route == "half" else (w, h) if route == "full" else SIZE_OF[(w, h)]


def serve_look(gpu, path, opts, kind, args, lk, order=ORDER, batch=2):
    """frames 2..4, then 0..1 (at another gain), in batches of 2, through one fresh handle with the look set -> (files, flags, results, gains)"""
    fresh(gpu)
    r, m = open_mount(path, opts)
    files, flags, results, gains = [], [], [], []
    with r, m:
        m.set_look(lk)
        for first, count, gain in order:
            res = np.full(count, -1, np.int32)
            if kind == "jpeg":
                a, fl = m.jpeg(first, count, gain=gain, quality=QUALITY, batch=batch, results=res, **args)
            else:
                a = m.rgb(first, count, gain=gain, batch=batch, results=res, **args)
                a, fl = [f.tobytes() for f in a], [None] * count
            files += a
            flags += fl
            results += list(res)
            gains += [gain] * count
    return files, flags, results, gains


def renderings(full, gains, w, h, route, lk):
    """the definition, with the look, applied to every full-size .dng file"""
    out = []
    for f, gain in zip(full, gains):
        assert len(f) == 65536 + w * h * 2
        p = render.params_from_header(f[:65536], int(round(256 * gain)))
        px = np.frombuffer(f, "<u2", offset=65536).reshape(h, w)
        if route == "half":
            out.append(render.render(px, p, look=lk))
        elif route == "full":
            out.append(demosaic.render(px, p, look=lk))
        else:
            out.append(scale.render(px, p, *SIZE_OF[(w, h)], look=lk))
    return out


def check_tiffs(want, tiffs, size, label):
    from PIL import Image
    ow, oh = size
    assert len(want) == len(tiffs)
    for k, (px, t) in enumerate(zip(want, tiffs)):
        assert len(t) == HDR + ow * oh * 3, (label, k)
        got = render.split_file(t, ow, oh)
        assert np.array_equal(got, px), f"{label} frame {k}: {(got != px).sum()} bytes are not the definition's of the .dng file with the look"
        assert t[:HDR] == render.tiff_header(ow, oh), (label, k)
        with Image.open(io.BytesIO(t)) as im:
            assert im.mode == "RGB" and im.size == (ow, oh) and np.array_equal(np.asarray(im), px), (label, k)


def check_jpegs(want, files, flags, size, label, quality=QUALITY):
    """each file: the definition's JPEG file of the rendering, or, where that is the larger, the TIFF with flag bit 0"""
    from PIL import Image
    ow, oh = size
    assert len(want) == len(files) == len(flags)
    for k, (px, j, fl) in enumerate(zip(want, files, flags)):
        file = jpeg.header(ow, oh, quality) + jpeg.encode(px, quality)
        tiff = render.tiff_header(ow, oh) + px.tobytes()
        fallback = len(file) > len(tiff)
        assert fl == int(fallback), (label, k, fl, len(file), len(tiff))
        assert j == (tiff if fallback else file), f"{label} frame {k}: not the definition's file of the rendering with the look"
        with Image.open(io.BytesIO(j)) as im:
            assert im.format == ("TIFF" if fallback else "JPEG") and im.mode == "RGB" and im.size == (ow, oh)
            im.load()


# the look of each case: every N, the edge table, the non-monotone shapers and the linear one take their turn
CASES = [(payload, w, h, name, opts) for payload in ("plain", "lj92") for w, h in rc.MOUNT_SIZES for name, opts in OPTION_SETS]
LOOK_OF_CASE = ["random17", "random33", "random65", "linear33", "random2", "random3", "edge2", "identity17"]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _ in CASES])
def test_mount_look_is_the_dng_file_rendered_with_the_look(gpu, tmp_path, k):
    payload, w, h, name, opts = CASES[k]
    lname = LOOK_OF_CASE[k]
    label = f"{payload}:{w}x{h}:{name}:{lname}"
    path = make_clip(tmp_path, payload, w, h)
    full, res_full, _ = serve(gpu, path, opts, "dng")
    plain_half, _, _ = serve(gpu, path, opts, "rgb")
    with look.Look(*LOOKS[lname]) as lk:
        for route, _ in ROUTES:
            args, size = route_args(route, w, h), out_size(route, w, h)
            tiffs, _, res_rgb, gains = serve_look(gpu, path, opts, "rgb", args, lk)
            jpgs, flags, res_jpg, _ = serve_look(gpu, path, opts, "jpeg", args, lk)
            assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full), (label, route)
            want = renderings(full, gains, w, h, route, LOOKS[lname])
            check_tiffs(want, tiffs, size, f"{label}:{route}")
            check_jpegs(want, jpgs, flags, size, f"{label}:{route}")
            if route == "half":                                  # the look did something, unless it is the identity
                assert (tiffs == plain_half) == (lname == "identity17"), label


def test_a_look_is_set_changed_and_cleared_between_calls(gpu, tmp_path):
    """one handle: .dng, look A, .dng, look B on another route, cleared, look A as JPEG -- every file is what a handle serves that makes
    the same calls with the looks applied on the host, and the .dng files are a look-free handle's"""
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=8)
    opts = dict(cs=5, stripes=1)
    A, B = LOOKS["random17"], LOOKS["linear33"]
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        want_dng = [f.tobytes() for f in m.dng(0, 8, batch=2)]
    px = [np.frombuffer(f, "<u2", offset=65536).reshape(h, w) for f in want_dng]
    par = [render.params_from_header(f[:65536], 256) for f in want_dng]
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m, look.Look(*A) as la, look.Look(*B) as lb:
        d0 = m.dng(0, 1, batch=2)
        m.set_look(la)
        a1 = m.rgb(1, 1, batch=2)                                # look A, half size
        d2 = m.dng(2, 1, batch=2)                                # the .dng route never sees it
        m.set_look(lb)                                           # changed, after frames were served
        b3 = m.rgb(3, 1, batch=2, full=True)
        b4 = m.rgb(4, 1, batch=2, size=(21, 16))
        m.set_look(None)                                         # cleared
        p5 = m.rgb(5, 1, batch=2)
        ll6, _ = m.dng_lossless(6, 1, batch=2)
        m.set_look(la)
        j7, f7 = m.jpeg(7, 1, quality=QUALITY, batch=2)
    assert d0[0].tobytes() == want_dng[0] and d2[0].tobytes() == want_dng[2]
    assert np.array_equal(render.split_file(a1[0].tobytes(), 32, 24), render.render(px[1], par[1], look=A))
    assert np.array_equal(render.split_file(b3[0].tobytes(), w, h), demosaic.render(px[3], par[3], look=B))
    assert np.array_equal(render.split_file(b4[0].tobytes(), 21, 16), scale.render(px[4], par[4], 21, 16, look=B))
    assert np.array_equal(render.split_file(p5[0].tobytes(), 32, 24), render.render(px[5], par[5]))
    check_jpegs([render.render(px[7], par[7], look=A)], j7, f7, (32, 24), "look A as JPEG")
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        m.dng(0, 6, batch=2)
        assert m.dng_lossless(6, 1, batch=2)[0] == ll6           # nor does the lossless route


def test_a_handle_that_set_and_cleared_a_look_serves_what_one_without_serves(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 64, 48, n=6)
    opts = dict(cs=5, stripes=1)

    def run(with_look):
        fresh(gpu)
        r, m = open_mount(path, opts)
        out = []
        with r, m, look.Look(*LOOKS["random33"]) as lk:
            out.append(m.dng(0, 2, batch=2).tobytes())
            if with_look:
                m.set_look(lk)
                m.set_look(None)
            out.append(m.rgb(2, 2, batch=2).tobytes())
            out.append(b"".join(m.jpeg(4, 1, batch=2)[0]))
            out.append(m.rgb(4, 1, batch=2, full=True).tobytes())
            out.append(m.rgb(5, 1, batch=2, size=(20, 15)).tobytes())
            out.append(b"".join(m.dng_lossless(5, 1, batch=2)[0]))
        return out

    assert run(False) == run(True)


def test_the_render_tool_takes_a_cube_file(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --lut (its main(), in this process) on a 3^3 .cube text: the files are the mount's with that look, behind
    each of the three shapers"""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mlv_render_tool", os.path.join(root, "tools", "mlv_render.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    T = lc.random_table(3, 4)
    cube = tmp_path / "grade.cube"
    cube.write_text(lc.cube_text(3, T))
    assert look.read_cube(cube)[1].tolist() == T.tolist()

    def run(out, extra):
        fresh(gpu)
        monkeypatch.setattr(sys, "argv", ["mlv_render.py", path, str(out), "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
        return tool.main()

    for k, (shaper, extra, args) in enumerate([("srgb", [], dict()), ("linear", ["--lut-input", "linear", "--size", "20x15"], dict(size=(20, 15))),
                                               ("log2:10", ["--lut-input", "log2:10", "--full"], dict(full=True))]):
        with look.Look(look.shaper(shaper), 3, T) as lk:
            want, _, _, _ = serve_look(gpu, path, opts, "rgb", args, lk, order=((0, 3, 1.5),))
        out = tmp_path / f"out{k}"
        assert run(out, ["--lut", str(cube)] + extra) == 0
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.tif" % i for i in range(3)] and [open(out / n, "rb").read() for n in names] == want
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        plain = [f.tobytes() for f in m.rgb(0, 3, gain=1.5, batch=2)]
    assert [open(tmp_path / "out0" / n, "rb").read() for n in sorted(os.listdir(tmp_path / "out0"))] != plain
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_1D_SIZE 2\n0 0 0\n1 1 1\n")
    for extra in (["--lut", str(bad)], ["--lut", str(tmp_path / "none.cube")], ["--lut", str(cube), "--lut-input", "gamma"]):
        with pytest.raises(SystemExit):
            run(tmp_path / "out9", extra)
    assert not os.path.exists(tmp_path / "out9")
