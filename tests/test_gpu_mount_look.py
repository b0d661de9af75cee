"""A look through the mount (csrc/mount.cpp, csrc/k_tone_dev.h): with mlvfs_amd_mount_set_look every rendered route --
TIFF and JPEG, at half size, at full size and at a smaller size -- serves the definition of mlvfs_amd/look.py applied to the pixels of
the .dng the same options serve (for JPEG: mlvfs_amd/jpeg.py's encoding of that), on plain and LJ92 clips whose sizes take the fast
and the generic kernels; a look is set, changed and cleared between calls on one handle while the .dng calls in between serve what a
handle without a look serves; a handle that set and cleared a look serves what one that never did serves; and tools/mlv_render.py
--lut writes those files from a .cube text.  All comparisons are for equality."""
import os

import numpy as np
import pytest

from mlvfs_amd import demosaic, look, render, scale

import look_cases as lc
import render_cases as rc
from mount_harness import QUALITY, check_jpegs, check_tiffs, fresh, load_tool, make_clip, open_mount, out_size, renderings, route_args, run_tool, serve

pytestmark = pytest.mark.gpu
LOOKS = {name: (S, n, T) for name, S, n, T in lc.looks()}
OPTION_SETS = [("none", dict()), ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1))]
SIZE_OF = {(64, 48): (21, 16), (418, 266): (140, 89)}
ROUTES = ("half", "full", "scaled")                                                # scaled: size=SIZE_OF[(w, h)]


# the look of each case: every N, the edge table, the non-monotone shapers and the linear one take their turn
CASES = [(payload, w, h, name, opts) for payload in ("plain", "lj92") for w, h in rc.MOUNT_SIZES for name, opts in OPTION_SETS]
LOOK_OF_CASE = ["random17", "random33", "random65", "linear33", "random2", "random3", "edge2", "identity17"]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _ in CASES])
def test_mount_look_is_the_dng_file_rendered_with_the_look(gpu, tmp_path, k):
    payload, w, h, name, opts = CASES[k]
    lname = LOOK_OF_CASE[k]
    label = f"{payload}:{w}x{h}:{name}:{lname}"
    path = make_clip(tmp_path, payload, w, h)
    full, _, res_full, _ = serve(gpu, path, opts, "dng")
    plain_half, _, _, _ = serve(gpu, path, opts, "rgb")
    with look.Look(*LOOKS[lname]) as lk:
        set_look = lambda m: m.set_look(lk)
        for route in ROUTES:
            args, size = route_args(route, SIZE_OF[(w, h)]), out_size(route, w, h, SIZE_OF[(w, h)])
            tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", args, setup=set_look)
            jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", args, setup=set_look)
            assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full), (label, route)
            want = renderings(full, gains, w, h, route, SIZE_OF[(w, h)], look=LOOKS[lname])
            check_tiffs(want, tiffs, size, f"{label}:{route}")
            check_jpegs(want, jpgs, flags, size, f"{label}:{route}", QUALITY)
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
    check_jpegs([render.render(px[7], par[7], look=A)], j7, f7, (32, 24), "look A as JPEG", QUALITY)
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
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    T = lc.random_table(3, 4)
    cube = tmp_path / "grade.cube"
    cube.write_text(lc.cube_text(3, T))
    assert look.read_cube(cube)[1].tolist() == T.tolist()

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    for k, (shaper, extra, args) in enumerate([("srgb", [], dict()), ("linear", ["--lut-input", "linear", "--size", "20x15"], dict(size=(20, 15))),
                                               ("log2:10", ["--lut-input", "log2:10", "--full"], dict(full=True))]):
        with look.Look(look.shaper(shaper), 3, T) as lk:
            want, _, _, _ = serve(gpu, path, opts, "rgb", args, order=((0, 3, 1.5),), setup=lambda m: m.set_look(lk))
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
