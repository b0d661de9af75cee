"""The 16-bit TIFF routes through the mount (csrc/mount.cpp, csrc/k_tone_dev.h): on a small synthetic clip served at the
three sizes, each file is tiff_header(..., bits=16) plus the numpy definition's samples of the frame the .dng route serves, and PIL opens
it at the right size with the samples' high bytes as pixels; 8-bit calls interleaved on the same handle are byte for byte what they are
alone, and the other way round; a look set with set_look does not change a 16-bit file; out_stride at the size and above it; every
refusal leaves the output buffer untouched; tools/mlv_render.py --bits 16 writes those files.  All comparisons are for equality."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from mlvfs_amd import lib, look, render

import deep_cases as dp
import look_cases as lc
from mount_harness import HDR, fresh, load_tool, make_clip, open_mount, out_size, route_args, run_tool, serve

pytestmark = pytest.mark.gpu
LOOKS = {name: (S, n, T) for name, S, n, T in dp.looks()}
OPTS = dict(cs=5, badpix=1, stripes=1)
SCALED = {(64, 48): (21, 16), (418, 266): (140, 89)}
ROUTES = ("half", "full", "scaled")
GAIN = 1.5


def want_files(dngs, w, h, route, lk, gain=GAIN):
    """the definition applied to every .dng file: header + samples"""
    ow, oh = out_size(route, w, h, SCALED[(w, h)])
    out = []
    for f in dngs:
        assert len(f) == 65536 + w * h * 2
        p = render.params_from_header(f[:65536], int(round(256 * gain)))
        px = np.frombuffer(f, "<u2", offset=65536).reshape(h, w)
        out.append(render.tiff_header(ow, oh, bits=16) + dp.file_bytes(dp.definition({"half": 2, "full": 1, "scaled": 0}[route], px, p, lk, (ow, oh))))
    return out


def serve_dng(gpu, path, n, opts=OPTS):
    return serve(gpu, path, opts, "dng", order=((0, n, 1.0),))[0]


@pytest.mark.parametrize("payload,w,h,name", [("plain", 64, 48, "random3"), ("lj92", 64, 48, "linear0"), ("plain", 418, 266, "srgb17"),
                                              ("plain", 418, 266, "case0")], ids=lambda v: str(v))
def test_mount_rgb16_is_the_dng_file_rendered_at_16_bits(gpu, tmp_path, payload, w, h, name):
    from PIL import Image
    path = make_clip(tmp_path, payload, w, h, n=5)
    dngs = serve_dng(gpu, path, 5)
    with look.Look16(*LOOKS[name]) as lk:
        for route in ROUTES:
            ow, oh = out_size(route, w, h, SCALED[(w, h)])
            kw = route_args(route, SCALED[(w, h)])
            fresh(gpu)
            r, m = open_mount(path, OPTS)
            with r, m:
                res = np.full(5, -1, np.int32)
                size = m.rgb_size(0, bits=16, **kw)
                assert size == HDR + 6 * ow * oh == 2 * m.rgb_size(0, **kw) - HDR
                files = [f.tobytes() for f in m.rgb(0, 5, gain=GAIN, batch=2, results=res, look16=lk, **kw)]
            assert all(v in (0, 1) for v in res)
            want = want_files(dngs, w, h, route, LOOKS[name])
            for k in range(5):
                assert len(files[k]) == size and files[k][:HDR] == want[k][:HDR], (route, k)
                assert files[k] == want[k], (route, k, int((np.frombuffer(files[k], np.uint8) != np.frombuffer(want[k], np.uint8)).sum()))
                with Image.open(io.BytesIO(files[k])) as im:
                    assert im.mode == "RGB" and im.size == (ow, oh)
                    assert np.array_equal(np.asarray(im), render.split_file16(files[k], ow, oh) >> 8), (route, k)


def test_8_bit_and_16_bit_calls_interleave_on_one_handle(gpu, tmp_path):
    """one handle: every file of a mixed sequence of calls is what a handle serves that makes only the calls of its kind -- 8-bit calls
    with a look set, which the 16-bit files do not see -- and the .dng and lossless calls in between are untouched"""
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=8)
    dngs = serve_dng(gpu, path, 8)
    A = LOOKS["random65"]
    L8 = lc.look_of("random17")
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*A) as la, look.Look16(*LOOKS["linear0"]) as lb, look.Look(*L8) as l8:
        m.set_look(l8)
        mixed = [m.rgb(0, 1, gain=GAIN, batch=2, look16=la), m.rgb(1, 1, gain=GAIN, batch=2), m.rgb(2, 1, gain=GAIN, batch=2, full=True, look16=lb),
                 m.rgb(3, 1, gain=GAIN, batch=2, full=True), m.dng(4, 1, batch=2), m.rgb(5, 1, gain=GAIN, batch=2, size=(21, 16), look16=la),
                 m.rgb(6, 1, gain=GAIN, batch=2, size=(21, 16)), m.rgb(7, 1, gain=GAIN, batch=2, look16=lb)]
        jp, _ = m.jpeg(7, 1, gain=GAIN, batch=2)
        ll, _ = m.dng_lossless(7, 1, batch=2)
    mixed = [a[0].tobytes() for a in mixed]
    # the 16-bit files: the definition, with the call's deep look and not the handle's look
    assert mixed[0] == want_files(dngs[0:1], w, h, "half", A)[0] and mixed[2] == want_files(dngs[2:3], w, h, "full", LOOKS["linear0"])[0]
    assert mixed[5] == want_files(dngs[5:6], w, h, "scaled", A)[0] and mixed[7] == want_files(dngs[7:8], w, h, "half", LOOKS["linear0"])[0]
    assert mixed[4] == dngs[4]
    # the 8-bit files: a handle that makes no 16-bit call, the same frames in the same order
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look(*L8) as l8:
        m.set_look(l8)
        m.dng(0, 1, batch=2)
        alone = [m.rgb(1, 1, gain=GAIN, batch=2), m.dng(2, 1, batch=2), m.rgb(3, 1, gain=GAIN, batch=2, full=True), m.dng(4, 2, batch=2),
                 m.rgb(6, 1, gain=GAIN, batch=2, size=(21, 16))]
        jp_alone, _ = m.jpeg(7, 1, gain=GAIN, batch=2)
        ll_alone, _ = m.dng_lossless(7, 1, batch=2)
    assert mixed[1] == alone[0][0].tobytes() and mixed[3] == alone[2][0].tobytes() and mixed[6] == alone[4][0].tobytes()
    assert jp == jp_alone and ll == ll_alone
    # and the other way round: 16-bit calls alone, with no look ever set
    fresh(gpu)
    r, m = open_mount(path, OPTS)
    with r, m, look.Look16(*A) as la:
        first = m.rgb(0, 1, gain=GAIN, batch=2, look16=la)[0].tobytes()
        m.dng(1, 4, batch=2)
        sixth = m.rgb(5, 1, gain=GAIN, batch=2, size=(21, 16), look16=la)[0].tobytes()
    assert first == mixed[0] and sixth == mixed[5]


def test_out_stride_and_the_refusals(gpu, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    dngs = serve_dng(gpu, path, 4)
    name = "random2"
    want = {route: want_files(dngs, w, h, route, LOOKS[name], gain=1.0) for route in ROUTES}
    vp = lambda a: C.c_void_p(a) if a else None
    with look.Look16(*LOOKS[name]) as lk:
        def call(m, route, first, count, buf, stride, look_h, ow=21, oh=16):
            res = np.zeros(4, np.int32)
            if route == "scaled":
                return gpu.mlvfs_amd_mount_rgb16_scaled(m.h, first, count, lib.ptr(buf), stride, 256, ow, oh, vp(look_h), 2, 0, lib.ptr(res))
            f = gpu.mlvfs_amd_mount_rgb16_full if route == "full" else gpu.mlvfs_amd_mount_rgb16
            return f(m.h, first, count, lib.ptr(buf), stride, 256, vp(look_h), 2, 0, lib.ptr(res))

        for route in ROUTES:
            size = len(want[route][0])
            for stride in (size, size + 1, size + 777):          # at the size and above it
                fresh(gpu)
                r, m = open_mount(path, OPTS)
                with r, m:
                    buf = np.full(4 * stride + 8, 0xA5, np.uint8)
                    assert call(m, route, 0, 4, buf, stride, lk.h) == 0, gpu.mlvfs_amd_last_error()
                for k in range(4):
                    assert buf[k * stride:k * stride + size].tobytes() == want[route][k], (route, stride, k)
                    assert (buf[k * stride + size:(k + 1) * stride] == 0xA5).all()
                assert (buf[4 * stride:] == 0xA5).all()
            # the refusals, on one fresh handle: each leaves the buffer untouched
            fresh(gpu)
            r, m = open_mount(path, OPTS)
            with r, m:
                buf = np.full(4 * size, 0xA5, np.uint8)
                assert call(m, route, 0, 2, buf, size, 0) == lib.ERR_ARG and b"deep look" in gpu.mlvfs_amd_last_error()      # a null deep look
                assert call(m, route, 0, 2, buf, size - 1, lk.h) == lib.ERR_ARG                                             # out_stride below the size
                assert call(m, route, 0, 2, buf, HDR + (size - HDR) // 2, lk.h) == lib.ERR_ARG                              # the 8-bit file's size
                assert call(m, route, 3, 2, buf, size, lk.h) == lib.ERR_ARG and call(m, route, -1, 1, buf, size, lk.h) == lib.ERR_ARG
                if route == "scaled":                                                                                      # a size outside the geometry
                    for ow, oh in ((0, 16), (21, 0), (33, 16), (21, 25), (-1, -1)):
                        assert call(m, route, 0, 2, buf, 4 * size, lk.h, ow, oh) == lib.ERR_ARG, (ow, oh)
                        assert gpu.mlvfs_amd_mount_rgb16_scaled_size(m.h, 0, ow, oh) == 0
                assert (buf == 0xA5).all()
                assert call(m, route, 0, 1, buf, size, lk.h) == 0 and buf[:size].tobytes() == want[route][0]                # the handle still serves
            fresh(gpu)
            r, m = open_mount(path, OPTS, proxy=2)                                                                         # a proxy handle
            with r, m:
                buf = np.full(4 * size, 0xA5, np.uint8)
                assert call(m, route, 0, 2, buf, size, lk.h) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
                assert (buf == 0xA5).all()
        assert gpu.mlvfs_amd_mount_rgb16(None, 0, 1, lib.ptr(np.zeros(8, np.uint8)), 8, 256, vp(lk.h), 2, 0, None) == lib.ERR_ARG
        assert gpu.mlvfs_amd_mount_rgb16_size(None, 0) == 0 and gpu.mlvfs_amd_mount_rgb16_full_size(None, 0) == 0


def test_the_render_tool_writes_16_bit_files(gpu, tmp_path, monkeypatch):
    """tools/mlv_render.py --bits 16 (its main(), in this process): behind a log2 curve with no table, behind the default sRGB curve with
    a 3^3 .cube table at full size, and linear at a smaller size -- the mount's files, which PIL opens; --bits 16 --jpeg is an error"""
    from PIL import Image
    tool = load_tool("mlv_render")
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=3)
    opts = dict(cs=5, stripes=1)
    dngs = serve_dng(gpu, path, 3, opts)
    T = lc.random_table(3, 4)
    cube = tmp_path / "grade.cube"
    cube.write_text(lc.cube_text(3, T))

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5", "--bits", "16"] + extra)
    for k, (lk, extra, route) in enumerate([((look.shaper16_log2(12), 0, None), ["--lut-input", "log2:12"], "half"),
                                            ((look.shaper16_srgb(), 3, T), ["--lut", str(cube), "--full"], "full"),
                                            ((look.shaper16_linear(), 0, None), ["--lut-input", "linear", "--size", "21x16"], "scaled")]):
        out = tmp_path / f"out{k}"
        assert run(out, extra) == 0
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.tif" % i for i in range(3)]
        assert [open(out / n, "rb").read() for n in names] == want_files(dngs, w, h, route, lk)
        with Image.open(out / names[0]) as im:
            assert im.mode == "RGB" and im.size == out_size(route, w, h, SCALED[(w, h)])
            im.load()
    for extra in (["--jpeg"], ["--jpeg", "80"], ["--lut-input", "gamma"]):
        with pytest.raises(SystemExit):
            run(tmp_path / "out9", extra)
    assert not os.path.exists(tmp_path / "out9")
