"""What the tests of the mount's routes share (tests/test_gpu_mount*.py, test_gpu_render.py, test_gpu_jpeg.py, test_gpu_proxy.py,
test_gpu_lossless_dng.py), once each: the synthetic clips and the handles on them, the one loop that serves a clip through a fresh
handle, the table of the rendered routes with their numpy definitions, the checks of a served TIFF and JPEG file, and the loading of a
tool.  A helper module like the *_cases.py ones: no test lives here; tests/test_mount_harness.py holds the checks to what the copies
they replace asserted."""
import contextlib
import functools
import importlib.util
import io
import os
import struct
import sys

import numpy as np

from mlvfs_amd import amaze_render, amaze_resample, demosaic, jpeg, mlvfile, render, resample, scale, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "M07-1234.MLV"
W, H = 416, 264                                      # the size the dual-ISO tests convert at
HDR = render.HEADER_BYTES
GAIN_A, GAIN_B = 1.0, 2.5                            # the two calls of a serve
ORDER = ((2, 3, GAIN_A), (0, 2, GAIN_B))             # first, count, gain[, quality]
QUALITY = 85
PAYLOADS = ["plain", "lzma", "lj92"]
OPTION_SETS = [
    ("none", dict(), False),
    ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1), False),
    ("pnoise+deflicker", dict(pnoise=1, deflicker=3000), False),
    ("dual_iso=2", dict(dual_iso=2, hdr_interp=0), False),
    ("dark+flat", dict(), True),
]


# ------------------------------------------------------------------ clips and handles
def fresh(gpu):
    gpu.free_focus_pixel_maps()                     # a fresh process: no bad-pixel map yet, no dual-ISO table caches
    gpu.mlvfs_amd_dualiso_reset()


def mount_opts(opts):
    from mlvfs_amd.pipeline import MlvfsOptions
    o = MlvfsOptions(chroma_smooth=opts.get("cs", 0), fix_bad_pixels=opts.get("badpix", 0), fix_stripes=opts.get("stripes", 0),
                     dual_iso=opts.get("dual_iso", 0), fix_pattern_noise=opts.get("pnoise", 0),
                     hdr_interpolation_method=opts.get("hdr_interp", 0), hdr_no_fullres=opts.get("no_fullres", 0),
                     hdr_no_alias_map=opts.get("no_alias", 0))
    return o, opts.get("deflicker", 0), opts.get("fps1000", 0) / 1000.0


def open_mount(path, opts, dark=None, flat=None, proxy=1):
    from mlvfs_amd.mount import Mount
    opt, defl, fps = mount_opts(opts)
    r = mlvfile.MlvReader(path)
    return r, Mount(r, opt, deflicker=defl, fps=fps, basename="/" + NAME, dark=dark, flat=flat, proxy=proxy)


def payloads(frames, kind, reference=None):
    """the frames as VIDF payloads, "lj92", "lzma" or (any other kind) plain -> (payloads, the clip's video class)"""
    if kind == "lj92":
        from oracle import lj92_testenc as enc
        from test_lj92 import quadrants
        return [struct.pack("<I", f.size * 2) + enc.encode(quadrants(f), 6, 14) for f in frames], 1 | 0x100
    if kind == "lzma":
        return [reference.lzma_payload(synth.pack_bits(f).tobytes()) for f in frames], 1 | 0x80
    return [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], 1


def make_clip(tmp_path, payload, w, h, dual=False, reference=None, n=5, name=NAME, normal_at=None):
    """-> the clip's path; dual: dual-ISO frames; normal_at: a dual-ISO clip but for these frames"""
    d = tmp_path / "card"
    d.mkdir(exist_ok=True)
    normal = range(n) if not dual and normal_at is None else normal_at or ()
    frames = [synth.normal_frame(w, h, seed=9, frame=k, hot=60, cold=60) if k in normal else synth.dual_iso_frame(w, h, frame=k) for k in range(n)]
    pl, vc = payloads(frames, payload, reference)
    mlvfile.write_clip(str(d / name), pl, w, h, chunks=2, frame_space=32, shuffle=True, video_class=vc)
    return str(d / name)


def dual_clip(tmp_path, payload, reference=None, normal_at=(), n=5):
    """a W x H dual-ISO clip of any payload kind; frames in normal_at are not dual ISO -> the clip's directory"""
    make_clip(tmp_path, payload, W, H, reference=reference, n=n, normal_at=normal_at)
    return tmp_path / "card"


def noise_clip(tmp_path, w, h, n=3, flat_at=(1,), top=15000):
    """frames of noise from black to below `top`; those in flat_at one grey level"""
    g = np.random.default_rng(11)
    frames = [np.full((h, w), 6000, np.uint16) if k in flat_at else g.integers(synth.BLACK, top, (h, w)).astype(np.uint16) for k in range(n)]
    path = str(tmp_path / NAME)
    mlvfile.write_clip(path, payloads(frames, "plain")[0], w, h)
    return path


@contextlib.contextmanager
def calibration(cal, w, h):
    """the dict(dark=..., flat=...) of a `cal` case for open_mount and the serve loops, or {}"""
    if not cal:
        yield {}
        return
    import dark_cases as dc
    import flat_cases as fc
    from mlvfs_amd.dark import Dark
    from mlvfs_amd.flat import Flat
    with Dark.from_plane(dc.dark_plane(w, h), 14, synth.BLACK) as dark, Flat.from_plane(fc.clip_flat(w, h), 14, synth.BLACK) as flat:
        yield dict(dark=dark, flat=flat)


# ------------------------------------------------------------------ the routes
# keywords of Mount.rgb / Mount.jpeg (size=None: the caller's size goes there), the numpy definition.  The two AMaZE routes are served
# after set_demosaic("amaze") / set_resample_demosaic("amaze"), and their definitions take the oracle's amaze_demosaic
ROUTES = {
    "half": (dict(), render.render),
    "full": (dict(full=True), demosaic.render),
    "scaled": (dict(size=None), scale.render),
    "resampled": (dict(size=None, resample=True), resample.render),
    "full+amaze": (dict(full=True), amaze_render.render),
    "resampled+amaze": (dict(size=None, resample=True), amaze_resample.render),
}


def route_args(route, size=None):
    kw = dict(ROUTES[route][0])
    return dict(kw, size=tuple(size)) if "size" in kw else kw


def out_size(route, w, h, size=None):
    """(ow, oh) of a w x h frame: route a name in ROUTES, or the keywords themselves"""
    kw = route_args(route, size) if isinstance(route, str) else route
    return tuple(kw["size"]) if kw.get("size") else (w, h) if kw.get("full") else render.geom(w, h)


@functools.lru_cache(None)
def lut():
    return render.srgb_lut12()


def renderings(full, gains, w, h, route, size=None, amaze=None, **tone):
    """a route's definition applied to every full-size .dng file; tone: look=, look16= or nothing (the sRGB table)"""
    define = ROUTES[route][1]
    args = ((amaze,) if route.endswith("+amaze") else ()) + (tuple(size) if "size" in ROUTES[route][0] else ())
    tone = tone or dict(lut=lut())
    out = []
    for f, gain in zip(full, gains):
        assert len(f) == 65536 + w * h * 2
        p = render.params_from_header(f[:65536], int(round(256 * gain)))
        out.append(define(np.frombuffer(f, "<u2", offset=65536).reshape(h, w), p, *args, **tone))
    return out


# ------------------------------------------------------------------ the serve loop
def serve_calls(gpu, path, opts, call, order, setup=None, **mount_args):
    """`call(m, first, count, results, *rest)` for each (first, count, *rest) of the order through one fresh handle, after `setup(m)`
    -> (what the calls returned, results)"""
    fresh(gpu)
    r, m = open_mount(path, opts, **mount_args)
    got, results = [], []
    with r, m:
        if setup:
            setup(m)
        for first, count, *rest in order:
            res = np.full(count, -1, np.int32)
            got.append(call(m, first, count, res, *rest))
            results += list(res)
    return got, results


def check_rgb_call(gpu, m, first, count, a, route):
    """what every Mount.rgb call of a serve must return: (count, size), the size the C query's and the header + the samples"""
    kw = {k: v for k, v in route.items() if k != "look16"}
    deep = route.get("look16") is not None
    fh = m._reader.frame_headers(first)[1].rawi_hdr
    ow, oh = out_size(kw, fh.xRes, fh.yRes)
    kind = "_resampled" if kw.get("resample") else "_scaled" if kw.get("size") else "_full" if kw.get("full") else ""
    query = getattr(gpu, f"mlvfs_amd_mount_rgb{'16' if deep else ''}{kind}_size")
    nbytes = m.rgb_size(first, bits=16 if deep else 8, **kw)
    assert a.shape == (count, nbytes) and nbytes == query(m.h, first, *kw.get("size", ())) == HDR + 3 * (2 if deep else 1) * ow * oh, (route, a.shape)


def serve(gpu, path, opts, kind, route={}, order=ORDER, batch=2, quality=QUALITY, setup=None, **mount_args):
    """frames 2..4, then 0..1 (at another gain), in batches of 2, through one fresh handle -> (files, flags, results, gains); kind: dng,
    rgb or jpeg; route: the keywords of Mount.rgb / Mount.jpeg (route_args, plus look16= for rgb); an order entry may carry its quality"""
    def call(m, first, count, res, gain, q=quality):
        if kind == "jpeg":
            return m.jpeg(first, count, gain=gain, quality=q, batch=batch, results=res, **route)
        if kind == "dng":
            a = m.dng(first, count, batch=batch, results=res)
        else:
            a = m.rgb(first, count, gain=gain, batch=batch, results=res, **route)
            check_rgb_call(gpu, m, first, count, a, route)
        return [f.tobytes() for f in a], [None] * count

    got, results = serve_calls(gpu, path, opts, call, order, setup, **mount_args)
    return [f for a, _ in got for f in a], [f for _, fl in got for f in fl], results, [e[2] for e in order for _ in range(e[1])]


# ------------------------------------------------------------------ the checks of served files
def check_tiffs(want, files, size, label, bits=8):
    """each file is the TIFF of its rendering in `want`, which PIL opens at that size"""
    from PIL import Image
    ow, oh = size
    assert len(want) == len(files), label
    for k, (px, t) in enumerate(zip(want, files)):
        if bits == 16:
            assert t == render.tiff_header(ow, oh, 16) + np.ascontiguousarray(px, "<u2").tobytes(), f"{label} frame {k}: not the definition's 16-bit file"
        else:
            assert len(t) == HDR + ow * oh * 3, (label, k)
            got = render.split_file(t, ow, oh)
            assert np.array_equal(got, px), f"{label} frame {k}: {(got != px).sum() if got.shape == px.shape else 'all'} bytes are not the definition's of the .dng file"
            assert t[:HDR] == render.tiff_header(ow, oh), (label, k)
        with Image.open(io.BytesIO(t)) as im:
            assert im.size == (ow, oh), (label, k)
            assert bits == 16 or im.mode == "RGB" and np.array_equal(np.asarray(im), px), (label, k)


def check_jpegs(want, files, flags, size, label, quality, sampling=420):
    """each file: the definition's JPEG file of the rendering at `quality` (one, or one per file) and `sampling`, or, where that is the
    larger, the TIFF with flag bit 0"""
    from PIL import Image
    ow, oh = size
    assert len(want) == len(files) == len(flags), label
    quals = list(quality) if isinstance(quality, (list, tuple)) else [quality] * len(want)
    for k, (px, j, fl, q) in enumerate(zip(want, files, flags, quals)):
        file = jpeg.header(ow, oh, q, sampling) + jpeg.encode(px, q, None, sampling)
        tiff = render.tiff_header(ow, oh) + px.tobytes()
        fallback = len(file) > len(tiff)
        assert fl == int(fallback), (label, k, fl, len(file), len(tiff))
        assert j == (tiff if fallback else file), f"{label} frame {k}: not the definition's file of the rendering"
        assert fallback or jpeg.file_sampling(j) == sampling, (label, k)
        with Image.open(io.BytesIO(j)) as im:
            assert im.format == ("TIFF" if fallback else "JPEG") and im.mode == "RGB" and im.size == (ow, oh), (label, k)
            im.load()


# ------------------------------------------------------------------ the tools
def load_tool(name):
    """tools/<name>.py as a module"""
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def run_tool(gpu, monkeypatch, tool, argv):
    """the tool's main() in this process, on a fresh process state -> its exit status"""
    fresh(gpu)
    monkeypatch.setattr(sys, "argv", [os.path.basename(tool.__file__)] + [str(a) for a in argv])
    return tool.main()
