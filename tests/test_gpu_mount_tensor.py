"""The tensor route through the mount (csrc/mount.cpp, csrc/k_tensor.hip).  An RGB tensor equals the definition
(mlvfs_amd/tensor.py) applied to the pixel bytes of the file the host route serves for the same arguments -- half, full, scaled, resampled,
full with AMaZE, with a look, with a deep look -- on plain and LJ92 clips with no option, cs5 + bad pixels + stripes, dual_iso = 2 on a
mixed clip, and a dark frame + a flat field; results[] are equal.  A Bayer tensor equals the definition applied to the pixels of the .dng
the same options serve, with that file's header levels.  Tensor and file calls interleave on one handle; out= takes a frame stride; the
refusals leave the destination untouched; one 3584x1320 frame at half and full size; tools/mlv_tensor.py writes the tensors.  All
comparisons are of bytes, so floats are compared by their bits."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import lib, look, mlvfile, render, synth, tensor as T

import deep_cases as dp
import look_cases as lc
import mount_harness
from mount_harness import H as DH, W as DW, calibration, fresh, load_tool, make_clip, open_mount, payloads, route_args, run_tool, serve_calls as serve

pytestmark = pytest.mark.gpu
GAIN = 1.5
ORDER = ((2, 3), (0, 2))                                 # frames 2..4, then 0..1, in batches of 2
DEEP = {name: (S, n, Tb) for name, S, n, Tb in dp.looks()}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = {"scaled": (20, 13), "resampled": (301, 190), "resampled_small": (45, 29)}
ROUTES = {route: route_args(route.split("_")[0], SIZES.get(route)) for route in ("half", "full", "scaled", "resampled", "resampled_small")}
TORCH_NAMES = {T.F32: "float32", T.F16: "float16", T.BF16: "bfloat16", T.U8: "uint8", T.U16: "uint16"}


def tensor_bytes(t):
    """a tensor's frames as bytes"""
    import torch
    t = t.contiguous().cpu()
    flat = t.view(torch.uint8) if t.element_size() == 1 else t.view({2: torch.int16, 4: torch.int32}[t.element_size()])
    return [flat[k].numpy().tobytes() for k in range(t.shape[0])]


def out_size(route, w, h):
    return mount_harness.out_size(ROUTES[route], w, h)


def want_rgb(files, route, w, h, deep, dtype, layout, scale, bias):
    ow, oh = out_size(route, w, h)
    split = render.split_file16 if deep else render.split_file
    return [T.rgb(split(f, ow, oh), 16 if deep else 8, dtype, layout, scale, bias).tobytes() for f in files]


def want_bayer(dngs, w, h, dtype, layout, scale, bias):
    out = []
    for f in dngs:
        assert len(f) == 65536 + w * h * 2
        black, white = render.header_colour(f[:65536])[:2]
        out.append(T.bayer(np.frombuffer(f, "<u2", offset=65536).reshape(h, w), black, white, dtype, layout, scale, bias).tobytes())
    return out


def serve_dng(gpu, path, opts, order=ORDER, **cal):
    files, _, res, _ = mount_harness.serve(gpu, path, opts, "dng", order=[(f, c, GAIN) for f, c in order], **cal)
    return files, res


def check_route(gpu, path, opts, w, h, route, tone, dtype, layout, norm, cal, order=ORDER, amaze=False):
    """the file route and the tensor route of the same arguments on fresh handles of their own: the tensor is the definition of the
    file's pixels, and the results[] are the same"""
    deep = tone == "deep"
    mean, std = (MEAN, STD) if norm else (None, None)
    scale, bias = T.normalisation(mean, std, 3)
    with look.Look(*lc.look_of("random17")) as l8, look.Look16(*DEEP["random3"]) as l16:
        def setup(m):
            if tone == "look":
                m.set_look(l8)
            if amaze:
                m.set_demosaic("amaze")
                m.set_resample_demosaic("amaze")
        kw = dict(ROUTES[route], gain=GAIN, batch=2, look16=l16 if deep else None)
        files, res_f = serve(gpu, path, opts, lambda m, f, c, r: m.rgb(f, c, results=r, **kw), order, setup=setup, **cal)
        files = [f.tobytes() for a in files for f in a]
        tens, res_t = serve(gpu, path, opts, lambda m, f, c, r: m.tensor(f, c, dtype=TORCH_NAMES[dtype], layout="NCHW" if layout == T.NCHW else "NHWC", mean=mean,
                                                                        std=std, results=r, **kw), order, setup=setup, **cal)
    ow, oh = out_size(route, w, h)
    for t, (first, count) in zip(tens, order):
        assert tuple(t.shape) == (count,) + T.shape_of(3, oh, ow, layout) and t.is_cuda and str(t.dtype) == "torch." + TORCH_NAMES[dtype]
    got = [b for t in tens for b in tensor_bytes(t)]
    want = want_rgb(files, route, w, h, deep, dtype, layout, scale, bias)
    assert res_t == res_f and all(v in (0, 1) for v in res_t), (route, res_t, res_f)
    for k in range(len(want)):
        assert got[k] == want[k], (route, tone, dtype, layout, k, int((np.frombuffer(got[k], np.uint8) != np.frombuffer(want[k], np.uint8)).sum()))
    assert len(set(got)) == len(got), "two frames' tensors alike"


def check_bayer(gpu, path, opts, w, h, dtype, layout, norm, cal, order=ORDER):
    mean, std = ((0.1, 0.2, 0.2, 0.3), (0.5, 0.25, 0.25, 2.0)) if norm else (None, None)
    scale, bias = T.normalisation(mean, std, 4)
    dngs, res_d = serve_dng(gpu, path, opts, order, **cal)
    tens, res_t = serve(gpu, path, opts, lambda m, f, c, r: m.tensor(f, c, kind="bayer", dtype=TORCH_NAMES[dtype], layout="NCHW" if layout == T.NCHW else "NHWC",
                                                                    mean=mean, std=std, batch=2, results=r), order, **cal)
    for t, (first, count) in zip(tens, order):
        assert tuple(t.shape) == (count,) + T.shape_of(4, h // 2, w // 2, layout)
    got = [b for t in tens for b in tensor_bytes(t)]
    want = want_bayer(dngs, w, h, dtype, layout, scale, bias)
    assert res_t == res_d
    for k in range(len(want)):
        assert got[k] == want[k], ("bayer", dtype, layout, k, int((np.frombuffer(got[k], np.uint8) != np.frombuffer(want[k], np.uint8)).sum()))
    return dngs, res_d


OPTION_SETS = [("none", dict(), False), ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1), False), ("dark+flat", dict(), True)]
CASES = [(p, w, h, name, opts, cal) for p in ("plain", "lj92") for w, h in ((64, 48), (418, 266)) for name, opts, cal in OPTION_SETS]
TONES = (None, "look", "deep")


@pytest.mark.parametrize("payload,w,h,name,opts,cal", CASES, ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _, _ in CASES])
def test_mount_tensor_is_the_definition_of_the_served_file(gpu, tmp_path, payload, w, h, name, opts, cal):
    """the four sizes, each with another tone, dtype, layout and normalisation from case to case, and the Bayer tensor"""
    i = CASES.index((payload, w, h, name, opts, cal))
    path = make_clip(tmp_path, payload, w, h)
    with calibration(cal, w, h) as cal_args:
        for j, route in enumerate(("half", "full", "scaled", "resampled" if w > 301 else "resampled_small")):
            tone = TONES[(i + j) % 3]
            legal = [d for d in (T.F16, T.F32, T.BF16, T.U8, T.U16) if T.legal(d, 16 if tone == "deep" else 8)]
            check_route(gpu, path, opts, w, h, route, tone, legal[(i + 2 * j) % 4], (i + j) % 2, (i + j) % 3 != 0, cal_args)
        check_bayer(gpu, path, opts, w, h, (T.F16, T.F32, T.BF16, T.U16)[i % 4], i % 2, i % 3 == 0, cal_args)


@pytest.mark.parametrize("payload", ["plain", "lj92"])
def test_mount_tensor_on_a_mixed_dual_iso_clip(gpu, tmp_path, payload):
    """dual_iso = 2, frame 1 is not dual ISO: the converted frames have the x4 levels, in the Bayer tensor's unit as in the rendering"""
    path = make_clip(tmp_path, payload, DW, DH, normal_at=(1,), n=3)
    opts = dict(dual_iso=2, hdr_interp=1, cs=2)
    order = ((0, 3),)
    dngs, res = check_bayer(gpu, path, opts, DW, DH, T.F32 if payload == "plain" else T.F16, T.NCHW, False, {}, order)
    assert res == [1, 0, 1]
    levels = [render.header_colour(f[:65536])[:2] for f in dngs]
    assert levels[0] == (4 * 2048, 4 * 15000) and levels[1] == (2048, 15000)
    check_route(gpu, path, opts, DW, DH, "half", None, T.F16 if payload == "plain" else T.F32, T.NCHW, True, {}, order)


def test_mount_tensor_full_size_with_amaze(gpu, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h)
    check_route(gpu, path, dict(cs=5, stripes=1), w, h, "full", None, T.F16, T.NCHW, True, {}, amaze=True)
    check_route(gpu, path, dict(), w, h, "resampled_small", "deep", T.U16, T.NHWC, False, {}, amaze=True)


def test_tensor_and_file_calls_interleave_on_one_handle(gpu, tmp_path):
    """one handle that makes calls of all kinds serves, frame by frame, what handles serve that make calls of one kind only"""
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8),)
    dngs, _ = serve_dng(gpu, path, opts, order)
    rgbs, _ = serve(gpu, path, opts, lambda m, f, c, r: m.rgb(f, c, gain=GAIN, batch=4, results=r), order)
    rgbs = [f.tobytes() for f in rgbs[0]]
    fulls, _ = serve(gpu, path, opts, lambda m, f, c, r: m.rgb(f, c, gain=GAIN, batch=4, full=True, results=r), order)
    fulls = [f.tobytes() for f in fulls[0]]
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a = m.tensor(0, 2, gain=GAIN, batch=2)
        b = m.dng(2, 1, batch=2)
        c = m.tensor(3, 1, kind="bayer", dtype="float32", batch=2)
        d = m.rgb(4, 1, gain=GAIN, batch=2)
        e = m.tensor(5, 1, gain=GAIN, full=True, dtype="uint8", layout="NHWC", batch=2)
        f = m.rgb(6, 1, gain=GAIN, full=True, batch=2)
        g = [t for t in m.tensors(6, 2, batch=1, gain=GAIN, dtype="bfloat16")]
        ll, flags = m.dng_lossless(7, 1, batch=2)
    assert tensor_bytes(a) == want_rgb(rgbs[0:2], "half", w, h, False, T.F16, T.NCHW, one, zero)
    assert b[0].tobytes() == dngs[2] and tensor_bytes(c) == want_bayer(dngs[3:4], w, h, T.F32, T.NCHW, one, zero)
    assert d[0].tobytes() == rgbs[4] and tensor_bytes(e) == want_rgb(fulls[5:6], "full", w, h, False, T.U8, T.NHWC, one, zero)
    assert f[0].tobytes() == fulls[6] and len(g) == 2
    assert tensor_bytes(g[0]) + tensor_bytes(g[1]) == want_rgb(rgbs[6:8], "half", w, h, False, T.BF16, T.NCHW, one, zero)
    assert flags == [0] and len(ll[0]) < len(dngs[7])


def test_out_with_a_frame_stride_and_the_refusals(gpu, tmp_path):
    import torch
    w, h = 64, 48
    pw, ph = w // 2, h // 2
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    rgbs, _ = serve(gpu, path, opts, lambda m, f, c, r: m.rgb(f, c, gain=GAIN, batch=2, results=r), ((0, 4),))
    rgbs = [f.tobytes() for f in rgbs[0]]
    one, zero = np.ones(4, np.float32), np.zeros(4, np.float32)
    want = want_rgb(rgbs, "half", w, h, False, T.F16, T.NCHW, one, zero)
    n = 3 * pw * ph
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        buf = torch.full((4, n + 24), -23131, dtype=torch.int16, device="cuda")          # 0xA5A5
        out = torch.as_strided(buf.view(torch.float16), (4, 3, ph, pw), (n + 24, ph * pw, pw, 1))
        assert m.tensor(0, 4, gain=GAIN, batch=3, out=out) is out
        host = buf.cpu().numpy()
        assert [host[k, :n].tobytes() for k in range(4)] == want and (host[:, n:] == -23131).all()
        # what Python refuses: another shape, dtype, device, frames that are not contiguous
        for bad in (torch.empty((4, 3, ph, pw + 1), dtype=torch.float16, device="cuda"), torch.empty((4, 3, ph, pw), dtype=torch.float32, device="cuda"),
                    torch.empty((4, 3, ph, pw), dtype=torch.float16), torch.empty((4, 3, ph, 2 * pw), dtype=torch.float16, device="cuda")[..., ::2],
                    torch.empty((4, ph, pw, 3), dtype=torch.float16, device="cuda").permute(0, 3, 1, 2)):
            with pytest.raises(ValueError):
                m.tensor(0, 4, gain=GAIN, out=bad)
        # what the library refuses, each with the destination untouched: a host pointer, an illegal dtype, a shape the route does not take
        dst = torch.full((4 * n,), -23131, dtype=torch.int16, device="cuda")
        hostbuf = np.full(4 * n, 0xA5A5, np.uint16)
        sp = lib.TensorSpec(kind=T.RGB, dtype=T.F16, layout=T.NCHW, gain_q8=256)
        sp.scale[:] = [1.0] * 4
        call = lambda mh, ptr, spec_, stride=2 * n: gpu.mlvfs_amd_mount_tensor(mh, 0, 2, C.c_void_p(ptr), stride, C.byref(spec_), 2, 0, None)
        assert call(m.h, hostbuf.ctypes.data, sp) == lib.ERR_ARG and b"device memory" in gpu.mlvfs_amd_last_error()
        assert call(m.h, dst.data_ptr(), sp, 2 * n - 2) == lib.ERR_ARG
        bad = lib.TensorSpec(kind=T.RGB, dtype=T.U16, layout=T.NCHW, gain_q8=256)
        assert call(m.h, dst.data_ptr(), bad) == lib.ERR_ARG and b"illegal" in gpu.mlvfs_amd_last_error()
        wide = lib.TensorSpec(kind=T.RGB, dtype=T.F16, layout=T.NCHW, gain_q8=256, size=T.SCALED, ow=pw + 1, oh=3)
        wide.scale[:] = [1.0] * 4
        assert call(m.h, dst.data_ptr(), wide, 1 << 16) == lib.ERR_ARG and b"not supported" in gpu.mlvfs_amd_last_error()
        with pytest.raises(lib.MlvfsAmdError):
            m.tensor(0, 2, dtype="uint16")
        with pytest.raises(lib.MlvfsAmdError):
            m.tensor(0, 2, size=(pw + 1, 3))
        with pytest.raises(lib.MlvfsAmdError):
            m.tensor(3, 2)
        torch.cuda.synchronize()
        assert bool((dst == -23131).all()) and (hostbuf == 0xA5A5).all()
        assert tensor_bytes(m.tensor(0, 1, gain=GAIN)) == want[:1]              # the handle still serves: the refusals spoilt nothing
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)                                       # a proxy handle
    with r, m:
        dst = torch.full((4 * n,), -23131, dtype=torch.int16, device="cuda")
        with pytest.raises(lib.MlvfsAmdError, match="prox"):
            m.tensor(0, 2)
        with pytest.raises(lib.MlvfsAmdError, match="prox"):
            m.tensor(0, 2, kind="bayer")
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)


def test_mount_tensor_at_3584x1320(gpu, tmp_path):
    w, h = 3584, 1320
    frame = synth.normal_frame(w, h, seed=1, frame=0)
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, payloads([frame], "plain")[0], w, h)
    opts = dict(cs=5, stripes=1)
    scale, bias = T.normalisation(MEAN, STD, 3)
    for route in ("half", "full"):
        kw = dict(ROUTES[route], gain=1.0, batch=1)
        files, _ = serve(gpu, path, opts, lambda m, f, c, r: m.rgb(f, c, results=r, **kw), ((0, 1),))
        tens, _ = serve(gpu, path, opts, lambda m, f, c, r: m.tensor(f, c, mean=MEAN, std=STD, results=r, **kw), ((0, 1),))
        ow, oh = out_size(route, w, h)
        assert tuple(tens[0].shape) == (1, 3, oh, ow)
        assert tensor_bytes(tens[0]) == want_rgb([files[0][0].tobytes()], route, w, h, False, T.F16, T.NCHW, scale, bias), route


def test_the_tensor_tool_writes_the_tensors(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_tensor.py (its main(), in this process): the .npy files hold Mount.tensor's frames; a second run overwrites nothing"""
    tool = load_tool("mlv_tensor")
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=3)
    opts = dict(cs=5, stripes=1)

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2"] + extra)
    for k, (extra, kw) in enumerate([(["--gain", "1.5", "--mean", "0.485,0.456,0.406", "--std", "0.229,0.224,0.225"], dict(gain=1.5, mean=MEAN, std=STD)),
                                     (["--kind", "bayer", "--dtype", "bfloat16", "--layout", "NHWC"], dict(kind="bayer", dtype="bfloat16", layout="NHWC")),
                                     (["--size", "20x13", "--dtype", "uint8"], dict(size=(20, 13), dtype="uint8"))]):
        out = tmp_path / f"out{k}"
        assert run(out, extra) == 0
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.npy" % i for i in range(3)]
        tens, _ = serve(gpu, path, opts, lambda m, f, c, r: m.tensor(f, c, batch=2, results=r, **kw), ((0, 3),))
        assert [np.load(out / n).tobytes() for n in names] == tensor_bytes(tens[0])
        assert np.load(out / names[0]).shape == tuple(tens[0].shape[1:])
    capsys.readouterr()
    assert run(tmp_path / "out0", []) == 1 and "nothing is overwritten" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run(tmp_path / "out9", ["--kind", "bayer", "--full"])
    assert not os.path.exists(tmp_path / "out9")
