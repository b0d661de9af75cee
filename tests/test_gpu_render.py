"""Rendered half-size sRGB frames on the GPU (csrc/k_render.hip, csrc/mount.cpp): mlvfs_amd_render2_dev against the
numpy definition of mlvfs_amd/render.py, and mlvfs_amd_mount_rgb against a full-size mount of the same clip and options: the TIFF's
pixels are the definition applied to the pixels of the full-size .dng file, with the parameters the tags of that file's header give
(so every stage in front of the rendering ran as it does for a .dng, and the levels are the frame's final ones), results[] are the
same, and PIL opens every file.  All comparisons are for equality."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, render, synth

import render_cases as rc
from mount_harness import (GAIN_A, HDR, OPTION_SETS, PAYLOADS, calibration, check_tiffs, fresh, load_tool, lut, make_clip, open_mount, payloads,
                           renderings, run_tool, serve)
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ mlvfs_amd_render2_dev
def up16(v):
    return (v + 15) // 16 * 16


def run_render2(gpu, frames, params, src_off, dst_off, aligned):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    pw, ph = render.geom(w, h)
    n, img, pimg = len(frames), w * h * 2, pw * ph * 3
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(rc.params_array(params)).cuda()
    lib.check(gpu.mlvfs_amd_render2_dev(C.c_void_p(src.data_ptr() + src_off), stride, w, h, C.c_void_p(par.data_ptr()),
                                        C.c_void_p(dst.data_ptr() + dst_off), ostride, n, None), "render2_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [p.reshape(ph, pw, 3) for p in parts], rest


@pytest.mark.parametrize("w,h", rc.SIZES, ids=lambda v: str(v))
def test_render2_dev_equals_numpy(gpu, w, h):
    for batch, src_off, dst_off, aligned in rc.dev_cases(w, h):
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        got, rest = run_render2(gpu, frames, params, src_off, dst_off, aligned)
        assert (rest == PAD).all(), (len(batch), src_off, dst_off, "bytes outside the renderings changed")
        for k, (f, p) in enumerate(batch):
            want = render.render(f, p, lut())
            assert np.array_equal(got[k], want), (len(batch), src_off, dst_off, k, int((got[k] != want).sum()))


def test_render2_dev_extreme_parameters(gpu):
    """black at both ends of its type and below zero, A at its cap, the largest K a forward matrix of shorts can give"""
    w, h = 48, 6
    f = rc.full_frame(w, h, 0, 65535, seed=77)
    big_k = render.params(0, 65535, (1, 1) * 3, (32767, -32768, 32767) * 3, 256)[4:]
    sets = [[-(1 << 31), 1, 3, 2] + rc.param_set(0)[1][4:], [(1 << 31) - 1, 5, 5, 5] + rc.param_set(1)[1][4:],
            [-5000, render.A_MAX, 70000, 1 << 20] + rc.param_set(2)[1][4:], [100, 4000, 4100, 4200] + big_k,
            [65535, render.A_MAX, render.A_MAX, render.A_MAX] + big_k, [0, 0, 0, 0] + [0] * 9]
    for aligned, off in ((True, 0), (False, 2)):
        got, rest = run_render2(gpu, [f] * len(sets), sets, off, 0, aligned)
        assert (rest == PAD).all()
        for k, p in enumerate(sets):
            assert np.array_equal(got[k], render.render(f, p, lut())), (aligned, k)


def test_render2_dev_full_size(gpu):
    (b0, w0), p0 = rc.param_set(2)
    (b1, w1), p1 = rc.param_set(3)
    frames = [rc.range_frame(rc.BIG_W, rc.BIG_H, b0, w0, seed=1), rc.grey_ramp(rc.BIG_W, rc.BIG_H, b1, w1)]
    want = [render.render(frames[0], p0, lut()), render.render(frames[1], p1, lut())]
    got, rest = run_render2(gpu, frames, [p0, p1], 0, 0, True)
    assert (rest == PAD).all()
    for k in range(2):
        assert np.array_equal(got[k], want[k]), k
    got, rest = run_render2(gpu, frames[:1], [p0], 2, 1, False)          # the generic form at that size
    assert (rest == PAD).all() and np.array_equal(got[0], want[0])


def test_render2_dev_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(rc.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p = src.data_ptr(), dst.data_ptr(), par.data_ptr()
    vp = lambda a: C.c_void_p(a) if a else None
    call = lambda sp, st, w, h, pp, dp, ost, n: gpu.mlvfs_amd_render2_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    bad = [(0, 512, 16, 16, p, d, 192, 1), (s, 512, 16, 16, p, 0, 192, 1), (s, 512, 16, 16, 0, d, 192, 1), (s, 512, 1, 16, p, d, 192, 1),
           (s, 512, 16, 1, p, d, 192, 1), (s, 512, 1 << 14, 1 << 13, p, d, 192, 1), (s, 512, 16, 16, p, d, 192, -1), (s, 510, 16, 16, p, d, 192, 2),
           (s, 512, 16, 16, p, d, 191, 2), (s, 513, 16, 16, p, d, 192, 2), (s + 1, 512, 16, 16, p, d, 192, 1), (s, 512, 16, 16, p + 2, d, 192, 1),
           (d + 1024, 512, 16, 16, p, d + 1024, 192, 1), (d + 1024, 512, 16, 16, p, d + 1024 + 511, 192, 1), (d + 1024, 512, 16, 16, p, d + 1024 - 191, 192, 1),
           (d + 1024, 512, 16, 16, p, d + 1024 + 1024 + 511, 256, 3), (s, 512, 16, 16, d + 64, d, 192, 1)]
    for args in bad:
        assert call(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert call(d + 1024, 512, 16, 16, p, d + 1024 + 512, 192, 1) == 0      # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1536] == PAD).all() and (host[1536 + 192:] == PAD).all()
    want = render.render(np.full((16, 16), PAD | PAD << 8, np.uint16), rc.param_set(0)[1])
    assert np.array_equal(host[1536:1536 + 192].reshape(8, 8, 3), want)


# ------------------------------------------------------------------ the mount
CASES = [(p, w, h, name, opts, cal) for p in PAYLOADS for w, h in rc.MOUNT_SIZES for name, opts, cal in OPTION_SETS]


@pytest.mark.parametrize("payload,w,h,name,opts,cal", CASES, ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _, _ in CASES])
def test_mount_rgb_is_the_full_size_file_rendered(gpu, reference, tmp_path, payload, w, h, name, opts, cal):
    path = make_clip(tmp_path, payload, w, h, dual=bool(opts.get("dual_iso")), reference=reference)
    with calibration(cal, w, h) as cal_args:
        full, _, res_full, _ = serve(gpu, path, opts, "dng", **cal_args)
        rgb, _, res_rgb, gains = serve(gpu, path, opts, "rgb", **cal_args)
    assert res_rgb == res_full and all(r in (0, 1) for r in res_full)
    check_tiffs(renderings(full, gains, w, h, "half"), rgb, render.geom(w, h), f"{payload}:{w}x{h}:{name}")
    assert len({f for f in rgb}) == len(rgb), "two frames rendered alike"


def test_mount_rgb_uses_the_x4_levels_of_a_converted_frame(gpu, tmp_path):
    """416x264, the size the dual-ISO tests convert at: a mixed clip, frames 1 and 3 are not dual ISO and keep their levels"""
    path = make_clip(tmp_path, "plain", 416, 264, normal_at=(1, 3))
    opts = dict(dual_iso=2, hdr_interp=1, cs=2)
    order = ((0, 5, GAIN_A),)
    full, _, res_full, _ = serve(gpu, path, opts, "dng", order=order, batch=3)
    rgb, _, res_rgb, gains = serve(gpu, path, opts, "rgb", order=order, batch=3)
    assert res_full == res_rgb == [1, 0, 1, 0, 1]
    levels = [render.header_colour(f[:65536])[:2] for f in full]
    assert levels[0] == (4 * 2048, 4 * 15000) and levels[1] == (2048, 15000)
    check_tiffs(renderings(full, gains, 416, 264, "half"), rgb, render.geom(416, 264), "mixed dual ISO")


def test_mount_rgb_and_dng_calls_interleave_in_serve_order(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 416, 264, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, GAIN_A),)
    want_dng, _, _, _ = serve(gpu, path, opts, "dng", order=order, batch=4)
    want_rgb, _, _, gains = serve(gpu, path, opts, "rgb", order=order, batch=4)
    check_tiffs(renderings(want_dng, gains, 416, 264, "half"), want_rgb, render.geom(416, 264), "one kind")
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a = m.rgb(0, 3, batch=2)
        b = m.dng(3, 2, batch=2)
        c, flags = m.dng_lossless(5, 1, batch=2)
        d = m.rgb(6, 2, batch=2)
    assert [f.tobytes() for f in a] + [f.tobytes() for f in d] == want_rgb[:3] + want_rgb[6:]
    assert [f.tobytes() for f in b] == want_dng[3:5]
    assert flags == [0] and len(c[0]) < len(want_dng[5])


def test_mount_rgb_strides_and_a_proxy_handle(gpu, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve(gpu, path, opts, "rgb", order=order)
    size = HDR + 32 * 24 * 3
    assert size < 65536, "the file is smaller than a .dng header: no header of that kind may be written on the way"
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        out = np.full(4 * (size + 37) + 64, 0xA5, np.uint8)
        assert gpu.mlvfs_amd_mount_rgb(m.h, 0, 4, lib.ptr(out), size - 1, 256, 2, 0, None) == lib.ERR_ARG and (out == 0xA5).all()
        # exactly the file's size is room enough
        lib.check(gpu.mlvfs_amd_mount_rgb(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None), "mount_rgb")
        assert [out[k * size:(k + 1) * size].tobytes() for k in range(2)] == want[:2] and (out[2 * size:] == 0xA5).all()
        out[:] = 0xA5
        st = size + 37                                            # and anything above; the bytes between the files stay
        lib.check(gpu.mlvfs_amd_mount_rgb(m.h, 2, 2, lib.ptr(out), st, 256, 2, 0, None), "mount_rgb")
        assert [out[k * st:k * st + size].tobytes() for k in range(2)] == want[2:]
        assert (out[size:st] == 0xA5).all() and (out[st + size:] == 0xA5).all()
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        out[:] = 0xA5
        assert gpu.mlvfs_amd_mount_rgb(m.h, 0, 2, lib.ptr(out), size, 256, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert (out == 0xA5).all()
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2)
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)        # the refusal served nothing and spoilt nothing


def test_mount_rgb_full_size(gpu, tmp_path):
    w, h = rc.BIG_W, rc.BIG_H
    frames = [synth.normal_frame(w, h, seed=1, frame=k) for k in range(2)]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, payloads(frames, "plain")[0], w, h)
    opts = dict(cs=5, stripes=1)
    order = ((0, 2, GAIN_A),)
    full, _, _, _ = serve(gpu, path, opts, "dng", order=order)
    rgb, _, _, gains = serve(gpu, path, opts, "rgb", order=order)
    assert len(rgb[0]) == HDR + 1792 * 660 * 3
    check_tiffs(renderings(full, gains, w, h, "half"), rgb, render.geom(w, h), "3584x1320")


def test_the_render_tool_writes_the_sequence_and_overwrites_nothing(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py (its main(), in this process): the files are mlvfs_amd_mount_rgb's; a second run into the same place is
    refused and leaves the files"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, "rgb", order=((0, 3, 1.5),))
    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    out = tmp_path / "out"
    assert run(out, []) == 0
    names = sorted(os.listdir(out))
    assert names == ["M07-1234_%06d.tif" % k for k in range(3)]
    assert [open(out / n, "rb").read() for n in names] == want
    with Image.open(out / names[0]) as im:
        assert im.mode == "RGB" and im.size == (32, 24)
    capsys.readouterr()
    assert run(out, []) == 1 and "nothing is overwritten" in capsys.readouterr().err
    assert [open(out / n, "rb").read() for n in names] == want
