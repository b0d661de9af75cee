"""Rendered full-size sRGB frames on the GPU (csrc/k_demosaic.hip): mlvfs_amd_render1_dev against the numpy definition
of mlvfs_amd/demosaic.py on the cases of tests/demosaic_cases.py -- every size at which something can break, batches of 1 and 3 with
parameters of both matrix paths, padded strides, aligned and misaligned bases (so that k_render1_x16 and k_render1_generic both run at
every shape either could take, and are held to each other through the definition), the bytes around the renderings unchanged --,
parameters at the ends of their types, two 3584x1320 frames, and every refusal.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, render

import demosaic_cases as dm
import render_cases as rc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu


def up16(v):
    return (v + 15) // 16 * 16


def run_render1(gpu, frames, params, src_off, dst_off, aligned):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    n, img, pimg = len(frames), w * h * 2, w * h * 3
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(dm.params_array(params)).cuda()
    lib.check(gpu.mlvfs_amd_render1_dev(C.c_void_p(src.data_ptr() + src_off), stride, w, h, C.c_void_p(par.data_ptr()),
                                        C.c_void_p(dst.data_ptr() + dst_off), ostride, n, None), "render1_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [p.reshape(h, w, 3) for p in parts], rest


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


@pytest.mark.parametrize("w,h", dm.SIZES, ids=lambda v: str(v))
def test_render1_dev_equals_numpy(gpu, lut, w, h):
    for batch, src_off, dst_off, aligned in dm.dev_cases(w, h):
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        got, rest = run_render1(gpu, frames, params, src_off, dst_off, aligned)
        assert (rest == PAD).all(), (len(batch), src_off, dst_off, "bytes outside the renderings changed")
        for k, (f, p) in enumerate(batch):
            want = demosaic.render(f, p, lut)
            assert np.array_equal(got[k], want), (len(batch), src_off, dst_off, k, where(got[k], want))


def test_render1_dev_extreme_parameters(gpu, lut):
    """black at both ends of its type and below zero, A at its cap, K at both ends of its type and the largest a forward matrix of
    shorts can give; once through each form"""
    w, h = 48, 6
    f = rc.full_frame(w, h, 0, 65535, seed=77)
    big_k = render.params(0, 65535, (1, 1) * 3, (32767, -32768, 32767) * 3, 256)[4:]
    end_k = [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), -(1 << 31), -(1 << 31), (1 << 31) - 1]
    sets = [[-(1 << 31), 1, 3, 2] + rc.param_set(0)[1][4:], [(1 << 31) - 1, 5, 5, 5] + rc.param_set(1)[1][4:],
            [(1 << 31) - 70000, render.A_MAX, render.A_MAX, render.A_MAX] + rc.param_set(1)[1][4:],
            [-5000, render.A_MAX, 70000, 1 << 20] + rc.param_set(2)[1][4:], [100, 4000, 4100, 4200] + big_k,
            [65535, render.A_MAX, render.A_MAX, render.A_MAX] + big_k, [2048, 20000, 9000, 14000] + end_k,
            [0, 1 << 12, 1 << 12, 1 << 12] + [32767, 0, 0, 0, -32767, 0, 10000, -10000, 12767],          # the last K of the 32-bit path
            [0, 1 << 12, 1 << 12, 1 << 12] + [32767, 1, 0, 0, -32767, -1, 10000, -10000, 12768],         # the first of the 64-bit one
            [0, 0, 0, 0] + [0] * 9]
    assert [demosaic.matrix_fits_32(p) for p in sets[-3:]] == [True, False, True]
    for aligned, off in ((True, 0), (False, 2)):
        got, rest = run_render1(gpu, [f] * len(sets), sets, off, 0, aligned)
        assert (rest == PAD).all()
        for k, p in enumerate(sets):
            want = demosaic.render(f, p, lut)
            assert np.array_equal(got[k], want), (aligned, k, where(got[k], want))


def test_render1_dev_full_size(gpu, lut):
    (b0, w0), p0 = dm.param_set(2)
    (b1, w1), p1 = dm.param_set(4)
    assert demosaic.matrix_fits_32(p0) and not demosaic.matrix_fits_32(p1)
    frames = [rc.range_frame(dm.BIG_W, dm.BIG_H, b0, w0, seed=1), dm.speckle_frame(dm.BIG_W, dm.BIG_H, b1, w1)]
    want = [demosaic.render(frames[0], p0, lut), demosaic.render(frames[1], p1, lut)]
    got, rest = run_render1(gpu, frames, [p0, p1], 0, 0, True)
    assert (rest == PAD).all()
    for k in range(2):
        assert np.array_equal(got[k], want[k]), (k, where(got[k], want[k]))
    got, rest = run_render1(gpu, frames[:1], [p0], 2, 1, False)          # the generic form at that size
    assert (rest == PAD).all() and np.array_equal(got[0], want[0])


def test_render1_dev_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(dm.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p = src.data_ptr(), dst.data_ptr(), par.data_ptr()
    vp = lambda a: C.c_void_p(a) if a else None
    call = lambda sp, st, w, h, pp, dp, ost, n: gpu.mlvfs_amd_render1_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    # a 16 x 8 frame: 256 bytes in, 384 out
    bad = [(0, 256, 16, 8, p, d, 384, 1), (s, 256, 16, 8, p, 0, 384, 1), (s, 256, 16, 8, 0, d, 384, 1), (s, 256, 3, 8, p, d, 384, 1),
           (s, 256, 16, 3, p, d, 384, 1), (s, 256, 2, 2, p, d, 384, 1), (s, 256, 1 << 13, 1 << 12, p, d, 384, 1), (s, 256, -16, 8, p, d, 384, 1),
           (s, 256, 16, 8, p, d, 384, -1), (s, 254, 16, 8, p, d, 384, 2), (s, 256, 16, 8, p, d, 383, 2), (s, 257, 16, 8, p, d, 384, 2),
           (s + 1, 256, 16, 8, p, d, 384, 1), (s, 256, 16, 8, p + 2, d, 384, 1),
           (d + 1024, 256, 16, 8, p, d + 1024, 384, 1), (d + 1024, 256, 16, 8, p, d + 1024 + 255, 384, 1), (d + 1024, 256, 16, 8, p, d + 1024 - 383, 384, 1),
           (d + 1024, 256, 16, 8, p, d + 1024 + 512 + 255, 384, 3), (s, 256, 16, 8, d + 64, d, 384, 1)]
    for args in bad:
        assert call(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert call(d + 1024, 256, 16, 8, p, d + 1024 + 256, 384, 1) == 0       # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1280] == PAD).all() and (host[1280 + 384:] == PAD).all()
    want = demosaic.render(np.full((8, 16), PAD | PAD << 8, np.uint16), rc.param_set(0)[1])
    assert np.array_equal(host[1280:1280 + 384].reshape(8, 16, 3), want)
    pw, ph = C.c_int(-7), C.c_int(-7)
    assert gpu.mlvfs_amd_rgb_full_geom(7, 5, C.byref(pw), C.byref(ph)) == 0 and (pw.value, ph.value) == (7, 5)
    assert gpu.mlvfs_amd_rgb_full_geom(3, 5, C.byref(pw), C.byref(ph)) == lib.ERR_ARG and (pw.value, ph.value) == (7, 5)
