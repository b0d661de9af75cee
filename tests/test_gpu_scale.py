"""Rendered frames at any smaller size on the GPU (csrc/k_scale.hip): mlvfs_amd_render_scaled_dev against the numpy
definition of mlvfs_amd/scale.py on the cases of tests/scale_cases.py -- every source size at which a mechanism can break, each at
the output sizes that stress it, batches of 1 and 3 with different parameters per frame, padded strides, aligned and misaligned bases
(so that k_scale_x16 and k_scale_generic both run wherever either could, and are held to each other through the definition), the
source and the bytes around the renderings unchanged --, the identity against mlvfs_amd_render2_dev, the rounding cases, parameters at
the ends of their types, the white frame of the widest grid, and every refusal.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import lib, render, scale

import render_cases as rc
import scale_cases as sc
from test_gpu_mlv_transcode import PAD, device_buffer, split
from test_gpu_render import run_render2

pytestmark = pytest.mark.gpu


def up16(v):
    return (v + 15) // 16 * 16


def run_scaled(gpu, frames, params, ow, oh, src_off, dst_off, aligned):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    n, img, pimg = len(frames), w * h * 2, ow * oh * 3
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(sc.params_array(params)).cuda()
    lib.check(gpu.mlvfs_amd_render_scaled_dev(C.c_void_p(src.data_ptr() + src_off), stride, w, h, C.c_void_p(par.data_ptr()), ow, oh,
                                              C.c_void_p(dst.data_ptr() + dst_off), ostride, n, None), "render_scaled_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [p.reshape(oh, ow, 3) for p in parts], rest


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


@pytest.mark.parametrize("w,h", sc.SOURCES, ids=lambda v: str(v))
def test_render_scaled_dev_equals_numpy(gpu, lut, w, h):
    pw, ph = w // 2, h // 2
    for ow, oh, batch, src_off, dst_off, aligned in sc.dev_cases(w, h):
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        got, rest = run_scaled(gpu, frames, params, ow, oh, src_off, dst_off, aligned)
        assert (rest == PAD).all(), (ow, oh, len(batch), src_off, dst_off, "bytes outside the renderings changed")
        for k, (f, p) in enumerate(batch):
            want = scale.render(f, p, ow, oh, lut)
            assert np.array_equal(got[k], want), (ow, oh, len(batch), src_off, dst_off, k, where(got[k], want))
        if (ow, oh) == (pw, ph):                                             # the identity: what mlvfs_amd_render2_dev writes
            half, _ = run_render2(gpu, frames, params, src_off, dst_off, aligned)
            for k in range(len(batch)):
                assert np.array_equal(got[k], half[k]), (len(batch), src_off, k)


def test_render_scaled_dev_rounds_the_half_up(gpu, lut):
    """the cases with a known average, through the form their width selects and through the generic one"""
    cases = sc.rounding_cases() + sc.half_case(7) + sc.half_case(40000, 2)
    for f, p, ow, oh, byte in cases:
        for aligned, off in ((True, 0), (False, 2)):
            got, rest = run_scaled(gpu, [f], [p], ow, oh, off, 0, aligned)
            assert (rest == PAD).all() and (got[0] == byte).all(), (f.shape, ow, oh, byte, aligned, got[0].ravel()[:6].tolist())


def test_render_scaled_dev_extreme_parameters(gpu, lut):
    """black at both ends of its type and below zero, A at its cap, the largest K a forward matrix of shorts can give"""
    w, h = 48, 6
    f = rc.full_frame(w, h, 0, 65535, seed=77)
    big_k = render.params(0, 65535, (1, 1) * 3, (32767, -32768, 32767) * 3, 256)[4:]
    end_k = [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), -(1 << 31), -(1 << 31), (1 << 31) - 1]
    sets = [[-(1 << 31), 1, 3, 2] + rc.param_set(0)[1][4:], [(1 << 31) - 1, 5, 5, 5] + rc.param_set(1)[1][4:],
            [-5000, render.A_MAX, 70000, 1 << 20] + rc.param_set(2)[1][4:], [100, 4000, 4100, 4200] + big_k,
            [65535, render.A_MAX, render.A_MAX, render.A_MAX] + big_k, [2048, 20000, 9000, 14000] + end_k, [0, 0, 0, 0] + [0] * 9]
    for ow, oh in ((24, 3), (7, 2), (23, 1)):
        for aligned, off in ((True, 0), (False, 2)):
            got, rest = run_scaled(gpu, [f] * len(sets), sets, ow, oh, off, 0, aligned)
            assert (rest == PAD).all()
            for k, p in enumerate(sets):
                want = scale.render(f, p, ow, oh, lut)
                assert np.array_equal(got[k], want), (ow, oh, aligned, k, where(got[k], want))


@pytest.mark.parametrize("w,h", [(131070, 2), (131056, 2), (2, 131070)], ids=lambda v: str(v))
def test_a_white_frame_stays_white_at_one_pixel(gpu, w, h):
    """every n_j = 65535 over the widest span there is: the sum 65535 * 65535 + 32767 needs all 32 bits"""
    for f, p, ow, oh, byte in sc.white_cases(w, h):
        got, rest = run_scaled(gpu, [f], [p], ow, oh, 0, 0, True)
        assert (rest == PAD).all() and got[0].tolist() == [[[byte] * 3]], got[0].tolist()


def test_render_scaled_dev_at_the_bench_size(gpu, lut):
    (b0, w0), p0 = rc.param_set(2)
    (b1, w1), p1 = rc.param_set(3)
    frames = [rc.range_frame(sc.BIG_W, sc.BIG_H, b0, w0, seed=1), rc.grey_ramp(sc.BIG_W, sc.BIG_H, b1, w1)]
    for ow, oh in ((1280, 472), (160, 59)):
        want = [scale.render(frames[0], p0, ow, oh, lut), scale.render(frames[1], p1, ow, oh, lut)]
        got, rest = run_scaled(gpu, frames, [p0, p1], ow, oh, 0, 0, True)
        assert (rest == PAD).all()
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (ow, oh, k, where(got[k], want[k]))
    got, rest = run_scaled(gpu, frames[:1], [p0], 160, 59, 2, 1, False)          # the generic form at that size
    assert (rest == PAD).all() and np.array_equal(got[0], want[0])


def test_render_scaled_dev_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(sc.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p = src.data_ptr(), dst.data_ptr(), par.data_ptr()
    vp = lambda a: C.c_void_p(a) if a else None
    call = lambda sp, st, w, h, pp, ow, oh, dp, ost, n: gpu.mlvfs_amd_render_scaled_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, None)
    # a 32 x 8 frame: 512 bytes in, 7 x 3 = 63 out
    bad = [(0, 512, 32, 8, p, 7, 3, d, 64, 1), (s, 512, 32, 8, p, 7, 3, 0, 64, 1), (s, 512, 32, 8, 0, 7, 3, d, 64, 1), (s, 512, 1, 8, p, 1, 1, d, 64, 1),
           (s, 512, 32, 1, p, 1, 1, d, 64, 1), (s, 512, 1 << 14, 1 << 13, p, 7, 3, d, 64, 1), (s, 512, 131072, 2, p, 7, 1, d, 64, 1), (s, 512, -32, 8, p, 7, 3, d, 64, 1),
           (s, 512, 32, 8, p, 0, 3, d, 64, 1), (s, 512, 32, 8, p, 7, 0, d, 64, 1), (s, 512, 32, 8, p, 17, 3, d, 64, 1), (s, 512, 32, 8, p, 7, 5, d, 64, 1),
           (s, 512, 32, 8, p, -7, -3, d, 64, 1),
           (s, 512, 32, 8, p, 7, 3, d, 64, -1), (s, 510, 32, 8, p, 7, 3, d, 64, 2), (s, 512, 32, 8, p, 7, 3, d, 62, 2), (s, 513, 32, 8, p, 7, 3, d, 64, 2),
           (s + 1, 512, 32, 8, p, 7, 3, d, 64, 1), (s, 512, 32, 8, p + 2, 7, 3, d, 64, 1),
           (d + 1024, 512, 32, 8, p, 7, 3, d + 1024, 64, 1), (d + 1024, 512, 32, 8, p, 7, 3, d + 1024 + 511, 64, 1), (d + 1024, 512, 32, 8, p, 7, 3, d + 1024 - 62, 64, 1),
           (d + 1024, 512, 32, 8, p, 7, 3, d + 1024 + 1024 + 511, 64, 3), (s, 512, 32, 8, d + 32, 7, 3, d, 64, 1)]
    for args in bad:
        assert call(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert call(d + 1024, 512, 32, 8, p, 7, 3, d + 1024 + 512, 64, 1) == 0   # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1536] == PAD).all() and (host[1536 + 63:] == PAD).all()
    want = scale.render(np.full((8, 32), PAD | PAD << 8, np.uint16), rc.param_set(0)[1], 7, 3)
    assert np.array_equal(host[1536:1536 + 63].reshape(3, 7, 3), want)
    ow, oh = C.c_int(-7), C.c_int(-7)
    assert gpu.mlvfs_amd_rgb_fit(32, 8, 7, 7, C.byref(ow), C.byref(oh)) == 0 and (ow.value, oh.value) == (7, 2)
