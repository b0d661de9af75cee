"""Rendered frames resampled from the full-size rendering on the GPU (csrc/k_resample.hip):
mlvfs_amd_render_resampled_dev and its look and deep forms against the numpy definition of mlvfs_amd/resample.py on the cases of
tests/resample_cases.py -- every source size at which a mechanism can break, each at the output sizes that stress it, batches of 1 and
3 with different parameters per frame (both matrix paths in a batch of three), padded strides, aligned and misaligned bases (so that
k_resample_x16 and k_resample_generic both run wherever both can, and are held to each other through the definition), the source and
the bytes around the renderings unchanged --, the identity against mlvfs_amd_render1_dev, parameters at the ends of their types, white
frames of the widest grids, two frames at the bench size, and every refusal.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, look, render, resample

import deep_cases as dp
import demosaic_cases as dc
import look_cases as lc
import render_cases as rc
import resample_cases as rs
from test_gpu_demosaic import run_render1
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
LOOKS = {name: (S, n, T) for name, S, n, T in lc.looks()}
LOOKS16 = {name: (S, n, T) for name, S, n, T in dp.looks()}


def up16(v):
    return (v + 15) // 16 * 16


def run_resampled(gpu, frames, params, ow, oh, src_off, dst_off, aligned, lk=None, lk16=None):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    bpx = 6 if lk16 else 3
    n, img, pimg = len(frames), w * h * 2, ow * oh * bpx
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(rs.params_array(params)).cuda()
    s, d, p = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off), C.c_void_p(par.data_ptr())
    if lk16:
        rc_ = gpu.mlvfs_amd_render_resampled_deep_dev(s, stride, w, h, p, ow, oh, d, ostride, n, C.c_void_p(lk16.h), None)
    elif lk:
        rc_ = gpu.mlvfs_amd_render_resampled_look_dev(s, stride, w, h, p, ow, oh, d, ostride, n, C.c_void_p(lk.h), None)
    else:
        rc_ = gpu.mlvfs_amd_render_resampled_dev(s, stride, w, h, p, ow, oh, d, ostride, n, None)
    lib.check(rc_, "render_resampled_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    if lk16:
        return [np.frombuffer(q.tobytes(), "<u2").reshape(oh, ow, 3) for q in parts], rest
    return [q.reshape(oh, ow, 3) for q in parts], rest


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


@pytest.mark.parametrize("w,h", rs.SOURCES, ids=lambda v: str(v))
def test_render_resampled_dev_equals_numpy(gpu, lut, w, h):
    for ow, oh, batch, src_off, dst_off, aligned in rs.dev_cases(w, h):
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        got, rest = run_resampled(gpu, frames, params, ow, oh, src_off, dst_off, aligned)
        assert (rest == PAD).all(), (ow, oh, len(batch), src_off, dst_off, "bytes outside the renderings changed")
        for k, (f, p) in enumerate(batch):
            want = resample.render(f, p, ow, oh, lut)
            assert np.array_equal(got[k], want), (ow, oh, len(batch), src_off, dst_off, k, where(got[k], want))
        if (ow, oh) == (w, h):                                               # the identity: what mlvfs_amd_render1_dev writes
            full, _ = run_render1(gpu, frames, params, src_off, dst_off, aligned)
            for k in range(len(batch)):
                assert np.array_equal(got[k], full[k]), (len(batch), src_off, k)


def test_render_resampled_dev_extreme_parameters(gpu, lut):
    w, h = 48, 6
    f = rc.full_frame(w, h, 0, 65535, seed=77)
    sets = rs.extreme_sets()
    for ow, oh in ((48, 6), (47, 5), (25, 2), (7, 2)):
        for aligned, off in ((True, 0), (False, 2)):
            got, rest = run_resampled(gpu, [f] * len(sets), sets, ow, oh, off, 0, aligned)
            assert (rest == PAD).all()
            for k, p in enumerate(sets):
                want = resample.render(f, p, ow, oh, lut)
                assert np.array_equal(got[k], want), (ow, oh, aligned, k, where(got[k], want))


@pytest.mark.parametrize("w,h", rs.WHITE, ids=lambda v: str(v))
def test_a_white_frame_stays_white(gpu, w, h):
    """every d_c = 65535 over the widest spans there are"""
    for f, p, ow, oh, byte in rs.white_cases(w, h):
        got, rest = run_resampled(gpu, [f], [p], ow, oh, 0, 0, True)
        assert (rest == PAD).all() and (got[0] == byte).all(), (ow, oh, got[0].ravel()[:6].tolist())


def test_a_flat_frame_renders_to_the_half_size_pixel(gpu, lut):
    _, p = dc.param_set(1)
    f = dc.flat_frame(96, 34, 1200, 3000, 1700)
    want = render.render(f[:2, :2], p, lut)[0, 0]
    for ow, oh in rs.out_sizes(96, 34):
        for aligned, off in ((True, 0), (False, 2)):
            got, rest = run_resampled(gpu, [f], [p], ow, oh, off, 0, aligned)
            assert (rest == PAD).all() and (got[0] == want).all(), (ow, oh, aligned)


LOOK_SHAPES = [((48, 6), (48, 6)), ((96, 34), (64, 23)), ((528, 65), (527, 64)), ((418, 267), (210, 134))]


@pytest.mark.parametrize("src,size", LOOK_SHAPES, ids=lambda v: str(v))
def test_render_resampled_look_and_deep_dev_equal_numpy(gpu, src, size):
    (w, h), (ow, oh) = src, size
    names, names16 = list(LOOKS), list(LOOKS16)
    for k, (n, src_off, dst_off, aligned) in enumerate(rs.PLACEMENTS):
        batch = dc.batch(w, h, n, k + w)
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        name, name16 = names[(k + w) % len(names)], names16[(k + w) % len(names16)]
        with look.Look(*LOOKS[name]) as lk:
            got, rest = run_resampled(gpu, frames, params, ow, oh, src_off, dst_off, aligned, lk=lk)
        assert (rest == PAD).all()
        for i, (f, p) in enumerate(batch):
            want = resample.render(f, p, ow, oh, look=LOOKS[name])
            assert np.array_equal(got[i], want), (name, n, aligned, i, where(got[i], want))
        with look.Look16(*LOOKS16[name16]) as lk16:
            got, rest = run_resampled(gpu, frames, params, ow, oh, src_off, 2 * dst_off, aligned, lk16=lk16)
        assert (rest == PAD).all()
        for i, (f, p) in enumerate(batch):
            want = resample.render(f, p, ow, oh, look16=LOOKS16[name16])
            assert np.array_equal(got[i], want), (name16, n, aligned, i, where(got[i], want))


def test_the_identity_look_reproduces_the_plain_call(gpu):
    """S = 257 LUT and the identity table: the plain kernels' bytes from the look kernels, through both forms"""
    batch = dc.batch(48, 6, 3, 5)
    frames, params = [f for f, _ in batch], [p for _, p in batch]
    with look.Look(look.shaper_srgb(), 17, look.identity(17)) as i17:
        for aligned, off in ((True, 0), (False, 2)):
            got, _ = run_resampled(gpu, frames, params, 33, 5, off, 0, aligned, lk=i17)
            want, _ = run_resampled(gpu, frames, params, 33, 5, off, 0, aligned)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), aligned


def test_render_resampled_dev_at_the_bench_size(gpu, lut):
    (b0, w0), p0 = rc.param_set(2)
    (b1, w1), p1 = dc.param_set(1)
    frames = [rc.range_frame(rs.BIG_W, rs.BIG_H, b0, w0, seed=1), rc.grey_ramp(rs.BIG_W, rs.BIG_H, b1, w1)]
    d = [demosaic.stages(frames[0], p0)["n"], demosaic.stages(frames[1], p1)["n"]]       # once per frame, for both sizes
    for ow, oh in rs.BIG_SIZES:
        want = [resample.render(frames[0], p0, ow, oh, lut, source=d[0]), resample.render(frames[1], p1, ow, oh, lut, source=d[1])]
        got, rest = run_resampled(gpu, frames, [p0, p1], ow, oh, 0, 0, True)
        assert (rest == PAD).all()
        for k in range(2):
            assert np.array_equal(got[k], want[k]), (ow, oh, k, where(got[k], want[k]))
    got, rest = run_resampled(gpu, frames[1:], [p1], ow, oh, 2, 1, False)            # the generic form at that size
    assert (rest == PAD).all() and np.array_equal(got[0], want[1])


def test_render_resampled_dev_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(rs.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p = src.data_ptr(), dst.data_ptr(), par.data_ptr()
    vp = lambda a: C.c_void_p(a) if a else None
    plain = lambda sp, st, w, h, pp, ow, oh, dp_, ost, n: gpu.mlvfs_amd_render_resampled_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp_), ost, n, None)
    # a 32 x 8 frame: 512 bytes in, 20 x 5 = 300 out
    bad = [(0, 512, 32, 8, p, 20, 5, d, 304, 1), (s, 512, 32, 8, p, 20, 5, 0, 304, 1), (s, 512, 32, 8, 0, 20, 5, d, 304, 1), (s, 512, 3, 8, p, 1, 1, d, 304, 1),
           (s, 512, 32, 3, p, 1, 1, d, 304, 1), (s, 512, 1 << 13, 1 << 12, p, 20, 5, d, 304, 1), (s, 512, 65536, 4, p, 20, 1, d, 304, 1), (s, 512, 4, 65536, p, 1, 5, d, 304, 1),
           (s, 512, -32, 8, p, 20, 5, d, 304, 1), (s, 512, 32, 8, p, 0, 5, d, 304, 1), (s, 512, 32, 8, p, 20, 0, d, 304, 1), (s, 512, 32, 8, p, 33, 5, d, 304, 1),
           (s, 512, 32, 8, p, 20, 9, d, 304, 1), (s, 512, 32, 8, p, -20, -5, d, 304, 1),
           (s, 512, 32, 8, p, 20, 5, d, 304, -1), (s, 510, 32, 8, p, 20, 5, d, 304, 2), (s, 512, 32, 8, p, 20, 5, d, 298, 2), (s, 513, 32, 8, p, 20, 5, d, 304, 2),
           (s + 1, 512, 32, 8, p, 20, 5, d, 304, 1), (s, 512, 32, 8, p + 2, 20, 5, d, 304, 1),
           (d + 1024, 512, 32, 8, p, 20, 5, d + 1024, 304, 1), (d + 1024, 512, 32, 8, p, 20, 5, d + 1024 + 511, 304, 1), (d + 1024, 512, 32, 8, p, 20, 5, d + 1024 - 299, 304, 1),
           (d + 1024, 512, 32, 8, p, 20, 5, d + 1024 + 1024 + 511, 304, 3), (s, 512, 32, 8, d + 32, 20, 5, d, 304, 1)]
    for args in bad:
        assert plain(*args) == lib.ERR_ARG, args
    with look.Look(*LOOKS[list(LOOKS)[0]]) as lk, look.Look16(*LOOKS16[list(LOOKS16)[0]]) as lk16:
        for fn, handle, bpx in ((gpu.mlvfs_amd_render_resampled_look_dev, lk.h, 3), (gpu.mlvfs_amd_render_resampled_deep_dev, lk16.h, 6)):
            call = lambda sp, w, h, ow, oh, dp_, ost, n, l: fn(vp(sp), 512, w, h, vp(p), ow, oh, vp(dp_), ost, n, vp(l), None)
            for args in ((s, 32, 8, 20, 5, d, 1024, 1, 0), (0, 32, 8, 20, 5, d, 1024, 1, handle), (s, 32, 8, 33, 5, d, 1024, 1, handle),
                         (s, 32, 8, 20, 9, d, 1024, 1, handle), (s, 32, 3, 20, 1, d, 1024, 1, handle), (s, 32, 8, 20, 5, d, 100 * bpx - 1, 2, handle),
                         (d + 1024, 32, 8, 20, 5, d + 1024, 1024, 1, handle)):
                assert call(*args) == lib.ERR_ARG, (bpx, args)
            assert call(s, 32, 8, 20, 5, d, 1024, 0, handle) == 0               # nothing to do is no error
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert plain(s, 512, 32, 8, p, 20, 5, d, 304, 0) == 0
    assert plain(d + 1024, 512, 32, 8, p, 20, 5, d + 1024 + 512, 304, 1) == 0   # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1536] == PAD).all() and (host[1536 + 300:] == PAD).all()
    want = resample.render(np.full((8, 32), PAD | PAD << 8, np.uint16), rc.param_set(0)[1], 20, 5)
    assert np.array_equal(host[1536:1536 + 300].reshape(5, 20, 3), want)
    ow, oh = C.c_int(-7), C.c_int(-7)
    assert gpu.mlvfs_amd_rgb_fit_full(32, 8, 20, 20, C.byref(ow), C.byref(oh)) == 0 and (ow.value, oh.value) == (20, 5)
