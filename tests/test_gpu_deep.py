"""Rendered frames at 16 bits on the GPU (csrc/k_tone_dev.h, csrc/look.cpp): the six deep kernels and k_look16_apply
against the numpy definition, for equality.  mlvfs_amd_look16_apply_dev -- step 4 alone -- on the chosen triples of tests/look_cases.py
and on 100 000 random ones per look; mlvfs_amd_render2_deep_dev at the shapes of tests/deep_cases.py (the x16 kernel at 16 x 2, 32 x 4
and 48 x 6 as three frames at padded strides; the generic kernel at 2 x 2, 3 x 3, 18 x 6 and at 32 x 4 with the source, or the
destination, off the fast form's alignment -- the same samples as the fast form gives); mlvfs_amd_render1_deep_dev and
mlvfs_amd_render_scaled_deep_dev at the shapes with which tests/demosaic_cases.py and tests/scale_cases.py reach their kernels'
borders, strip seams and band seams; the scaled route at the half size against the half-size route; every refusal.  Bytes between and
behind the renderings, and the sources, stay what they were."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import lib, look

import deep_cases as dp
import demosaic_cases as dc
import look_cases as lc
import render_cases as rc
import scale_cases as sc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
LOOKS = {name: (S, n, T) for name, S, n, T in dp.looks()}


@pytest.fixture(scope="module")
def handles(gpu):
    """the deep looks of tests/deep_cases.py on the device, each created at its first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = look.Look16(*LOOKS[name])
        return made[name]
    yield get
    for lk in made.values():
        lk.close()


def up16(v):
    return (v + 15) // 16 * 16


def apply_dev(gpu, lk, t, dst_off=0):
    """t (3, count) -> (samples (3, count), every other byte of the destination)"""
    import torch
    count = t.shape[1]
    src = torch.from_numpy(np.ascontiguousarray(t.T).astype(np.uint16).view(np.int16)).cuda()
    before = src.clone()
    dst = device_buffer(torch, [np.full(6 * count, PAD, np.uint8)], 6 * count, dst_off)
    lib.check(gpu.mlvfs_amd_look16_apply_dev(C.c_void_p(lk.h), C.c_void_p(src.data_ptr()), count, C.c_void_p(dst.data_ptr() + dst_off), None),
              "look16_apply_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the indices changed"
    parts, rest = split(dst, 1, 6 * count, 6 * count, dst_off)
    return parts[0].view("<u2").reshape(count, 3).T, rest


@pytest.mark.parametrize("name", list(LOOKS))
def test_look16_apply_dev_equals_numpy(gpu, handles, name):
    S, n, T = LOOKS[name]
    lk = handles(name)
    for t, off in ((lc.case_triples(), 0), (dp.random_triples16(100000, n), 2)):
        got, rest = apply_dev(gpu, lk, t, off)
        want = look.apply16(t, S, n, T)
        assert (rest == PAD).all() and np.array_equal(got, want), (name, off, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def run_deep(gpu, route, frames, params, lk, src_off, dst_off, aligned, size=None):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings (oh, ow, 3) uint16, every other byte
    of the destination).  route: 2 half size, 1 full size, 0 scaled to `size`"""
    import torch
    h, w = frames[0].shape
    ow, oh = (w // 2, h // 2) if route == 2 else (w, h) if route == 1 else size
    n, img, pimg = len(frames), w * h * 2, ow * oh * 6
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(rc.params_array(params)).cuda()
    s, d, p = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off), C.c_void_p(par.data_ptr())
    if route == 2:
        rc_ = gpu.mlvfs_amd_render2_deep_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(lk.h), None)
    elif route == 1:
        rc_ = gpu.mlvfs_amd_render1_deep_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(lk.h), None)
    else:
        rc_ = gpu.mlvfs_amd_render_scaled_deep_dev(s, stride, w, h, p, ow, oh, d, ostride, n, C.c_void_p(lk.h), None)
    lib.check(rc_, "render_deep_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)            # the canary bytes between and behind the frames are `rest`
    return [np.frombuffer(q.tobytes(), "<u2").reshape(oh, ow, 3) for q in parts], rest


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


def check(gpu, handles, route, batch, src_off, dst_off, aligned, name, size=None):
    frames, params = [f for f, _ in batch], [p for _, p in batch]
    got, rest = run_deep(gpu, route, frames, params, handles(name), src_off, dst_off, aligned, size)
    assert (rest == PAD).all(), (name, len(batch), src_off, dst_off, "bytes outside the renderings changed")
    for k, (f, p) in enumerate(batch):
        want = dp.definition(route, f, p, LOOKS[name], size)
        assert np.array_equal(got[k], want), (route, f.shape, size, name, len(batch), src_off, dst_off, k, where(got[k], want))
    return got


HALF = dp.half_cases()


@pytest.mark.parametrize("k", range(len(HALF)), ids=["%dx%d:%d:+%d:+%d:%s" % (c[0][0][0].shape[1], c[0][0][0].shape[0], len(c[0]), c[1], c[2], c[4]) for c in HALF])
def test_render2_deep_dev_equals_numpy(gpu, handles, k):
    check(gpu, handles, 2, *HALF[k])


def test_render2_deep_generic_agrees_with_the_fast_form(gpu, handles):
    """32 x 4 on the fast form's alignment, with the source base off a 16-byte boundary, and with the destination base 8 bytes off one:
    the same samples"""
    batch = dp.batch(32, 4, 1, 4)
    outs = [check(gpu, handles, 2, batch, so, do, True, "random65")[0] for so, do in ((0, 0), (2, 0), (0, 8), (16, 16))]
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])


def test_the_linear_file_holds_t_and_a_constant_shaper_a_constant(gpu, handles):
    f, p = dp.rounding_frame()
    for do in (0, 8):
        got, = check(gpu, handles, 2, [(f, p)], 0, do, True, "linear0")
        assert got[0, :4, 0].tolist() == [0, 1, 1, 2] and got[0, :4, 2].tolist() == [1, 0, 2, 1]      # 2047 | 2048, 6143 | 6144
        got, = check(gpu, handles, 2, [(f, p)], 0, do, True, "const0")
        assert (got == 12345).all()


@pytest.mark.parametrize("w,h", dc.SIZES, ids=lambda v: str(v))
def test_render1_deep_dev_equals_numpy(gpu, handles, w, h):
    for case in dp.full_cases(w, h):
        check(gpu, handles, 1, *case)


@pytest.mark.parametrize("w,h", sc.SOURCES, ids=lambda v: str(v))
def test_render_scaled_deep_dev_equals_numpy(gpu, handles, w, h):
    for ow, oh, batch, so, do, al, name in dp.scaled_cases(w, h):
        check(gpu, handles, 0, batch, so, do, al, name, (ow, oh))


@pytest.mark.parametrize("w,h", [(32, 8), (48, 6), (418, 266)], ids=lambda v: str(v))
def test_the_scaled_route_at_the_half_size_is_the_half_size_route(gpu, handles, w, h):
    batch = dp.batch(w, h, 3, w)
    for name in ("case0", "random3"):
        half = check(gpu, handles, 2, batch, 0, 0, True, name)
        scaled = check(gpu, handles, 0, batch, 0, 0, True, name, (w // 2, h // 2))
        assert all(np.array_equal(a, b) for a, b in zip(half, scaled))


def test_a_look_destroyed_and_another_created_between_two_calls(gpu):
    batch = dp.batch(48, 6, 3, 0)
    frames, params = [f for f, _ in batch], [p for _, p in batch]
    for name in ("random65", "linear0", "random3", "const0"):     # each handle is gone before the next is made: the same memory may serve again
        with look.Look16(*LOOKS[name]) as lk:
            got, rest = run_deep(gpu, 2, frames, params, lk, 0, 0, True)
        assert lk.h is None and (rest == PAD).all()
        for k, (f, p) in enumerate(batch):
            assert np.array_equal(got[k], dp.definition(2, f, p, LOOKS[name])), (name, k)
    lk.close()                                                   # a second close is nothing


def test_deep_dev_refusals_leave_the_destination(gpu, handles):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(rc.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p, lk = src.data_ptr(), dst.data_ptr(), par.data_ptr(), handles("random3").h
    vp = lambda a: C.c_void_p(a) if a else None
    r2 = lambda sp, st, w, h, pp, dp_, ost, n, l: gpu.mlvfs_amd_render2_deep_dev(vp(sp), st, w, h, vp(pp), vp(dp_), ost, n, vp(l), None)
    r1 = lambda sp, st, w, h, pp, dp_, ost, n, l: gpu.mlvfs_amd_render1_deep_dev(vp(sp), st, w, h, vp(pp), vp(dp_), ost, n, vp(l), None)
    rs = lambda sp, st, w, h, pp, dp_, ost, n, l: gpu.mlvfs_amd_render_scaled_deep_dev(vp(sp), st, w, h, vp(pp), 7, 3, vp(dp_), ost, n, vp(l), None)
    # a 32 x 8 frame: 512 bytes in; 384, 1536 or 126 bytes out
    bad = [(s, 512, 32, 8, p, d, 2048, 1, 0), (0, 512, 32, 8, p, d, 2048, 1, lk), (s, 512, 32, 8, 0, d, 2048, 1, lk), (s, 512, 32, 8, p, 0, 2048, 1, lk),
           (s, 512, 1, 8, p, d, 2048, 1, lk), (s, 512, 32, 1, p, d, 2048, 1, lk), (s, 512, 1 << 14, 1 << 13, p, d, 2048, 1, lk), (s, 512, -32, 8, p, d, 2048, 1, lk),
           (s, 512, 32, 8, p, d, 2048, -1, lk), (s, 510, 32, 8, p, d, 2048, 2, lk), (s, 512, 32, 8, p, d, 100, 2, lk), (s, 513, 32, 8, p, d, 2048, 2, lk),
           (s + 1, 512, 32, 8, p, d, 2048, 1, lk), (s, 512, 32, 8, p + 2, d, 2048, 1, lk),
           (d + 2048, 512, 32, 8, p, d + 2048, 2048, 1, lk), (d + 2048, 512, 32, 8, p, d + 2048 + 511, 2048, 1, lk), (d + 2048, 512, 32, 8, p, d + 2048 - 125, 2048, 1, lk),
           (s, 512, 32, 8, d + 32, d, 2048, 1, lk)]
    for call in (r2, r1, rs):
        for args in bad:
            assert call(*args) == lib.ERR_ARG, args
    # the stride checks use 6 bytes per pixel: what holds an 8-bit rendering does not hold this one
    assert r2(s, 512, 32, 8, p, d, 383, 2, lk) == lib.ERR_ARG and r1(s, 512, 32, 8, p, d, 1535, 2, lk) == lib.ERR_ARG
    assert rs(s, 512, 32, 8, p, d, 125, 2, lk) == lib.ERR_ARG
    t = torch.zeros(64, dtype=torch.int16, device="cuda").data_ptr()
    ap = lambda l, tp, n, dp_: gpu.mlvfs_amd_look16_apply_dev(vp(l), vp(tp), n, vp(dp_), None)
    for args in ((0, t, 8, d), (lk, 0, 8, d), (lk, t, 8, 0), (lk, t + 1, 8, d), (lk, t, 8, d + 1), (lk, d + 64, 8, d + 64), (lk, d + 64, 8, d + 64 + 46),
                 (lk, d + 64, 8, d + 64 - 46)):
        assert ap(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert r2(d + 2048, 512, 32, 8, p, d + 2048 + 512, 2048, 1, lk) == 0         # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:2560] == PAD).all() and (host[2560 + 384:] == PAD).all()
    want = dp.definition(2, np.full((8, 32), PAD | PAD << 8, np.uint16), rc.param_set(0)[1], LOOKS["random3"])
    assert host[2560:2560 + 384].tobytes() == dp.file_bytes(want)
