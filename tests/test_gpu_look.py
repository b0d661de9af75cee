"""A look for the rendered frames on the GPU (csrc/k_tone_dev.h, csrc/look.cpp): mlvfs_amd_look_apply_dev -- step 4 alone
-- on the chosen triples of tests/look_cases.py and on 100 000 random ones against the numpy definition of mlvfs_amd/look.py, at N = 2,
3, 17, 33 and 65, behind random, all-zero and all-65535 tables and a shaper that is not monotone; then mlvfs_amd_render2_look_dev,
mlvfs_amd_render1_look_dev and mlvfs_amd_render_scaled_look_dev against the definition at the smallest shapes that reach each form,
in batches of 1 and 3 with different parameters per frame (both matrix paths in one batch), padded strides, aligned and misaligned
bases (so that each x16 kernel and each generic kernel runs wherever either could), one look per launch; the identity look against
the plain calls; a look destroyed and another created between two calls; every refusal; one 3584 x 1320 frame per route.  All
comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, look, render, scale

import look_cases as lc
import render_cases as rc
from test_gpu_demosaic import run_render1
from test_gpu_mlv_transcode import PAD, device_buffer, split
from test_gpu_render import run_render2
from test_gpu_scale import run_scaled

pytestmark = pytest.mark.gpu
LOOKS = {name: (S, n, T) for name, S, n, T in lc.looks()}


@pytest.fixture(scope="module")
def handles(gpu):
    """the looks of tests/look_cases.py on the device, each created at its first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = look.Look(*LOOKS[name])
        return made[name]
    yield get
    for lk in made.values():
        lk.close()


def up16(v):
    return (v + 15) // 16 * 16


def apply_dev(gpu, lk, t, dst_off=0):
    """t (3, count) -> (bytes (3, count), every other byte of the destination)"""
    import torch
    count = t.shape[1]
    src = torch.from_numpy(np.ascontiguousarray(t.T).astype(np.uint16).view(np.int16)).cuda()
    before = src.clone()
    dst = device_buffer(torch, [np.full(3 * count, PAD, np.uint8)], 3 * count, dst_off)
    lib.check(gpu.mlvfs_amd_look_apply_dev(C.c_void_p(lk.h), C.c_void_p(src.data_ptr()), count, C.c_void_p(dst.data_ptr() + dst_off), None), "look_apply_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the indices changed"
    parts, rest = split(dst, 1, 3 * count, 3 * count, dst_off)
    return parts[0].reshape(count, 3).T, rest


@pytest.mark.parametrize("name", list(LOOKS))
def test_look_apply_dev_equals_numpy(gpu, handles, name):
    S, n, T = LOOKS[name]
    lk = handles(name)
    for t, off in ((lc.case_triples(), 0), (lc.random_triples(100000, n), 1)):
        got, rest = apply_dev(gpu, lk, t, off)
        want = look.apply(t, S, n, T)
        assert (rest == PAD).all() and np.array_equal(got, want), (name, off, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    t = lc.case_triples()[:, :999]                               # bits above the twelfth are masked
    got, _ = apply_dev(gpu, lk, t | 0xF000)
    assert np.array_equal(got, look.apply(t, S, n, T))


def run_look(gpu, route, frames, params, lk, src_off, dst_off, aligned, size=None):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination).
    route: 2 half size, 1 full size, 0 scaled to `size`"""
    import torch
    h, w = frames[0].shape
    ow, oh = (w // 2, h // 2) if route == 2 else (w, h) if route == 1 else size
    n, img, pimg = len(frames), w * h * 2, ow * oh * 3
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(rc.params_array(params)).cuda()
    s, d, p = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off), C.c_void_p(par.data_ptr())
    if route == 2:
        rc_ = gpu.mlvfs_amd_render2_look_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(lk.h), None)
    elif route == 1:
        rc_ = gpu.mlvfs_amd_render1_look_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(lk.h), None)
    else:
        rc_ = gpu.mlvfs_amd_render_scaled_look_dev(s, stride, w, h, p, ow, oh, d, ostride, n, C.c_void_p(lk.h), None)
    lib.check(rc_, "render_look_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [q.reshape(oh, ow, 3) for q in parts], rest


def definition(route, f, p, lk, size=None):
    if route == 2:
        return render.render(f, p, look=lk)
    if route == 1:
        return demosaic.render(f, p, look=lk)
    return scale.render(f, p, size[0], size[1], look=lk)


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


def check_route(gpu, handles, route, w, h, size=None):
    for batch, src_off, dst_off, aligned, name in lc.frame_cases(w, h, first=route):
        frames, params = [f for f, _ in batch], [p for _, p in batch]
        got, rest = run_look(gpu, route, frames, params, handles(name), src_off, dst_off, aligned, size)
        assert (rest == PAD).all(), (name, len(batch), src_off, dst_off, "bytes outside the renderings changed")
        for k, (f, p) in enumerate(batch):
            want = definition(route, f, p, LOOKS[name], size)
            assert np.array_equal(got[k], want), (name, len(batch), src_off, dst_off, k, where(got[k], want))


@pytest.mark.parametrize("w,h", lc.HALF_SIZES, ids=lambda v: str(v))
def test_render2_look_dev_equals_numpy(gpu, handles, w, h):
    check_route(gpu, handles, 2, w, h)


@pytest.mark.parametrize("w,h", lc.FULL_SIZES, ids=lambda v: str(v))
def test_render1_look_dev_equals_numpy(gpu, handles, w, h):
    check_route(gpu, handles, 1, w, h)


@pytest.mark.parametrize("src,size", lc.SCALED_SIZES, ids=lambda v: str(v))
def test_render_scaled_look_dev_equals_numpy(gpu, handles, src, size):
    check_route(gpu, handles, 0, src[0], src[1], size)


def test_the_identity_look_reproduces_the_plain_calls(gpu):
    """S = 257 LUT and the identity table: the plain kernels' bytes from the look kernels, through both forms of every route"""
    with look.Look(look.shaper_srgb(), 17, look.identity(17)) as i17, look.Look(look.shaper_srgb(), 2, look.identity(2)) as i2:
        for (n, src_off, dst_off, aligned), lk in zip(lc.PLACEMENTS[:2], (i17, i2)):
            batch = rc.batch(48, 8, n, 5)
            frames, params = [f for f, _ in batch], [p for _, p in batch]
            for route, plain, size in ((2, run_render2, None), (1, run_render1, None), (0, None, (7, 3))):
                got, rest = run_look(gpu, route, frames, params, lk, src_off, dst_off, aligned, size)
                if route:
                    want, _ = plain(gpu, frames, params, src_off, dst_off, aligned)
                else:
                    want, _ = run_scaled(gpu, frames, params, 7, 3, src_off, dst_off, aligned)
                assert (rest == PAD).all()
                for k in range(n):
                    assert np.array_equal(got[k], want[k]), (route, aligned, k, where(got[k], want[k]))


def test_a_look_destroyed_and_another_created_between_two_calls(gpu):
    (batch, src_off, dst_off, aligned, _), = lc.frame_cases(48, 4)[:1]
    frames, params = [f for f, _ in batch], [p for _, p in batch]
    for name in ("random33", "random3", "linear33", "zero3"):    # each handle is gone before the next is made: the same memory may serve again
        with look.Look(*LOOKS[name]) as lk:
            got, rest = run_look(gpu, 2, frames, params, lk, src_off, dst_off, aligned)
        assert lk.h is None and (rest == PAD).all()
        for k, (f, p) in enumerate(batch):
            assert np.array_equal(got[k], render.render(f, p, look=LOOKS[name])), (name, k)
    lk.close()                                                   # a second close is nothing


def test_look_dev_refusals_leave_the_destination(gpu, handles):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(rc.params_array([rc.param_set(k)[1] for k in range(3)])).cuda()
    s, d, p, lk = src.data_ptr(), dst.data_ptr(), par.data_ptr(), handles("random17").h
    vp = lambda a: C.c_void_p(a) if a else None
    r2 = lambda sp, st, w, h, pp, dp, ost, n, l: gpu.mlvfs_amd_render2_look_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(l), None)
    r1 = lambda sp, st, w, h, pp, dp, ost, n, l: gpu.mlvfs_amd_render1_look_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(l), None)
    rs = lambda sp, st, w, h, pp, dp, ost, n, l: gpu.mlvfs_amd_render_scaled_look_dev(vp(sp), st, w, h, vp(pp), 7, 3, vp(dp), ost, n, vp(l), None)
    # a 32 x 8 frame: 512 bytes in; 192, 768 or 63 bytes out
    bad = [(s, 512, 32, 8, p, d, 1024, 1, 0), (0, 512, 32, 8, p, d, 1024, 1, lk), (s, 512, 32, 8, 0, d, 1024, 1, lk), (s, 512, 32, 8, p, 0, 1024, 1, lk),
           (s, 512, 1, 8, p, d, 1024, 1, lk), (s, 512, 32, 1, p, d, 1024, 1, lk), (s, 512, 1 << 14, 1 << 13, p, d, 1024, 1, lk), (s, 512, -32, 8, p, d, 1024, 1, lk),
           (s, 512, 32, 8, p, d, 1024, -1, lk), (s, 510, 32, 8, p, d, 1024, 2, lk), (s, 512, 32, 8, p, d, 40, 2, lk), (s, 513, 32, 8, p, d, 1024, 2, lk),
           (s + 1, 512, 32, 8, p, d, 1024, 1, lk), (s, 512, 32, 8, p + 2, d, 1024, 1, lk),
           (d + 1024, 512, 32, 8, p, d + 1024, 1024, 1, lk), (d + 1024, 512, 32, 8, p, d + 1024 + 511, 1024, 1, lk), (d + 1024, 512, 32, 8, p, d + 1024 - 62, 1024, 1, lk),
           (s, 512, 32, 8, d + 32, d, 1024, 1, lk)]
    for call in (r2, r1, rs):
        for args in bad:
            assert call(*args) == lib.ERR_ARG, args
    for ow, oh in ((0, 3), (7, 0), (17, 3), (7, 5)):
        assert gpu.mlvfs_amd_render_scaled_look_dev(vp(s), 512, 32, 8, vp(p), ow, oh, vp(d), 1024, 1, vp(lk), None) == lib.ERR_ARG
    assert r1(s, 512, 2, 2, p, d, 1024, 1, lk) == lib.ERR_ARG
    t = torch.zeros(64, dtype=torch.int16, device="cuda").data_ptr()
    ap = lambda l, tp, n, dp: gpu.mlvfs_amd_look_apply_dev(vp(l), vp(tp), n, vp(dp), None)
    for args in ((0, t, 8, d), (lk, 0, 8, d), (lk, t, 8, 0), (lk, t + 1, 8, d), (lk, d + 64, 8, d + 64), (lk, d + 64, 8, d + 64 + 47), (lk, d + 64, 8, d + 64 - 23)):
        assert ap(*args) == lib.ERR_ARG, args
    assert gpu.mlvfs_amd_mount_set_look(None, vp(lk)) == lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert r2(d + 1024, 512, 32, 8, p, d + 1024 + 512, 1024, 1, lk) == 0         # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1536] == PAD).all() and (host[1536 + 192:] == PAD).all()
    want = render.render(np.full((8, 32), PAD | PAD << 8, np.uint16), rc.param_set(0)[1], look=LOOKS["random17"])
    assert np.array_equal(host[1536:1536 + 192].reshape(4, 16, 3), want)


@pytest.mark.parametrize("route,size", [(2, None), (0, (1280, 472)), (1, None)], ids=["half", "1280x472", "full"])
def test_look_dev_at_3584x1320(gpu, handles, route, size):
    """one frame per route at the bench's size, with a 33^3 table as the bench has it"""
    (b0, w0), p0 = rc.param_set(2)
    f = rc.range_frame(lc.BIG_W, lc.BIG_H, b0, w0, seed=1)
    name = "linear33"
    got, rest = run_look(gpu, route, [f], [p0], handles(name), 0, 0, True, size)
    want = definition(route, f, p0, LOOKS[name], size)
    assert (rest == PAD).all() and np.array_equal(got[0], want), (route, where(got[0], want))
