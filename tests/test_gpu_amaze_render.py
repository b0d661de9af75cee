"""Rendered full-size frames demosaiced by AMaZE on the GPU (csrc/k_amaze_render.hip, csrc/amaze_render.cpp), against
the definition of mlvfs_amd/amaze_render.py with the checker's AMaZE, for equality: mlvfs_amd_amaze_balance_dev against float32(b);
mlvfs_amd_amaze_tone_dev on crafted planes and on the checker's planes in the three tone forms and both matrix paths; the three
mlvfs_amd_render1_amaze calls end to end at the sizes of tests/amaze_render_cases.py -- batches of 1 and 3 with parameters of their own,
padded strides, aligned and misaligned bases (the fast and the generic forms), the bytes around the renderings and the source
unchanged --; geometries in turn on one thread, with the dual-ISO route's AMaZE call in between; a failed growth of the work memory;
one 3584 x 1320 frame; every refusal."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import amaze_render, lib, look, render

import amaze_render_cases as ac
import deep_cases as dc
import demosaic_cases as dm
import look_cases as lc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
FORMS = ("plain", "look", "deep")
LOOK, LOOK16 = lc.look_of("random17"), dc.look_of("random3")
BPX = {"plain": 3, "look": 3, "deep": 6}


@pytest.fixture(scope="module")
def handles(gpu):
    made = {"plain": None, "look": look.Look(*LOOK), "deep": look.Look16(*LOOK16)}
    yield made
    for lk in made.values():
        if lk is not None:
            lk.close()


def up16(v):
    return (v + 15) // 16 * 16


def develop(form, t, t16):
    """step 4 of one form on the definition's indices -> (H, W, 3)"""
    if form == "deep":
        return np.ascontiguousarray(look.apply16(t16, *LOOK16).transpose(1, 2, 0)).astype(np.uint16)
    return render.tone(t, look=LOOK if form == "look" else None)


def as_pixels(form, part, w, h):
    return np.frombuffer(part.tobytes(), "<u2").reshape(h, w, 3) if form == "deep" else part.reshape(h, w, 3)


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


def run_render1(gpu, handles, form, frames, params, src_off, dst_off, aligned):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    n, img, pimg = len(frames), w * h * 2, w * h * BPX[form]
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(ac.params_array(params)).cuda()
    s, d, p = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off), C.c_void_p(par.data_ptr())
    if form == "plain":
        rc = gpu.mlvfs_amd_render1_amaze_dev(s, stride, w, h, p, d, ostride, n, None)
    elif form == "look":
        rc = gpu.mlvfs_amd_render1_amaze_look_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(handles["look"].h), None)
    else:
        rc = gpu.mlvfs_amd_render1_amaze_deep_dev(s, stride, w, h, p, d, ostride, n, C.c_void_p(handles["deep"].h), None)
    lib.check(rc, "render1_amaze_" + form)
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [as_pixels(form, q, w, h) for q in parts], rest


def end_to_end(gpu, oracle, handles, w, h, forms=FORMS, placements=ac.PLACEMENTS):
    batch = ac.batch(w, h, 3, first=(w + h) % 4)
    staged = [amaze_render.stages(f, p, oracle.amaze_demosaic) for f, p in batch]
    for form in forms:
        want = [develop(form, st["t"], st["t16"]) for st in staged]
        for n, src_off, dst_off, aligned in placements:
            got, rest = run_render1(gpu, handles, form, [f for f, _ in batch[:n]], [p for _, p in batch[:n]], src_off, dst_off, aligned)
            assert (rest == PAD).all(), (form, n, src_off, dst_off, "bytes outside the renderings changed")
            for k in range(n):
                assert np.array_equal(got[k], want[k]), (w, h, form, n, src_off, dst_off, k, where(got[k], want[k]))


@pytest.mark.parametrize("w,h", ac.SIZES + [ac.FAST_SIZE], ids=lambda v: str(v))
def test_render1_amaze_equals_the_definition(gpu, oracle, handles, w, h):
    end_to_end(gpu, oracle, handles, w, h)


def test_render1_amaze_with_a_complete_tile(gpu, oracle, handles):
    w, h, nfx, nfy = ac.rows_size()
    assert nfx * nfy == 1                                         # k_amaze_rows runs
    end_to_end(gpu, oracle, handles, w, h)


@pytest.mark.parametrize("w,h", ac.SIZES + [ac.FAST_SIZE], ids=lambda v: str(v))
def test_amaze_balance_dev_is_float32_of_b(gpu, w, h):
    import torch
    from mlvfs_amd import demosaic
    batch = ac.batch(w, h, 3)
    want = [demosaic.stages(f, p)["b"].astype(np.float32) for f, p in batch]
    npix, img = w * h, w * h * 2
    for n, src_off, pl_off, aligned in ((1, 0, 0, True), (3, 0, 0, True), (3, 16, 16, True), (3, 2, 4, False), (1, 0, 4, False)):
        stride, pstride = (up16(img) + 32, (npix + 3) // 4 * 4 + 8) if aligned else (img + 6, npix + 1)
        src = device_buffer(torch, [f for f, _ in batch[:n]], stride, src_off)
        before = src.clone()
        dst = device_buffer(torch, [np.full(4 * npix, PAD, np.uint8)] * n, 4 * pstride, pl_off)
        par = torch.from_numpy(ac.params_array([p for _, p in batch[:n]])).cuda()
        lib.check(gpu.mlvfs_amd_amaze_balance_dev(C.c_void_p(src.data_ptr() + src_off), stride, w, h, C.c_void_p(par.data_ptr()),
                                                  C.c_void_p(dst.data_ptr() + pl_off), pstride, n, None), "amaze_balance_dev")
        torch.cuda.synchronize()
        assert torch.equal(src, before), "the source changed"
        parts, rest = split(dst, n, 4 * pstride, 4 * npix, pl_off)
        assert (rest == PAD).all(), (n, src_off, pl_off)
        for k in range(n):
            got = np.frombuffer(parts[k].tobytes(), np.float32).reshape(h, w)
            assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)), (n, src_off, pl_off, k, int((got != want[k]).sum()))


def run_tone(gpu, handles, form, planes, params, pl_off, dst_off, aligned):
    """planes: per frame (3, H, W) float32 -> (renderings, every other byte of the destination); the planes lie as three batches"""
    import torch
    n, (_, h, w) = len(planes), planes[0].shape
    npix, pimg = w * h, w * h * BPX[form]
    pstride, ostride = ((npix + 3) // 4 * 4 + 8, up16(pimg) + 16) if aligned else (npix + 1, pimg + 5)
    bufs = [device_buffer(torch, [np.ascontiguousarray(pl[c]) for pl in planes], 4 * pstride, pl_off) for c in range(3)]
    before = [b.clone() for b in bufs]
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(ac.params_array(params)).cuda()
    lk = None if form != "look" else C.c_void_p(handles["look"].h)
    lk16 = None if form != "deep" else C.c_void_p(handles["deep"].h)
    lib.check(gpu.mlvfs_amd_amaze_tone_dev(*[C.c_void_p(b.data_ptr() + pl_off) for b in bufs], pstride, w, h, C.c_void_p(par.data_ptr()),
                                           C.c_void_p(dst.data_ptr() + dst_off), ostride, n, lk, lk16, None), "amaze_tone_dev")
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.uint8), b0.view(torch.uint8)), "a plane changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [as_pixels(form, q, w, h) for q in parts], rest


TONE_PLACEMENTS = [(0, 0, True), (16, 16, True), (4, 1, False), (0, 8, True)]       # the last: aligned for 8 bits, not for the deep form


@pytest.mark.parametrize("form", FORMS)
def test_amaze_tone_dev_on_crafted_planes(gpu, handles, form):
    """NaN, the infinities, -0.0, k + 0.5, the neighbourhood of both clamps and 0.49999997 in every channel, through both matrix paths"""
    sets = [dm.param_set(0)[1], dm.param_set(1)[1], ac.wide_set()[1]]
    assert [ac.matrix_fits_32(p) for p in sets] == [True, False, False]
    for w, h in (ac.FAST_SIZE, (36, 36)):
        planes, n = ac.crafted_planes(w, h)
        want = [develop(form, *ac.matrix(p, n)) for p in sets]
        for pl_off, dst_off, aligned in TONE_PLACEMENTS:
            got, rest = run_tone(gpu, handles, form, [planes] * 3, sets, pl_off, dst_off, aligned)
            assert (rest == PAD).all(), (w, h, pl_off, dst_off)
            for k in range(3):
                assert np.array_equal(got[k], want[k]), (w, h, form, pl_off, dst_off, k, where(got[k], want[k]))


@pytest.mark.parametrize("form", FORMS)
def test_amaze_tone_dev_on_the_checkers_planes(gpu, oracle, handles, form):
    for w, h in (ac.FAST_SIZE, (164, 148)):
        batch = ac.batch(w, h, 3)
        staged = [amaze_render.stages(f, p, oracle.amaze_demosaic) for f, p in batch]
        assert [ac.matrix_fits_32(p) for _, p in batch] == [True, False, True]
        for pl_off, dst_off, aligned in TONE_PLACEMENTS[:3]:
            got, rest = run_tone(gpu, handles, form, [st["planes"] for st in staged], [p for _, p in batch], pl_off, dst_off, aligned)
            assert (rest == PAD).all()
            for k, st in enumerate(staged):
                want = develop(form, st["t"], st["t16"])
                assert np.array_equal(got[k], want), (w, h, form, pl_off, dst_off, k, where(got[k], want))


def test_geometries_in_turn_on_one_thread(gpu, oracle, handles):
    """the tile planes are zeroed when the geometry changes: a plane of another size in between -- through this route, and through the
    dual-ISO route's AMaZE call, which has tile planes of its own -- leaves nothing behind that the first geometry could read"""
    import torch
    one = [(1, 0, 0, True)]
    a, b = (164, 148), (292, 36)
    end_to_end(gpu, oracle, handles, *a, forms=("plain",), placements=one)
    end_to_end(gpu, oracle, handles, *b, forms=("plain",), placements=one)
    end_to_end(gpu, oracle, handles, *a, forms=("plain",), placements=one)
    w, h = 148, 40
    raw = torch.from_numpy(dm.speckle_frame(w, h, 2048, 15000).astype(np.float32)).cuda()
    out = [torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
    lib.check(gpu.mlvfs_amd_amaze_demosaic_dev(C.c_void_p(raw.data_ptr()), w, h, *[C.c_void_p(o.data_ptr()) for o in out], None), "amaze_demosaic_dev")
    torch.cuda.synchronize()
    want = oracle.amaze_demosaic(raw.cpu().numpy())
    end_to_end(gpu, oracle, handles, *a, forms=("deep",), placements=[(3, 0, 0, True)])
    lib.check(gpu.mlvfs_amd_amaze_demosaic_dev(C.c_void_p(raw.data_ptr()), w, h, *[C.c_void_p(o.data_ptr()) for o in out], None), "amaze_demosaic_dev")
    torch.cuda.synchronize()
    for g, x in zip(out, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), x.view(np.uint32))


def test_a_failed_growth_of_the_work_memory_halves_the_sub_batch(gpu, oracle, handles):
    """mlvfs_amd_test_fail_next(3) fails the next growth of a device buffer: with the thread's work memory given back that is the
    planes of a batch of 3, which then goes as 2 + 1 and renders what it always renders; a single frame whose work memory cannot be
    had is an error, and the call after it serves again"""
    import torch
    w, h = 148, 40
    gpu.mlvfs_amd_dualiso_trim()
    gpu.mlvfs_amd_test_fail_next(3)
    end_to_end(gpu, oracle, handles, w, h, forms=("plain",), placements=[(3, 0, 0, True)])
    gpu.mlvfs_amd_dualiso_trim()
    (f, p), = ac.batch(w, h, 1)
    src = torch.from_numpy(f.view(np.int16)).cuda()
    dst = torch.full((w * h * 3,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(ac.params_array([p])).cuda()
    gpu.mlvfs_amd_test_fail_next(3)
    assert gpu.mlvfs_amd_render1_amaze_dev(C.c_void_p(src.data_ptr()), w * h * 2, w, h, C.c_void_p(par.data_ptr()), C.c_void_p(dst.data_ptr()),
                                           w * h * 3, 1, None) == lib.ERR_HIP and b"injected" in gpu.mlvfs_amd_last_error()
    torch.cuda.synchronize()
    assert bool((dst == PAD).all())
    end_to_end(gpu, oracle, handles, w, h, forms=("look",), placements=[(3, 0, 0, True)])


def test_render1_amaze_full_size(gpu, oracle, handles):
    (b0, w0), p0 = dm.param_set(2)
    f = dm.speckle_frame(ac.BIG_W, ac.BIG_H, b0, w0)
    st = amaze_render.stages(f, p0, oracle.amaze_demosaic)
    got, rest = run_render1(gpu, handles, "plain", [f], [p0], 0, 0, True)
    want = develop("plain", st["t"], st["t16"])
    assert (rest == PAD).all() and np.array_equal(got[0], want), where(got[0], want)


def test_refusals_leave_the_destination(gpu, handles):
    import torch
    W, H, IMG, NP, OUT = 48, 36, 3456, 1728, 5184
    src = torch.full((3 * IMG + 64,), 7, dtype=torch.uint8, device="cuda")
    pl = torch.zeros((9 * NP + 16,), dtype=torch.float32, device="cuda")
    dst = torch.full((6 * OUT + 64,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(ac.params_array([dm.param_set(k)[1] for k in range(3)])).cuda()
    s, q, d, p = src.data_ptr(), pl.data_ptr(), dst.data_ptr(), par.data_ptr()
    qr, qg, qb = q, q + 12 * NP, q + 24 * NP
    L, L16 = handles["look"].h, handles["deep"].h
    vp = lambda a: C.c_void_p(a) if a else None
    bal = lambda sp, st, w, h, pp, qp, ps, n: gpu.mlvfs_amd_amaze_balance_dev(vp(sp), st, w, h, vp(pp), vp(qp), ps, n, None)
    tone = lambda r, g, b, ps, w, h, pp, dp, ost, n, l=0, l16=0: gpu.mlvfs_amd_amaze_tone_dev(vp(r), vp(g), vp(b), ps, w, h, vp(pp), vp(dp), ost, n, vp(l), vp(l16), None)
    r1 = lambda sp, st, w, h, pp, dp, ost, n: gpu.mlvfs_amd_render1_amaze_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, None)
    r1l = lambda sp, st, w, h, pp, dp, ost, n, l: gpu.mlvfs_amd_render1_amaze_look_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(l), None)
    r1d = lambda sp, st, w, h, pp, dp, ost, n, l: gpu.mlvfs_amd_render1_amaze_deep_dev(vp(sp), st, w, h, vp(pp), vp(dp), ost, n, vp(l), None)
    bad_geom = ((34, H), (W, 35), (46, H), (16, 8), (4, 4), (0, 0), (-48, H), (1 << 13, 1 << 12))
    bad = [bal(0, IMG, W, H, p, d, NP, 1), bal(s, IMG, W, H, 0, d, NP, 1), bal(s, IMG, W, H, p, 0, NP, 1), bal(s, IMG, W, H, p, d, NP, -1),
           bal(s, IMG - 2, W, H, p, d, NP, 2), bal(s, IMG, W, H, p, d, NP - 1, 2), bal(s, IMG + 1, W, H, p, d, NP, 2), bal(s + 1, IMG, W, H, p, d, NP, 1),
           bal(s, IMG, W, H, p + 2, d, NP, 1), bal(s, IMG, W, H, p, d + 2, NP, 1), bal(d + 1024, IMG, W, H, p, d + 1024, NP, 1),
           bal(d + 1024, IMG, W, H, p, d + 1024 + IMG - 4, NP, 1), bal(s, IMG, W, H, d + 64, d, NP, 1)]
    bad += [bal(s, IMG, w, h, p, d, NP, 1) for w, h in bad_geom]
    bad += [tone(0, qg, qb, NP, W, H, p, d, OUT, 1), tone(qr, 0, qb, NP, W, H, p, d, OUT, 1), tone(qr, qg, 0, NP, W, H, p, d, OUT, 1),
            tone(qr, qg, qb, NP, W, H, 0, d, OUT, 1), tone(qr, qg, qb, NP, W, H, p, 0, OUT, 1), tone(qr, qg, qb, NP, W, H, p, d, OUT, 1, L, L16),
            tone(qr, qg, qb, NP, W, H, p, d, OUT, -1), tone(qr, qg, qb, NP - 1, W, H, p, d, OUT, 2), tone(qr, qg, qb, NP, W, H, p, d, OUT - 1, 2),
            tone(qr, qg, qb, NP, W, H, p, d, 2 * OUT - 1, 2, 0, L16), tone(qr + 2, qg, qb, NP, W, H, p, d, OUT, 1), tone(qr, qg, qb, NP, W, H, p + 2, d, OUT, 1),
            tone(d + 8192, qg, qb, NP, W, H, p, d + 8192 + 4 * NP - 1, OUT, 1), tone(qr, qg, d + 8192, NP, W, H, p, d + 8192 - OUT + 1, OUT, 1),
            tone(qr, qg, qb, NP, W, H, d + 64, d, OUT, 1)]
    bad += [tone(qr, qg, qb, NP, w, h, p, d, OUT, 1) for w, h in bad_geom]
    bad += [r1(0, IMG, W, H, p, d, OUT, 1), r1(s, IMG, W, H, 0, d, OUT, 1), r1(s, IMG, W, H, p, 0, OUT, 1), r1(s, IMG, W, H, p, d, OUT, -1),
            r1(s, IMG - 2, W, H, p, d, OUT, 2), r1(s, IMG, W, H, p, d, OUT - 1, 2), r1(s, IMG + 1, W, H, p, d, OUT, 2), r1(s + 1, IMG, W, H, p, d, OUT, 1),
            r1(s, IMG, W, H, p + 2, d, OUT, 1), r1(d + 8192, IMG, W, H, p, d + 8192, OUT, 1), r1(d + 8192, IMG, W, H, p, d + 8192 + IMG - 1, OUT, 1),
            r1(d + 8192, IMG, W, H, p, d + 8192 - OUT + 1, OUT, 1), r1(s, IMG, W, H, d + 64, d, OUT, 1),
            r1l(s, IMG, W, H, p, d, OUT, 1, 0), r1d(s, IMG, W, H, p, d, 2 * OUT, 1, 0), r1d(s, IMG, W, H, p, d, 2 * OUT - 1, 2, L16),
            r1l(s, IMG, 34, H, p, d, OUT, 1, L), r1d(s, IMG, W, 35, p, d, 2 * OUT, 1, L16)]
    bad += [r1(s, IMG, w, h, p, d, OUT, 1) for w, h in bad_geom]
    assert all(rc == lib.ERR_ARG for rc in bad), [k for k, rc in enumerate(bad) if rc != lib.ERR_ARG]
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all()) and bool((pl == 0).all())
    # directly behind the source: no overlap
    lib.check(r1(d + 8192, IMG, W, H, p, d + 8192 + IMG, OUT, 1), "render1_amaze_dev")
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    at = 8192 + IMG
    assert (host[:at] == PAD).all() and (host[at + OUT:] == PAD).all() and not (host[at:at + OUT] == PAD).all()
    pw, ph = C.c_int(-7), C.c_int(-7)
    assert gpu.mlvfs_amd_rgb_amaze_geom(40, 38, C.byref(pw), C.byref(ph)) == 0 and (pw.value, ph.value) == (40, 38)
    assert gpu.mlvfs_amd_rgb_amaze_geom(38, 38, C.byref(pw), C.byref(ph)) == lib.ERR_ARG and (pw.value, ph.value) == (40, 38)
