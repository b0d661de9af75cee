"""Resampled rendered frames demosaiced by AMaZE on the GPU (csrc/k_amaze_resample.hip, csrc/amaze_render.cpp), against
the definition of mlvfs_amd/amaze_resample.py with the checker's AMaZE, for equality: mlvfs_amd_amaze_resample_dev on crafted planes and
on the checker's planes in the three tone forms, both matrix paths and both kernel forms wherever both apply (planes one float off a
16-byte boundary, or an odd deep destination, take the generic form); the three mlvfs_amd_render_resampled_amaze calls end to end at
every source and size of tests/amaze_resample_cases.py -- batches of 1 and 3 with parameters of their own, padded strides, aligned and
misaligned bases, the bytes around the renderings and the source unchanged --, the identity size against mlvfs_amd_render1_amaze_dev,
the identity look against the plain call; geometries in turn on one thread; a failed growth of the work memory; one 3584 x 1320 frame
to 1920 x 707; every refusal."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import amaze_render, lib, look, render, resample

import amaze_resample_cases as arc
import deep_cases as dc
import demosaic_cases as dm
import look_cases as lc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
FORMS = ("plain", "look", "deep")
LOOK, LOOK16 = lc.look_of("random17"), dc.look_of("random3")
BPX = {"plain": 3, "look": 3, "deep": 6}
# (frames, source offset, destination offset, aligned strides)
PLACEMENTS = [(1, 0, 0, True), (3, 0, 0, True), (3, 2, 1, False)]
# (plane offset in bytes, destination offset, aligned strides): the fast form where the sizes allow it; planes one float off, the generic
# form; an odd destination, the generic form for the deep look alone
PLANE_PLACEMENTS = [(0, 0, True), (16, 16, True), (4, 1, False), (0, 1, True)]


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
    """step 4 of one form on the definition's indices -> (oh, ow, 3)"""
    if form == "deep":
        return np.ascontiguousarray(look.apply16(t16, *LOOK16).transpose(1, 2, 0)).astype(np.uint16)
    return render.tone(t, look=LOOK if form == "look" else None)


def as_pixels(form, part, w, h):
    return np.frombuffer(part.tobytes(), "<u2").reshape(h, w, 3) if form == "deep" else part.reshape(h, w, 3)


def where(got, want):
    bad = np.argwhere((got != want).any(axis=2))
    return len(bad), bad[:4].tolist()


def want_of(form, f, p, n, ow, oh):
    st = resample.stages(f, p, ow, oh, source=n)
    return develop(form, st["t"], st["t16"])


def run_route(gpu, handles, form, frames, params, ow, oh, src_off, dst_off, aligned, full=False):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (renderings, every other byte of the destination);
    full: through mlvfs_amd_render1_amaze_dev and its forms instead (ow x oh is the frame's size then)"""
    import torch
    h, w = frames[0].shape
    n, img, pimg = len(frames), w * h * 2, ow * oh * BPX[form]
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 5)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(arc.params_array(params)).cuda()
    s, d, p = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off), C.c_void_p(par.data_ptr())
    size = () if full else (ow, oh)
    name = "mlvfs_amd_render1_amaze" if full else "mlvfs_amd_render_resampled_amaze"
    if form == "plain":
        rc = getattr(gpu, name + "_dev")(s, stride, w, h, p, *size, d, ostride, n, None)
    elif form == "look":
        rc = getattr(gpu, name + "_look_dev")(s, stride, w, h, p, *size, d, ostride, n, C.c_void_p(handles["look"].h), None)
    else:
        rc = getattr(gpu, name + "_deep_dev")(s, stride, w, h, p, *size, d, ostride, n, C.c_void_p(handles["deep"].h), None)
    lib.check(rc, name + "_" + form)
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [as_pixels(form, q, ow, oh) for q in parts], rest


@pytest.fixture(scope="module")
def staged(oracle):
    """the batch of every source, with the definition's n of each frame, computed once: {(w, h): [(frame, parameters, n)]}"""
    out = {}
    for w, h in arc.SOURCES:
        out[(w, h)] = [(f, p, amaze_render.stages(f, p, oracle.amaze_demosaic)["n"]) for f, p in arc.batch(w, h, 3, first=(w + h) % 4)]
    return out


def end_to_end(gpu, handles, batch, sizes, forms=FORMS, placements=PLACEMENTS):
    h, w = batch[0][0].shape
    for ow, oh in sizes:
        for form in forms:
            want = [want_of(form, f, p, n, ow, oh) for f, p, n in batch]
            for k, src_off, dst_off, aligned in placements:
                got, rest = run_route(gpu, handles, form, [b[0] for b in batch[:k]], [b[1] for b in batch[:k]], ow, oh, src_off, dst_off, aligned)
                assert (rest == PAD).all(), (w, h, ow, oh, form, k, src_off, dst_off, "bytes outside the renderings changed")
                for i in range(k):
                    assert np.array_equal(got[i], want[i]), (w, h, ow, oh, form, k, src_off, dst_off, i, where(got[i], want[i]))


@pytest.mark.parametrize("w,h", arc.SOURCES, ids=lambda v: str(v))
def test_render_resampled_amaze_equals_the_definition(gpu, handles, staged, w, h):
    end_to_end(gpu, handles, staged[(w, h)], arc.out_sizes(w, h))


@pytest.mark.parametrize("w,h", [(40, 38), (164, 148), (48, 70)], ids=lambda v: str(v))
def test_the_identity_size_is_render1_amaze(gpu, handles, staged, w, h):
    batch = staged[(w, h)]
    frames, params = [b[0] for b in batch], [b[1] for b in batch]
    for form in FORMS:
        a, _ = run_route(gpu, handles, form, frames, params, w, h, 0, 0, True)
        b, _ = run_route(gpu, handles, form, frames, params, w, h, 0, 0, True, full=True)
        for k in range(3):
            assert np.array_equal(a[k], b[k]), (w, h, form, k, where(a[k], b[k]))


def test_the_identity_look_is_the_plain_call(gpu, handles, staged):
    w, h = 48, 70
    batch = staged[(w, h)]
    frames, params = [b[0] for b in batch], [b[1] for b in batch]
    ident = look.Look(*lc.look_of("identity17"))
    try:
        for ow, oh in arc.out_sizes(w, h)[:4]:
            plain, _ = run_route(gpu, handles, "plain", frames, params, ow, oh, 0, 0, True)
            got, _ = run_route(gpu, {"look": ident}, "look", frames, params, ow, oh, 0, 0, True)
            for k in range(3):
                assert np.array_equal(got[k], plain[k]), (ow, oh, k)
    finally:
        ident.close()


def run_pass(gpu, handles, form, planes, params, ow, oh, pl_off, dst_off, aligned):
    """planes: per frame (3, H, W) float32 -> (renderings, every other byte of the destination); the planes lie as three batches"""
    import torch
    n, (_, h, w) = len(planes), planes[0].shape
    npix, pimg = w * h, ow * oh * BPX[form]
    pstride, ostride = ((npix + 3) // 4 * 4 + 8, up16(pimg) + 16) if aligned else (npix + 1, pimg + 5)
    bufs = [device_buffer(torch, [np.ascontiguousarray(pl[c]) for pl in planes], 4 * pstride, pl_off) for c in range(3)]
    before = [b.clone() for b in bufs]
    dst = device_buffer(torch, [np.full(pimg, PAD, np.uint8)] * n, ostride, dst_off)
    par = torch.from_numpy(arc.params_array(params)).cuda()
    lk = None if form != "look" else C.c_void_p(handles["look"].h)
    lk16 = None if form != "deep" else C.c_void_p(handles["deep"].h)
    lib.check(gpu.mlvfs_amd_amaze_resample_dev(*[C.c_void_p(b.data_ptr() + pl_off) for b in bufs], pstride, w, h, C.c_void_p(par.data_ptr()),
                                               ow, oh, C.c_void_p(dst.data_ptr() + dst_off), ostride, n, lk, lk16, None), "amaze_resample_dev")
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.uint8), b0.view(torch.uint8)), "a plane changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [as_pixels(form, q, ow, oh) for q in parts], rest


@pytest.mark.parametrize("form", FORMS)
def test_amaze_resample_dev_on_crafted_planes(gpu, handles, form):
    """NaN, the infinities, -0.0, k + 0.5, the neighbourhood of both clamps and 0.49999997 in every channel, through both matrix paths
    and both kernel forms"""
    sets = [dm.param_set(0)[1], dm.param_set(1)[1], arc.wide_set()[1]]
    assert [arc.matrix_fits_32(p) for p in sets] == [True, False, False]
    for w, h in ((48, 37), (36, 36), (528, 36)):
        planes, n = arc.crafted_planes(w, h)
        frame = np.zeros((h, w), np.uint16)
        for ow, oh in arc.out_sizes(w, h):
            want = [want_of(form, frame, p, n, ow, oh) for p in sets]
            for pl_off, dst_off, aligned in PLANE_PLACEMENTS:
                got, rest = run_pass(gpu, handles, form, [planes] * 3, sets, ow, oh, pl_off, dst_off, aligned)
                assert (rest == PAD).all(), (w, h, ow, oh, pl_off, dst_off)
                for k in range(3):
                    assert np.array_equal(got[k], want[k]), (w, h, ow, oh, form, pl_off, dst_off, k, where(got[k], want[k]))


@pytest.mark.parametrize("form", FORMS)
def test_amaze_resample_dev_on_the_checkers_planes(gpu, oracle, handles, form):
    for w, h in ((48, 70), (164, 148)):
        batch = arc.batch(w, h, 3)
        staged = [amaze_render.stages(f, p, oracle.amaze_demosaic) for f, p in batch]
        assert [arc.matrix_fits_32(p) for _, p in batch] == [True, False, True]
        for ow, oh in arc.out_sizes(w, h)[:5]:
            want = [want_of(form, f, p, st["n"], ow, oh) for (f, p), st in zip(batch, staged)]
            for pl_off, dst_off, aligned in PLANE_PLACEMENTS[:3]:
                got, rest = run_pass(gpu, handles, form, [st["planes"] for st in staged], [p for _, p in batch], ow, oh, pl_off, dst_off, aligned)
                assert (rest == PAD).all()
                for k in range(3):
                    assert np.array_equal(got[k], want[k]), (w, h, ow, oh, form, pl_off, dst_off, k, where(got[k], want[k]))


def test_the_route_differs_from_the_linear_resampled_route(gpu, handles, staged):
    import torch
    w, h = 164, 148
    f, p, n = staged[(w, h)][0]
    ow, oh = 110, 99
    got, _ = run_route(gpu, handles, "plain", [f], [p], ow, oh, 0, 0, True)
    src = torch.from_numpy(f.view(np.int16)).cuda()
    dst = torch.zeros((ow * oh * 3,), dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(arc.params_array([p])).cuda()
    lib.check(gpu.mlvfs_amd_render_resampled_dev(C.c_void_p(src.data_ptr()), w * h * 2, w, h, C.c_void_p(par.data_ptr()), ow, oh,
                                                 C.c_void_p(dst.data_ptr()), ow * oh * 3, 1, None), "render_resampled_dev")
    torch.cuda.synchronize()
    lin = dst.cpu().numpy().reshape(oh, ow, 3)
    assert np.array_equal(lin, resample.render(f, p, ow, oh)) and not np.array_equal(lin, got[0])


def test_geometries_in_turn_on_one_thread(gpu, oracle, handles, staged):
    """the tile planes are zeroed when the geometry changes: another size in between -- through this route, through the full-size AMaZE
    rendering, and through the dual-ISO route's AMaZE call, which has tile planes of its own -- leaves nothing behind"""
    import torch
    one = [(1, 0, 0, True)]
    a, b = (164, 148), (292, 36)
    end_to_end(gpu, handles, staged[a], [(110, 99)], forms=("plain",), placements=one)
    end_to_end(gpu, handles, staged[b], [(195, 25)], forms=("plain",), placements=one)
    end_to_end(gpu, handles, staged[a], [(110, 99)], forms=("plain",), placements=one)
    fa, pa, na = staged[a][0]
    full, _ = run_route(gpu, handles, "plain", [fa], [pa], *a, 0, 0, True, full=True)
    assert np.array_equal(full[0], want_of("plain", fa, pa, na, *a))
    w, h = 148, 40
    raw = torch.from_numpy(dm.speckle_frame(w, h, 2048, 15000).astype(np.float32)).cuda()
    out = [torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(3)]
    lib.check(gpu.mlvfs_amd_amaze_demosaic_dev(C.c_void_p(raw.data_ptr()), w, h, *[C.c_void_p(o.data_ptr()) for o in out], None), "amaze_demosaic_dev")
    torch.cuda.synchronize()
    want = oracle.amaze_demosaic(raw.cpu().numpy())
    end_to_end(gpu, handles, staged[a], [(83, 148)], forms=("deep",), placements=[(3, 0, 0, True)])
    lib.check(gpu.mlvfs_amd_amaze_demosaic_dev(C.c_void_p(raw.data_ptr()), w, h, *[C.c_void_p(o.data_ptr()) for o in out], None), "amaze_demosaic_dev")
    torch.cuda.synchronize()
    for g, x in zip(out, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), x.view(np.uint32))


def test_a_failed_growth_of_the_work_memory_halves_the_sub_batch(gpu, handles, staged):
    """mlvfs_amd_test_fail_next(3) fails the next growth of a device buffer: with the thread's work memory given back that is the
    planes of a batch of 3, which then goes as 2 + 1 and renders what it always renders; a single frame whose work memory cannot be
    had is an error, and the call after it serves again"""
    import torch
    w, h = 148, 40
    ow, oh = 99, 27
    gpu.mlvfs_amd_dualiso_trim()
    gpu.mlvfs_amd_test_fail_next(3)
    end_to_end(gpu, handles, staged[(w, h)], [(ow, oh)], forms=("plain",), placements=[(3, 0, 0, True)])
    gpu.mlvfs_amd_dualiso_trim()
    f, p, _ = staged[(w, h)][0]
    src = torch.from_numpy(f.view(np.int16)).cuda()
    dst = torch.full((ow * oh * 3,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(arc.params_array([p])).cuda()
    gpu.mlvfs_amd_test_fail_next(3)
    assert gpu.mlvfs_amd_render_resampled_amaze_dev(C.c_void_p(src.data_ptr()), w * h * 2, w, h, C.c_void_p(par.data_ptr()), ow, oh,
                                                    C.c_void_p(dst.data_ptr()), ow * oh * 3, 1, None) == lib.ERR_HIP and b"injected" in gpu.mlvfs_amd_last_error()
    torch.cuda.synchronize()
    assert bool((dst == PAD).all())
    end_to_end(gpu, handles, staged[(w, h)], [(ow, oh)], forms=("look",), placements=[(3, 0, 0, True)])


def test_a_full_size_frame_to_1920x707(gpu, oracle, handles):
    (b0, w0), p0 = dm.param_set(2)
    f = dm.speckle_frame(arc.BIG_W, arc.BIG_H, b0, w0)
    n = amaze_render.stages(f, p0, oracle.amaze_demosaic)["n"]
    ow, oh = arc.BIG_SIZE
    got, rest = run_route(gpu, handles, "plain", [f], [p0], ow, oh, 0, 0, True)
    want = want_of("plain", f, p0, n, ow, oh)
    assert (rest == PAD).all() and np.array_equal(got[0], want), where(got[0], want)


def test_refusals_leave_the_destination(gpu, handles):
    import torch
    W, H, IMG, NP, OW, OH = 48, 36, 3456, 1728, 30, 20
    OUT = 3 * OW * OH
    src = torch.full((3 * IMG + 64,), 7, dtype=torch.uint8, device="cuda")
    pl = torch.zeros((9 * NP + 16,), dtype=torch.float32, device="cuda")
    dst = torch.full((6 * 3 * W * H + 64,), PAD, dtype=torch.uint8, device="cuda")
    par = torch.from_numpy(arc.params_array([dm.param_set(k)[1] for k in range(3)])).cuda()
    s, q, d, p = src.data_ptr(), pl.data_ptr(), dst.data_ptr(), par.data_ptr()
    qr, qg, qb = q, q + 12 * NP, q + 24 * NP
    L, L16 = handles["look"].h, handles["deep"].h
    vp = lambda a: C.c_void_p(a) if a else None
    rs = lambda r, g, b, ps, w, h, pp, ow, oh, dp, ost, n, l=0, l16=0: gpu.mlvfs_amd_amaze_resample_dev(vp(r), vp(g), vp(b), ps, w, h, vp(pp), ow, oh, vp(dp), ost, n, vp(l), vp(l16), None)
    ra = lambda sp, st, w, h, pp, ow, oh, dp, ost, n: gpu.mlvfs_amd_render_resampled_amaze_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, None)
    ral = lambda sp, st, w, h, pp, ow, oh, dp, ost, n, l: gpu.mlvfs_amd_render_resampled_amaze_look_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, vp(l), None)
    rad = lambda sp, st, w, h, pp, ow, oh, dp, ost, n, l: gpu.mlvfs_amd_render_resampled_amaze_deep_dev(vp(sp), st, w, h, vp(pp), ow, oh, vp(dp), ost, n, vp(l), None)
    bad_geom = ((34, H), (W, 35), (46, H), (16, 8), (4, 4), (0, 0), (-48, H), (1 << 13, 1 << 12), (36, 65536))
    bad_size = ((0, OH), (OW, 0), (W + 1, OH), (OW, H + 1), (-1, -1), (1 << 20, 1))
    bad = [rs(0, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1), rs(qr, 0, qb, NP, W, H, p, OW, OH, d, OUT, 1), rs(qr, qg, 0, NP, W, H, p, OW, OH, d, OUT, 1),
           rs(qr, qg, qb, NP, W, H, 0, OW, OH, d, OUT, 1), rs(qr, qg, qb, NP, W, H, p, OW, OH, 0, OUT, 1), rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1, L, L16),
           rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT, -1), rs(qr, qg, qb, NP - 1, W, H, p, OW, OH, d, OUT, 2), rs(qr, qg, qb, NP, W, H, p, OW, OH, d, OUT - 1, 2),
           rs(qr, qg, qb, NP, W, H, p, OW, OH, d, 2 * OUT - 1, 2, 0, L16), rs(qr + 2, qg, qb, NP, W, H, p, OW, OH, d, OUT, 1),
           rs(qr, qg, qb, NP, W, H, p + 2, OW, OH, d, OUT, 1), rs(d + 8192, qg, qb, NP, W, H, p, OW, OH, d + 8192 + 4 * NP - 1, OUT, 1),
           rs(qr, qg, d + 8192, NP, W, H, p, OW, OH, d + 8192 - OUT + 1, OUT, 1), rs(qr, qg, qb, NP, W, H, d + 64, OW, OH, d, OUT, 1)]
    bad += [rs(qr, qg, qb, NP, w, h, p, 1, 1, d, OUT, 1) for w, h in bad_geom]
    bad += [rs(qr, qg, qb, NP, W, H, p, ow, oh, d, OUT, 1) for ow, oh in bad_size]
    bad += [ra(0, IMG, W, H, p, OW, OH, d, OUT, 1), ra(s, IMG, W, H, 0, OW, OH, d, OUT, 1), ra(s, IMG, W, H, p, OW, OH, 0, OUT, 1),
            ra(s, IMG, W, H, p, OW, OH, d, OUT, -1), ra(s, IMG - 2, W, H, p, OW, OH, d, OUT, 2), ra(s, IMG, W, H, p, OW, OH, d, OUT - 1, 2),
            ra(s, IMG + 1, W, H, p, OW, OH, d, OUT, 2), ra(s + 1, IMG, W, H, p, OW, OH, d, OUT, 1), ra(s, IMG, W, H, p + 2, OW, OH, d, OUT, 1),
            ra(d + 8192, IMG, W, H, p, OW, OH, d + 8192, OUT, 1), ra(d + 8192, IMG, W, H, p, OW, OH, d + 8192 + IMG - 1, OUT, 1),
            ra(d + 8192, IMG, W, H, p, OW, OH, d + 8192 - OUT + 1, OUT, 1), ra(s, IMG, W, H, d + 64, OW, OH, d, OUT, 1),
            ral(s, IMG, W, H, p, OW, OH, d, OUT, 1, 0), rad(s, IMG, W, H, p, OW, OH, d, 2 * OUT, 1, 0), rad(s, IMG, W, H, p, OW, OH, d, 2 * OUT - 1, 2, L16),
            ral(s, IMG, 34, H, p, OW, OH, d, OUT, 1, L), rad(s, IMG, W, 35, p, OW, OH, d, 2 * OUT, 1, L16), ral(s, IMG, W, H, p, W + 1, OH, d, OUT, 1, L)]
    bad += [ra(s, IMG, w, h, p, 1, 1, d, OUT, 1) for w, h in bad_geom]
    bad += [ra(s, IMG, W, H, p, ow, oh, d, OUT, 1) for ow, oh in bad_size]
    assert all(rc == lib.ERR_ARG for rc in bad), [k for k, rc in enumerate(bad) if rc != lib.ERR_ARG]
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all()) and bool((pl == 0).all())
    # directly behind the source: no overlap
    lib.check(ra(d + 8192, IMG, W, H, p, OW, OH, d + 8192 + IMG, OUT, 1), "render_resampled_amaze_dev")
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    at = 8192 + IMG
    assert (host[:at] == PAD).all() and (host[at + OUT:] == PAD).all() and not (host[at:at + OUT] == PAD).all()
    assert gpu.mlvfs_amd_rgb_amaze_resample_geom(40, 38, 40, 38) == 0 and gpu.mlvfs_amd_rgb_amaze_resample_geom(40, 38, 41, 38) == lib.ERR_ARG
