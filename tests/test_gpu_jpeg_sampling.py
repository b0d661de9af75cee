"""The chroma samplings of the rendered JPEG files on the GPU (csrc/k_jpeg.hip, csrc/jpeg.cpp):
mlvfs_amd_jpeg_encode_sampled_dev against the numpy definition of mlvfs_amd/jpeg.py at 4:2:2 and 4:4:4 on every case of
tests/jpeg_sampling_cases.py, at 4:2:0 against mlvfs_amd_jpeg_encode_dev, its room and its refusals.  All comparisons are for equality."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib

import jpeg_cases as jc
import jpeg_sampling_cases as sc
from test_gpu_mlv_transcode import PAD, device_buffer

pytestmark = pytest.mark.gpu


def encode_dev(gpu, images, quality, sampling, src_off=0, dst_off=0, room=None, gap=(7, 5), old_call=False):
    """the renderings at padded strides from byte src_off of a PAD-filled device buffer -> (destination buffer, stride, lengths, status);
    old_call: through mlvfs_amd_jpeg_encode_dev, which has no sampling"""
    import torch
    ph, pw = images[0].shape[:2]
    n, img = len(images), pw * ph * 3
    stride, ostride = img + gap[0], room + gap[1]
    src = device_buffer(torch, images, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(room, PAD, np.uint8)] * n, ostride, dst_off)
    need = gpu.mlvfs_amd_jpeg_scratch_bytes(pw, ph, n) if old_call else gpu.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, sc.CODE[sampling], n)
    assert need > 0
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    lengths, status = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, -1, np.int32)
    s, d = C.c_void_p(src.data_ptr() + src_off), C.c_void_p(dst.data_ptr() + dst_off)
    if old_call:
        rc = gpu.mlvfs_amd_jpeg_encode_dev(s, stride, pw, ph, quality, d, ostride, room, C.c_void_p(scratch.data_ptr()), need, lib.ptr(lengths),
                                           lib.ptr(status), n, None)
    else:
        rc = gpu.mlvfs_amd_jpeg_encode_sampled_dev(s, stride, pw, ph, quality, sc.CODE[sampling], d, ostride, room, C.c_void_p(scratch.data_ptr()),
                                                   need, lib.ptr(lengths), lib.ptr(status), n, None)
    lib.check(rc, "jpeg_encode_sampled_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    return dst, ostride, lengths, status


def check_batch(gpu, sampling, pw, ph, contents, quality, src_off, dst_off):
    """contents: [(content index, seed)]; every stream is the definition's, every other byte of the destination is untouched"""
    images = [sc.CONTENT[sampling][c](pw, ph, s) for c, s in contents]
    want = [sc.expected(sampling, pw, ph, c, quality, s) for c, s in contents]
    room = max(len(w) for w in want) + 3
    dst, ostride, lengths, status = encode_dev(gpu, images, quality, sampling, src_off, dst_off, room)
    host = dst.cpu().numpy()
    label = (sampling, pw, ph, contents, quality, src_off, dst_off)
    assert list(status) == [0] * len(want) and list(lengths) == [len(w) for w in want], label
    rest = np.ones(host.size, bool)
    for k, w in enumerate(want):
        a = dst_off + k * ostride
        assert host[a:a + len(w)].tobytes() == w, (label, k)
        rest[a:a + len(w)] = False
    assert (host[rest] == PAD).all(), label


SHAPES = [(s, pw, ph) for s in sc.SAMPLINGS for pw, ph in sc.shapes(s)]


@pytest.mark.parametrize("sampling,pw,ph", SHAPES, ids=lambda v: str(v))
def test_encode_sampled_dev_equals_numpy(gpu, sampling, pw, ph):
    """every content at every quality, in batches of 5 frames of distinct content, at padded strides and every alignment of the source and
    the destination"""
    assert len(sc.CONTENT[sampling]) == 9
    for qi, q in enumerate(sc.QUALITIES):
        check_batch(gpu, sampling, pw, ph, sc.batch(sampling, 5, 0), q, qi % 4, (qi + 1) % 4)
        check_batch(gpu, sampling, pw, ph, sc.batch(sampling, 5, 5), q, (qi + 2) % 4, (qi + 3) % 4)


LONG = [(s, pw, ph) for s in sc.SAMPLINGS for pw, ph in sc.LONG[s]]


@pytest.mark.parametrize("sampling,pw,ph", LONG, ids=lambda v: str(v))
def test_encode_sampled_dev_long_rows_and_many_rows(gpu, sampling, pw, ph):
    check_batch(gpu, sampling, pw, ph, [(1, 0), (3, 1)], 75, 1, 2)


def test_sampling_0_is_the_old_call(gpu):
    """MLVFS_AMD_JPEG_420 through the new call: the bytes, lengths and status of mlvfs_amd_jpeg_encode_dev, which are the definition's"""
    assert sc.CODE == {420: 0, 422: 1, 444: 2}
    for (pw, ph), q in zip([(17, 17), (40, 24), jc.WIDE, (208, 132)], (1, 75, 90, 100)):
        contents = jc.batch(pw, ph, 5, first=q)
        images = [jc.CONTENT[c](pw, ph, s) for c, s in contents]
        want = [jc.expected(pw, ph, c, q, s) for c, s in contents]
        room = max(len(w) for w in want) + 3
        new = encode_dev(gpu, images, q, 420, 1, 2, room)
        old = encode_dev(gpu, images, q, 420, 1, 2, room, old_call=True)
        assert new[1] == old[1] and list(new[2]) == list(old[2]) == [len(w) for w in want] and list(new[3]) == list(old[3]) == [0] * 5
        assert np.array_equal(new[0].cpu().numpy(), old[0].cpu().numpy())
        host = new[0].cpu().numpy()
        for k, w in enumerate(want):
            assert host[2 + k * new[1]:2 + k * new[1] + len(w)].tobytes() == w


@pytest.mark.parametrize("sampling", sc.SAMPLINGS)
def test_encode_sampled_dev_room(gpu, sampling):
    """room exactly the length passes; one byte short sets the status and touches nothing at or behind room"""
    pw, ph, q = 40, 24, 90
    images = [jc.formula(pw, ph), jc.noise(pw, ph)]
    want = [sc.expected(sampling, pw, ph, 1, q), sc.expected(sampling, pw, ph, 3, q)]
    assert len(want[0]) < len(want[1])
    for k in range(2):
        room = len(want[k])
        dst, ostride, lengths, status = encode_dev(gpu, images[k:k + 1], q, sampling, 0, 1, room)
        host = dst.cpu().numpy()
        assert status[0] == 0 and lengths[0] == room and host[1:1 + room].tobytes() == want[k]
        assert host[0] == PAD and (host[1 + room:] == PAD).all()
        dst, ostride, lengths, status = encode_dev(gpu, images[k:k + 1], q, sampling, 0, 1, room - 1)
        host = dst.cpu().numpy()
        assert status[0] == 1 and lengths[0] == room, "the length is known even where it does not fit"
        assert host[0] == PAD and (host[1 + room - 1:] == PAD).all()
    # in a batch: the frame that fits is served, the other one is flagged, and neither reaches its neighbour
    room = len(want[0])
    dst, ostride, lengths, status = encode_dev(gpu, images, q, sampling, 2, 3, room)
    host = dst.cpu().numpy()
    assert list(status) == [0, 1] and list(lengths) == [len(w) for w in want]
    assert host[3:3 + room].tobytes() == want[0] and (host[:3] == PAD).all() and (host[3 + room:3 + ostride] == PAD).all()
    assert (host[3 + ostride + room:] == PAD).all()


def test_encode_sampled_dev_refusals_leave_everything(gpu):
    import torch
    pw, ph = 16, 16
    img = pw * ph * 3
    need = max(gpu.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, k, 2) for k in range(3))
    assert gpu.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, 2, 2) == need
    buf = torch.full((8192 + need + 4096,), PAD, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 255) // 256 * 256
    s, d, scr = base, base + 2048, base + 8192
    lengths, status = np.full(2, 7, np.uint32), np.full(2, 7, np.int32)
    vp = lambda v: C.c_void_p(v) if v else None
    call = lambda sp, st, w, h, q, smp, dp, ost, room, scp, scb, lp, stp, n: gpu.mlvfs_amd_jpeg_encode_sampled_dev(
        vp(sp), st, w, h, q, smp, vp(dp), ost, room, vp(scp), scb, lp, stp, n, None)
    L, S = lib.ptr(lengths), lib.ptr(status)
    for smp in (1, 2):
        exact = gpu.mlvfs_amd_jpeg_scratch_bytes_sampled(pw, ph, smp, 2)
        bad = [
            (0, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, pw, ph, 90, smp, 0, 1024, 1024, scr, need, L, S, 2),
            (s, 1024, pw, ph, 90, smp, d, 1024, 1024, 0, need, L, S, 2), (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, None, S, 2),
            (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, None, 2),
            (s, 1024, 0, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, pw, 0, 90, smp, d, 1024, 1024, scr, need, L, S, 2),
            (s, 1024, 65536, 1, 90, smp, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, 8192, 4096, 90, smp, d, 1024, 1024, scr, need, L, S, 2),
            (s, 1024, pw, ph, 0, smp, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, pw, ph, 101, smp, d, 1024, 1024, scr, need, L, S, 2),
            (s, 1024, pw, ph, 90, -1, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, pw, ph, 90, 3, d, 1024, 1024, scr, need, L, S, 2),
            (s, 1024, pw, ph, 90, 444, d, 1024, 1024, scr, need, L, S, 2),
            (s, img - 1, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 2), (s, 1024, pw, ph, 90, smp, d, 1023, 1024, scr, need, L, S, 2),
            (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, exact - 1, L, S, 2), (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr + 4, need, L, S, 2),
            (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, -1), (s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 65536),
            (s, 1024, pw, ph, 90, smp, s + 1024, 1024, 1024, scr, need, L, S, 2),  # the streams over the second rendering
            (s, 1024, pw, ph, 90, smp, d, 1024, 1024, d + 1024, need, L, S, 2),    # the scratch over the second stream
            (scr + 256, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 2),  # the renderings inside the scratch
        ]
        for args in bad:
            assert call(*args) == lib.ERR_ARG, args
        torch.cuda.synchronize()
        assert bool((buf == PAD).all()) and list(lengths) == [7, 7] and list(status) == [7, 7]
        assert call(s, 1024, pw, ph, 90, smp, d, 1024, 1024, scr, need, L, S, 0) == 0 and list(lengths) == [7, 7]
    # 4:4:4 takes more scratch than 4:2:0: what suffices for the old call is refused here
    small = gpu.mlvfs_amd_jpeg_scratch_bytes(pw, ph, 2)
    assert small < need and call(s, 1024, pw, ph, 90, 2, d, 1024, 1024, scr, small, L, S, 2) == lib.ERR_ARG
    assert bool((buf == PAD).all()) and list(lengths) == [7, 7] and list(status) == [7, 7]
