"""Rendered frames as baseline JPEG files on the GPU (csrc/k_jpeg.hip, csrc/jpeg.cpp, csrc/mount.cpp):
mlvfs_amd_jpeg_encode_dev against the numpy definition of mlvfs_amd/jpeg.py on every case of tests/jpeg_cases.py, and
mlvfs_amd_mount_jpeg against mlvfs_amd_mount_rgb on a second handle: each file is the definition's header and stream of the pixels the
TIFF of the same frame holds, results[] are the same, and PIL opens every file.  All comparisons are for equality."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import jpeg, lib, render

import jpeg_cases as jc
from mount_harness import HDR as TIFF, check_jpegs, fresh, load_tool, make_clip, open_mount, run_tool, serve
from test_gpu_mlv_transcode import PAD, device_buffer

pytestmark = pytest.mark.gpu
HDR = jpeg.HEADER_BYTES


# ------------------------------------------------------------------ mlvfs_amd_jpeg_encode_dev
def encode_dev(gpu, images, quality, src_off=0, dst_off=0, room=None, gap=(7, 5)):
    """the renderings at padded strides from byte src_off of a PAD-filled device buffer -> (destination buffer, stride, lengths, status)"""
    import torch
    ph, pw = images[0].shape[:2]
    n, img = len(images), pw * ph * 3
    stride, ostride = img + gap[0], room + gap[1]
    src = device_buffer(torch, images, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(room, PAD, np.uint8)] * n, ostride, dst_off)
    need = gpu.mlvfs_amd_jpeg_scratch_bytes(pw, ph, n)
    assert need > 0
    scratch = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    lengths, status = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, -1, np.int32)
    lib.check(gpu.mlvfs_amd_jpeg_encode_dev(C.c_void_p(src.data_ptr() + src_off), stride, pw, ph, quality, C.c_void_p(dst.data_ptr() + dst_off),
                                            ostride, room, C.c_void_p(scratch.data_ptr()), need, lib.ptr(lengths), lib.ptr(status), n, None),
              "jpeg_encode_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    return dst, ostride, lengths, status


def check_batch(gpu, pw, ph, contents, quality, src_off, dst_off):
    """contents: [(content index, seed)]; every stream is the oracle's, every other byte of the destination is untouched"""
    images = [jc.CONTENT[c](pw, ph, s) for c, s in contents]
    want = [jc.expected(pw, ph, c, quality, s) for c, s in contents]
    room = max(len(w) for w in want) + 3
    dst, ostride, lengths, status = encode_dev(gpu, images, quality, src_off, dst_off, room)
    host = dst.cpu().numpy()
    label = (pw, ph, contents, quality, src_off, dst_off)
    assert list(status) == [0] * len(want) and list(lengths) == [len(w) for w in want], label
    rest = np.ones(host.size, bool)
    for k, w in enumerate(want):
        a = dst_off + k * ostride
        assert host[a:a + len(w)].tobytes() == w, (label, k)
        rest[a:a + len(w)] = False
    assert (host[rest] == PAD).all(), label


@pytest.mark.parametrize("pw,ph", jc.SHAPES + [jc.WIDE], ids=lambda v: str(v))
def test_encode_dev_equals_numpy(gpu, pw, ph):
    """every content at every quality, in batches of 3, 1 and 3 with different content per frame, at padded strides and every alignment
    of the source and the destination"""
    n = len(jc.CONTENT)
    assert n == 7
    for qi, q in enumerate(jc.QUALITIES):
        check_batch(gpu, pw, ph, [(0, 0), (1, 0), (2, 0)], q, qi % 4, (qi + 1) % 4)
        check_batch(gpu, pw, ph, [(3, 0)], q, (qi + 2) % 4, (qi + 3) % 4)
        check_batch(gpu, pw, ph, [(4, 0), (5, 0), (6, 0)], q, (qi + 3) % 4, qi % 4)


@pytest.mark.parametrize("pw,ph", jc.LONG, ids=lambda v: str(v))
def test_encode_dev_long_rows_and_many_rows(gpu, pw, ph):
    check_batch(gpu, pw, ph, [(1, 0), (3, 1)], 75, 1, 2)


def test_encode_dev_full_size(gpu):
    pw, ph = jc.BIG
    check_batch(gpu, pw, ph, [(1, 0)], 90, 0, 0)


def test_encode_dev_room(gpu):
    """room exactly the length passes; one byte short sets the status and touches nothing at or behind room"""
    pw, ph, q = 40, 24, 90
    images = [jc.formula(pw, ph), jc.noise(pw, ph)]
    want = [jc.expected(pw, ph, 1, q), jc.expected(pw, ph, 3, q)]
    assert len(want[0]) < len(want[1])
    for k in range(2):
        room = len(want[k])
        dst, ostride, lengths, status = encode_dev(gpu, images[k:k + 1], q, 0, 1, room)
        host = dst.cpu().numpy()
        assert status[0] == 0 and lengths[0] == room and host[1:1 + room].tobytes() == want[k]
        assert host[0] == PAD and (host[1 + room:] == PAD).all()
        dst, ostride, lengths, status = encode_dev(gpu, images[k:k + 1], q, 0, 1, room - 1)
        host = dst.cpu().numpy()
        assert status[0] == 1 and lengths[0] == room, "the length is known even where it does not fit"
        assert host[0] == PAD and (host[1 + room - 1:] == PAD).all()
    # in a batch: the frame that fits is served, the other one is flagged, and neither reaches its neighbour
    room = len(want[0])
    dst, ostride, lengths, status = encode_dev(gpu, images, q, 2, 3, room)
    host = dst.cpu().numpy()
    assert list(status) == [0, 1] and list(lengths) == [len(w) for w in want]
    assert host[3:3 + room].tobytes() == want[0] and (host[:3] == PAD).all() and (host[3 + room:3 + ostride] == PAD).all()
    assert (host[3 + ostride + room:] == PAD).all()


def test_encode_dev_refusals_leave_everything(gpu):
    import torch
    pw, ph = 16, 16
    img = pw * ph * 3
    need = gpu.mlvfs_amd_jpeg_scratch_bytes(pw, ph, 2)
    buf = torch.full((8192 + need + 4096,), PAD, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 255) // 256 * 256
    s, d, sc = base, base + 2048, base + 8192
    lengths, status = np.full(2, 7, np.uint32), np.full(2, 7, np.int32)
    vp = lambda v: C.c_void_p(v) if v else None
    call = lambda sp, st, w, h, q, dp, ost, room, scp, scb, lp, stp, n: gpu.mlvfs_amd_jpeg_encode_dev(
        vp(sp), st, w, h, q, vp(dp), ost, room, vp(scp), scb, lp, stp, n, None)
    L, S = lib.ptr(lengths), lib.ptr(status)
    bad = [
        (0, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, S, 2), (s, 1024, pw, ph, 90, 0, 1024, 1024, sc, need, L, S, 2),
        (s, 1024, pw, ph, 90, d, 1024, 1024, 0, need, L, S, 2), (s, 1024, pw, ph, 90, d, 1024, 1024, sc, need, None, S, 2),
        (s, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, None, 2),
        (s, 1024, 0, ph, 90, d, 1024, 1024, sc, need, L, S, 2), (s, 1024, pw, 0, 90, d, 1024, 1024, sc, need, L, S, 2),
        (s, 1024, 65536, 1, 90, d, 1024, 1024, sc, need, L, S, 2), (s, 1024, 8192, 4096, 90, d, 1024, 1024, sc, need, L, S, 2),
        (s, 1024, pw, ph, 0, d, 1024, 1024, sc, need, L, S, 2), (s, 1024, pw, ph, 101, d, 1024, 1024, sc, need, L, S, 2),
        (s, img - 1, pw, ph, 90, d, 1024, 1024, sc, need, L, S, 2), (s, 1024, pw, ph, 90, d, 1023, 1024, sc, need, L, S, 2),
        (s, 1024, pw, ph, 90, d, 1024, 1024, sc, need - 1, L, S, 2), (s, 1024, pw, ph, 90, d, 1024, 1024, sc + 4, need, L, S, 2),
        (s, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, S, -1), (s, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, S, 65536),
        (s, 1024, pw, ph, 90, s + 1024, 1024, 1024, sc, need, L, S, 2),        # the streams over the second rendering
        (s, 1024, pw, ph, 90, d, 1024, 1024, d + 1024, need, L, S, 2),         # the scratch over the second stream
        (sc + 256, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, S, 2),        # the renderings inside the scratch
    ]
    for args in bad:
        assert call(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((buf == PAD).all()) and list(lengths) == [7, 7] and list(status) == [7, 7]
    assert call(s, 1024, pw, ph, 90, d, 1024, 1024, sc, need, L, S, 0) == 0 and list(lengths) == [7, 7]


# ------------------------------------------------------------------ the mount
OPTION_SETS = [("none", dict()), ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1))]
ORDER = ((2, 3, 1.0, 90), (0, 2, 2.5, 50))          # first, count, gain, quality: two calls at two qualities


def check_jpeg(tiffs, jpgs, flags, order, w, h, label):
    """every JPEG file is the definition's of the pixels the TIFF holds, at its call's quality, and none is the TIFF"""
    size = render.geom(w, h)
    check_jpegs([render.split_file(t, *size) for t in tiffs], jpgs, flags, size, label, [q for _, count, _, q in order for _ in range(count)])
    assert flags == [0] * len(jpgs) and all(len(j) < len(t) for j, t in zip(jpgs, tiffs)), label


CASES = [(p, w, h, name, opts) for p in ("plain", "lj92") for w, h in ((64, 48), (418, 266)) for name, opts in OPTION_SETS]


@pytest.mark.parametrize("payload,w,h,name,opts", CASES, ids=[f"{p}:{w}x{h}:{name}" for p, w, h, name, _ in CASES])
def test_mount_jpeg_is_the_rendering_encoded(gpu, tmp_path, payload, w, h, name, opts):
    path = make_clip(tmp_path, payload, w, h)
    tiffs, _, res_rgb, _ = serve(gpu, path, opts, "rgb", order=ORDER)
    jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", order=ORDER)
    assert res_jpg == res_rgb
    check_jpeg(tiffs, jpgs, flags, ORDER, w, h, f"{payload}:{w}x{h}:{name}")
    assert len(set(jpgs)) == len(jpgs), "two frames encoded alike"


def test_mount_jpeg_serves_the_tiff_where_that_is_smaller(gpu, tmp_path):
    """a 16 x 8 clip renders to 8 x 4: the TIFF is 352 bytes, a JPEG file more than its 629 bytes of header"""
    path = make_clip(tmp_path, "plain", 16, 8, n=3)
    order = ((0, 3, 1.0, 90),)
    tiffs, _, res_rgb, _ = serve(gpu, path, {}, "rgb", order=order)
    files, flags, res_jpg, _ = serve(gpu, path, {}, "jpeg", order=order)
    assert flags == [1, 1, 1] and files == tiffs and len(files[0]) == TIFF + 8 * 4 * 3 == 352 and res_jpg == res_rgb


def test_mount_jpeg_interleaves_with_rgb_and_dng(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 416, 264, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, 1.0, 75),)
    want_rgb, _, _, _ = serve(gpu, path, opts, "rgb", order=order, batch=4)
    want_jpg, flags, _, _ = serve(gpu, path, opts, "jpeg", order=order, batch=4)
    check_jpeg(want_rgb, want_jpg, flags, order, 416, 264, "one kind")
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        full = m.dng(0, 8, batch=4)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a, _ = m.jpeg(0, 3, quality=75, batch=2)
        b = m.dng(3, 2, batch=2)
        c = m.rgb(5, 1, batch=2)
        d, _ = m.jpeg(6, 2, quality=75, batch=2)
    assert a + d == want_jpg[:3] + want_jpg[6:]
    assert [f.tobytes() for f in b] == [f.tobytes() for f in full[3:5]] and c[0].tobytes() == want_rgb[5]


def test_mount_jpeg_refusals(gpu, tmp_path):
    w, h = 64, 48
    path = make_clip(tmp_path, "plain", w, h, n=4)
    size = TIFF + 32 * 24 * 3
    out = np.full(2 * size + 64, PAD, np.uint8)
    sizes, flags = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        j = lambda o, stride, gain, q, s, f: gpu.mlvfs_amd_mount_jpeg(m.h, 0, 2, o, stride, gain, q, s, f, 2, 0, None)
        O, S, F = lib.ptr(out), lib.ptr(sizes), lib.ptr(flags)
        for args in ((O, size, 256, 0, S, F), (O, size, 256, 101, S, F), (O, size, 0, 90, S, F), (O, size, 65536, 90, S, F),
                     (O, size - 1, 256, 90, S, F), (None, size, 256, 90, S, F), (O, size, 256, 90, None, F), (O, size, 256, 90, S, None)):
            assert j(*args) == lib.ERR_ARG, args
        assert (out == PAD).all() and list(sizes) == [7, 7] and list(flags) == [7, 7]
        with pytest.raises(ValueError):
            m.jpeg(0, 2, quality=0)
        lib.check(j(O, size, 256, 90, S, F), "mount_jpeg")                       # exactly the TIFF's size is room enough
        assert list(flags) == [0, 0] and all(HDR < s < size for s in sizes)
        for k in range(2):
            assert (out[k * size + int(sizes[k]):(k + 1) * size] == PAD).all(), "bytes behind a file were touched"
    fresh(gpu)
    r, m = open_mount(path, {}, proxy=2)
    with r, m:
        out[:] = PAD
        assert gpu.mlvfs_amd_mount_jpeg(m.h, 0, 2, lib.ptr(out), size, 256, 90, lib.ptr(sizes), lib.ptr(flags), 2, 0, None) == lib.ERR_ARG
        assert b"prox" in gpu.mlvfs_amd_last_error() and (out == PAD).all()
        with pytest.raises(lib.MlvfsAmdError):
            m.jpeg(0, 2)
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)            # the refusal served nothing and spoilt nothing


def test_the_render_tool_writes_jpeg_files(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --jpeg (its main(), in this process): the files are mlvfs_amd_mount_jpeg's"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, flags, _, _ = serve(gpu, path, opts, "jpeg", order=((0, 3, 1.5, 80),))
    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    out = tmp_path / "out"
    assert run(out, ["--jpeg", "80"]) == 0
    names = sorted(os.listdir(out))
    assert names == ["M07-1234_%06d.jpg" % k for k in range(3)] and flags == [0, 0, 0]
    assert [open(out / n, "rb").read() for n in names] == want
    with Image.open(out / names[0]) as im:
        assert im.format == "JPEG" and im.size == (32, 24)
    capsys.readouterr()
    assert run(out, ["--jpeg"]) == 1 and "nothing is overwritten" in capsys.readouterr().err
    assert [open(out / n, "rb").read() for n in names] == want
    out2 = tmp_path / "out2"
    assert run(out2, ["--jpeg"]) == 0                                           # quality 90 where none is given
    first = open(out2 / names[0], "rb").read()
    assert first[:HDR] == jpeg.header(32, 24, 90)
