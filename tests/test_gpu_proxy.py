"""Half-size Bayer proxies on the GPU (csrc/k_proxy.hip, csrc/mount.cpp): mlvfs_amd_bin2_dev against the numpy
restatement of tests/proxy_cases.py, and a mount with mlvfs_amd_mount_set_proxy(2) against a full-size mount of the same clip and
options: the proxy's pixels are bin2 of the full-size file's pixels (so every stage in front of the binning ran at full size), its
header is the full-size header with the header rule applied, results[] are the same; lossless streams are the reference encoder's
of the proxy pixels.  All comparisons are for equality."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth

import proxy_cases as pc
from lossless_cases import jpeg_view, max_class
from mount_harness import H, NAME, PAYLOADS, W, calibration, dual_clip, fresh, load_tool, open_mount, payloads, run_tool
from test_gpu_mlv_transcode import PAD, device_buffer, split
from test_gpu_ref_host import make_clip

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ mlvfs_amd_bin2_dev
def up16(v):
    return (v + 15) // 16 * 16


def run_bin2(gpu, frames, src_off, dst_off, aligned):
    """the frames at padded strides from byte src_off of a PAD-filled device buffer -> (proxies, every other byte of the destination)"""
    import torch
    h, w = frames[0].shape
    pw, ph = pc.proxy_size(w, h)
    n, img, pimg = len(frames), w * h * 2, pw * ph * 2
    stride, ostride = (up16(img) + 32, up16(pimg) + 16) if aligned else (img + 6, pimg + 10)
    src = device_buffer(torch, frames, stride, src_off)
    before = src.clone()
    dst = device_buffer(torch, [np.full(pimg // 2, PAD | PAD << 8, np.uint16)] * n, ostride, dst_off)
    lib.check(gpu.mlvfs_amd_bin2_dev(C.c_void_p(src.data_ptr() + src_off), stride, w, h, C.c_void_p(dst.data_ptr() + dst_off), ostride, n, None), "bin2_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ostride, pimg, dst_off)
    return [np.frombuffer(bytes(p), "<u2").reshape(ph, pw) for p in parts], rest


@pytest.mark.parametrize("w,h", pc.BIN_SIZES, ids=lambda v: str(v))
def test_bin2_dev_equals_numpy(gpu, w, h):
    first = 0
    for n in (1, 3):
        for src_off, dst_off, aligned in ((0, 0, True), (2, 0, False), (0, 2, False), (16, 32, True), (2, 2, False)):
            frames = pc.batch(w, h, n, first)
            first += n                                          # every kind of content at every size
            got, rest = run_bin2(gpu, frames, src_off, dst_off, aligned)
            assert (rest == PAD).all(), (n, src_off, dst_off, "bytes outside the proxies changed")
            for k, f in enumerate(frames):
                want = pc.bin2(f)
                assert np.array_equal(got[k], want), (n, src_off, dst_off, k, int((got[k] != want).sum()))


def test_bin2_dev_full_size(gpu):
    frames = [pc.random_frame(pc.BIG_W, pc.BIG_H, 1), pc.position_frame(pc.BIG_W, pc.BIG_H)]
    got, rest = run_bin2(gpu, frames, 0, 0, True)
    assert (rest == PAD).all()
    for k, f in enumerate(frames):
        assert np.array_equal(got[k], pc.bin2(f)), k
    got, rest = run_bin2(gpu, frames[:1], 2, 2, False)          # the generic form at that size
    assert (rest == PAD).all() and np.array_equal(got[0], pc.bin2(frames[0]))


def test_bin2_dev_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()
    call = lambda sp, st, w, h, dp, ost, n: gpu.mlvfs_amd_bin2_dev(C.c_void_p(sp) if sp else None, st, w, h, C.c_void_p(dp) if dp else None, ost, n, None)
    bad = [(0, 512, 16, 16, d, 128, 1), (s, 512, 16, 16, 0, 128, 1), (s, 512, 3, 16, d, 128, 1), (s, 512, 16, 3, d, 128, 1),
           (s, 512, 1 << 14, 1 << 13, d, 128, 1), (s, 512, 16, 16, d, 128, -1), (s, 510, 16, 16, d, 128, 2), (s, 512, 16, 16, d, 126, 2),
           (s, 513, 16, 16, d, 128, 2), (s + 1, 512, 16, 16, d, 128, 1), (s, 512, 16, 16, d + 1, 128, 1),
           (d + 1024, 512, 16, 16, d + 1024, 128, 1), (d + 1024, 512, 16, 16, d + 1024 + 510, 128, 1), (d + 1024, 512, 16, 16, d + 1024 - 126, 128, 1),
           (d + 1024, 512, 16, 16, d + 1024 + 1024 + 510, 256, 3)]
    for args in bad:
        assert call(*args) == lib.ERR_ARG, args
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    assert call(d + 1024, 512, 16, 16, d + 1024 + 512, 128, 1) == 0      # directly behind the source: no overlap
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:1536] == PAD).all() and (host[1536 + 128:] == PAD).all()
    assert np.array_equal(host[1536:1536 + 128].view(np.uint16), np.full(64, PAD | PAD << 8, np.uint16))      # the mean of four equal pixels


# ------------------------------------------------------------------ the mount
OPTION_SETS = [
    ("none", dict(), False),
    ("cs5+badpix+stripes", dict(cs=5, badpix=1, stripes=1), False),
    ("pnoise+deflicker", dict(pnoise=1, deflicker=3000), False),
    ("dual_iso=1", dict(dual_iso=1), False),
    ("dual_iso=2,amaze", dict(dual_iso=2, hdr_interp=0), False),
    ("cs5+stripes,dark+flat", dict(cs=5, stripes=1), True),
]


def serve(gpu, path, opts, proxy, dark=None, flat=None, lossless=False, order=((2, 3), (0, 2)), batch=2):
    """frames 2..4, then 0..1, in batches of 2, through one fresh handle -> (files, flags or None, results, dng_size)"""
    fresh(gpu)
    r, m = open_mount(path, opts, dark, flat, proxy)
    files, flags, results = [], [], []
    with r, m:
        size = m.dng_size()
        assert size == gpu.mlvfs_amd_mount_dng_size(m.h, 0)
        for first, count in order:
            res = np.full(count, -1, np.int32)
            if lossless:
                a, fa = m.dng_lossless(first, count, batch=batch, results=res)
                files += a
                flags += fa
            else:
                a = m.dng(first, count, batch=batch, results=res)
                assert a.shape == (count, size)
                files += [f.tobytes() for f in a]
            results += list(res)
    return files, (flags if lossless else None), results, size


def fh_of(w, h):
    return SimpleNamespace(rawi_hdr=SimpleNamespace(xRes=w, yRes=h))


def check_proxy(full, proxy, w, h, label):
    """every proxy file against the full-size file of the same frame; -> the proxy frames"""
    pw, ph = pc.proxy_size(w, h)
    out = []
    assert len(full) == len(proxy)
    for k, (f, p) in enumerate(zip(full, proxy)):
        assert len(f) == 65536 + w * h * 2 and len(p) == 65536 + pw * ph * 2, (label, k)
        want = pc.bin2(np.frombuffer(f, "<u2", offset=65536).reshape(h, w))
        got = np.frombuffer(p, "<u2", offset=65536).reshape(ph, pw)
        assert np.array_equal(got, want), f"{label} frame {k}: {(got != want).sum()} proxy pixels are not bin2 of the full-size file's"
        hdr = pc.proxy_header(f[:65536], fh_of(w, h))
        if p[:65536] != hdr:
            bad = np.flatnonzero(np.frombuffer(p[:65536], np.uint8) != np.frombuffer(hdr, np.uint8))
            raise AssertionError(f"{label} frame {k}: the header differs from the rule's in {bad.size} bytes, first at {bad[0]}")
        out.append(got)
    return out


def check_lossless(reference, proxy, files, flags, w, h, label):
    pw, ph = pc.proxy_size(w, h)
    for k, (p, f) in enumerate(zip(proxy, files)):
        assert flags[k] == 0, f"{label} frame {k} fell back"
        v = jpeg_view(np.frombuffer(p, "<u2", offset=65536).reshape(ph, pw))
        assert v.shape == (ph // 2, 2 * pw)
        want = reference.lj92_encode_tile(v, v.shape[1], v.shape[0], 16)
        assert len(f) == 65536 + len(want) and f[65536:] == want, f"{label} frame {k}: the stream differs from the reference's encoding"
        assert f[:65536] == pc.proxy_header_from_proxy(p[:65536], len(want)), f"{label} frame {k}: the lossless header"
        st, back = reference.lj92_decode(f[65536:])
        assert st == 0 and np.array_equal(back, v), (label, k)


CASES = [(p, name, opts, cal) for p in PAYLOADS for name, opts, cal in OPTION_SETS]


@pytest.mark.parametrize("payload,name,opts,cal", CASES, ids=[f"{p}:{name}" for p, name, _, _ in CASES])
def test_mount_proxy_is_the_full_size_file_binned(gpu, reference, tmp_path, payload, name, opts, cal):
    if opts.get("dual_iso"):
        d = dual_clip(tmp_path, payload, reference)
    else:
        d, _ = make_clip(tmp_path, payload, reference=reference)
    path = str(d / NAME)
    with calibration(cal, W, H) as cal_args:
        full, _, res_full, size_full = serve(gpu, path, opts, 1, **cal_args)
        proxy, _, res_proxy, size_proxy = serve(gpu, path, opts, 2, **cal_args)
        files, flags, res_ll, _ = serve(gpu, path, opts, 2, lossless=True, **cal_args)
    assert size_full == 65536 + W * H * 2 and size_proxy == 65536 + (W // 2) * (H // 2) * 2
    assert res_full == res_proxy == res_ll == [1 if opts.get("dual_iso") else 0] * 5
    check_proxy(full, proxy, W, H, f"{payload}:{name}")
    check_lossless(reference, proxy, files, flags, W, H, f"{payload}:{name}")


def plain_clip(tmp_path, frames, name=NAME):
    d = tmp_path / "card"
    d.mkdir(exist_ok=True)
    h, w = frames[0].shape
    mlvfile.write_clip(str(d / name), payloads(frames, "plain")[0], w, h, chunks=2, frame_space=32, shuffle=True)
    return str(d / name)


@pytest.mark.parametrize("w,h", [(64, 48), (pc.DROP_W, pc.DROP_H)], ids=lambda v: str(v))
def test_mount_proxy_at_other_sizes(gpu, reference, tmp_path, w, h):
    """64x48, and a size that drops two columns and two rows"""
    path = plain_clip(tmp_path, [synth.normal_frame(w, h, seed=9, frame=k, hot=8, cold=8) for k in range(5)])
    for opts in (dict(), dict(cs=5, badpix=1, stripes=1)):
        full, _, _, _ = serve(gpu, path, opts, 1)
        proxy, _, _, size = serve(gpu, path, opts, 2)
        assert size == 65536 + 2 * (w // 4) * 2 * (h // 4) * 2
        check_proxy(full, proxy, w, h, f"{w}x{h}")
        files, flags, _, _ = serve(gpu, path, opts, 2, lossless=True)
        check_lossless(reference, proxy, files, flags, w, h, f"{w}x{h}")


def test_mount_proxy_serves_a_class_16_frame_uncompressed(gpu, reference, tmp_path):
    """frame 2's proxy begins with a 0 -- the four pixels that make it are 0 --: the first difference is -32768, class 16"""
    frames = [synth.normal_frame(W, H, seed=9, frame=k, hot=60, cold=60) for k in range(5)]
    frames[2] = frames[2].copy()
    for y, x in ((0, 0), (0, 2), (2, 0), (2, 2)):
        frames[2][y, x] = 0
    assert pc.bin2(frames[2])[0, 0] == 0 and all(pc.bin2(f)[0, 0] != 0 for k, f in enumerate(frames) if k != 2)
    path = plain_clip(tmp_path, frames)
    proxy, _, _, _ = serve(gpu, path, {}, 2, order=((0, 5),), batch=3)
    files, flags, _, _ = serve(gpu, path, {}, 2, lossless=True, order=((0, 5),), batch=3)
    assert flags[2] & 1, "the proxy whose first pixel is 0 must be served uncompressed"
    assert files[2] == proxy[2]
    assert np.array_equal(np.frombuffer(proxy[2], "<u2", offset=65536).reshape(H // 2, W // 2), pc.bin2(frames[2]))
    rest = [k for k in range(5) if k != 2]
    check_lossless(reference, [proxy[k] for k in rest], [files[k] for k in rest], [flags[k] for k in rest], W, H, "neighbours")
    assert all(max_class(files[k][65536:]) < 16 for k in rest)


def test_mount_proxy_calls_of_both_kinds_interleave_in_serve_order(gpu, tmp_path):
    d, _ = make_clip(tmp_path, "plain", n=8)
    path = str(d / NAME)
    opts = dict(cs=5, badpix=1, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, 2, order=((0, 8),), batch=4)
    want_ll, flags_ll, _, _ = serve(gpu, path, opts, 2, lossless=True, order=((0, 8),), batch=4)
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        a, fa = m.dng_lossless(0, 3, batch=2)
        b = m.dng(3, 3, batch=2)
        c, fc_ = m.dng_lossless(6, 2, batch=2)
    assert fa + fc_ == [0] * 5 and flags_ll == [0] * 8
    assert a + c == want_ll[:3] + want_ll[6:] and [f.tobytes() for f in b] == want[3:6]


def test_mount_proxy_strides_set_proxy_after_a_frame_and_factor_1(gpu, tmp_path):
    d, _ = make_clip(tmp_path, "plain", n=4)
    path = str(d / NAME)
    opts = dict(cs=5, stripes=1)
    full, _, _, size_full = serve(gpu, path, opts, 1, order=((0, 4),))
    proxy, _, _, size = serve(gpu, path, opts, 2, order=((0, 4),))
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        out = np.full(4 * size + 64, 0xA5, np.uint8)
        sizes, flags = np.zeros(4, np.uintp), np.zeros(4, np.int32)
        # one byte less than the proxy file: refused, by both calls, nothing written and nothing served
        assert gpu.mlvfs_amd_mount_dng(m.h, 0, 4, lib.ptr(out), size - 1, 2, 0, None) == lib.ERR_ARG
        assert gpu.mlvfs_amd_mount_dng_lossless(m.h, 0, 4, lib.ptr(out), size - 1, lib.ptr(sizes), lib.ptr(flags), 2, 0, None) == lib.ERR_ARG
        assert (out == 0xA5).all()
        m.set_proxy(2)                                           # nothing was served yet
        # exactly the proxy file's size -- far below the full-size file's -- is room enough
        lib.check(gpu.mlvfs_amd_mount_dng(m.h, 0, 2, lib.ptr(out), size, 2, 0, None), "mount_dng")
        assert [out[k * size:(k + 1) * size].tobytes() for k in range(2)] == proxy[:2] and (out[2 * size:] == 0xA5).all()
        lib.check(gpu.mlvfs_amd_mount_dng(m.h, 2, 2, lib.ptr(out), size + 32, 2, 0, None), "mount_dng")      # and anything above
        assert [out[k * (size + 32):k * (size + 32) + size].tobytes() for k in range(2)] == proxy[2:]
        for factor in (1, 2):
            assert gpu.mlvfs_amd_mount_set_proxy(m.h, factor) == lib.ERR_ARG and b"served" in gpu.mlvfs_amd_last_error()
        assert m.dng_size() == size
    # factor 1: today's bytes
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=1)
    with r, m:
        m.set_proxy(2)
        m.set_proxy(1)
        assert m.dng_size() == size_full
        assert [f.tobytes() for f in m.dng(0, 4, batch=2)] == full
        with pytest.raises(lib.MlvfsAmdError):
            m.set_proxy(2)


def test_mount_proxy_full_size(gpu, reference, tmp_path):
    w, h = pc.BIG_W, pc.BIG_H
    frames = [synth.normal_frame(w, h, seed=1, frame=k) for k in range(2)]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, payloads(frames, "plain")[0], w, h)
    opts = dict(cs=5, stripes=1)
    full, _, _, _ = serve(gpu, path, opts, 1, order=((0, 2),))
    proxy, _, _, size = serve(gpu, path, opts, 2, order=((0, 2),))
    assert size == 65536 + 1792 * 660 * 2
    check_proxy(full, proxy, w, h, "3584x1320")
    files, flags, _, _ = serve(gpu, path, opts, 2, lossless=True, order=((0, 2),))
    check_lossless(reference, proxy, files, flags, w, h, "3584x1320")
    print(f"2 frames of {w}x{h}: proxy {size} bytes, lossless proxy {sum(map(len, files)) / 2:.0f} bytes, full size {len(full[0])}")


def test_the_proxy_tool_writes_the_sequence_and_overwrites_nothing(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_proxy.py (its main(), in this process): the files are the proxy handle's, uncompressed and lossless; a second run
    into the same place is refused and leaves the files"""
    import os
    tool = load_tool("mlv_proxy")
    path = plain_clip(tmp_path, [synth.normal_frame(64, 48, seed=9, frame=k, hot=8, cold=8) for k in range(3)])
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, 2, order=((0, 3),))
    want_ll, _, _, _ = serve(gpu, path, opts, 2, lossless=True, order=((0, 3),))
    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2"] + extra)
    for extra, files in (([], want), (["--lossless"], want_ll)):
        out = tmp_path / ("out" + "".join(extra))
        assert run(out, extra) == 0
        names = sorted(os.listdir(out))
        assert names == ["M07-1234_%06d.dng" % k for k in range(3)]
        assert [open(out / n, "rb").read() for n in names] == files
    capsys.readouterr()
    assert run(out, []) == 1 and "nothing is overwritten" in capsys.readouterr().err
    assert [open(out / n, "rb").read() for n in names] == want_ll
