"""Rendered frames resampled from the full-size rendering through the mount (csrc/mount.cpp, csrc/k_resample.hip):
mlvfs_amd_mount_rgb_resampled against a full-size .dng mount of the same clip and options -- the TIFF's pixels are the definition of
mlvfs_amd/resample.py applied to the pixels of the .dng file, with the parameters the tags of that file's header give -- and
mlvfs_amd_mount_jpeg_resampled against mlvfs_amd/jpeg.py's encoding of that rendering; the 16-bit call and a handle's look; results[],
sizes[] and flags[]; PIL opens every file at ow x oh; every kind of call interleaves on one handle, and a handle that never makes a
resampled call is left as it was; strides; the refusals; a failed growth of the full-size buffer; the tool.  The clips, option sets and
helpers are those of tests/mount_harness.py.  All comparisons are for equality."""
import os

import numpy as np
import pytest

from mlvfs_amd import lib, look, resample

import deep_cases as dp
import look_cases as lc
import resample_cases as rs
from mount_harness import (GAIN_A, HDR, OPTION_SETS, PAYLOADS, QUALITY, calibration, check_jpegs, check_tiffs, fresh, load_tool, make_clip,
                           open_mount, renderings, run_tool, serve)

pytestmark = pytest.mark.gpu


def resampled(size, **more):
    return dict(size=size, resample=True, **more)


# every payload kind, both of the mount tests' frame sizes (the fast and the generic form), every option set, each at a size of its own
# above the half size: a ratio of 4 : 3, one more than the half size, the full width at a third of the height, one less a side, the
# full height
SIZES_OF = {(64, 48): [(48, 36), (33, 25), (64, 16), (63, 47), (40, 48)], (418, 266): [(280, 178), (210, 134), (418, 89), (417, 265), (300, 266)]}
CASES = [(pl, w, h, SIZES_OF[(w, h)][k], name, opts, cal) for pl in PAYLOADS for w, h in rs.MOUNT_SIZES for k, (name, opts, cal) in enumerate(OPTION_SETS)]


@pytest.mark.parametrize("payload,w,h,size,name,opts,cal", CASES, ids=[f"{pl}:{w}x{h}->{s[0]}x{s[1]}:{name}" for pl, w, h, s, name, _, _ in CASES])
def test_mount_resampled_is_the_full_size_file_resampled(gpu, reference, tmp_path, payload, w, h, size, name, opts, cal):
    label = f"{payload}:{w}x{h}->{size}:{name}"
    path = make_clip(tmp_path, payload, w, h, dual=bool(opts.get("dual_iso")), reference=reference)
    with calibration(cal, w, h) as cal_args:
        full, _, res_full, _ = serve(gpu, path, opts, "dng", **cal_args)
        tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", resampled(size), **cal_args)
        jpgs, flags, res_jpg, _ = serve(gpu, path, opts, "jpeg", resampled(size), **cal_args)
    assert res_rgb == res_full == res_jpg and all(r in (0, 1) for r in res_full)
    want = renderings(full, gains, w, h, "resampled", size)
    check_tiffs(want, tiffs, size, label)
    check_jpegs(want, jpgs, flags, size, label, QUALITY)
    assert len(set(tiffs)) == len(tiffs), "two frames rendered alike"


@pytest.mark.parametrize("w,h,size", [(64, 48, (48, 36)), (418, 266, (417, 265))], ids=lambda v: str(v))
def test_mount_resampled_with_a_look_and_at_16_bits(gpu, tmp_path, w, h, size):
    path = make_clip(tmp_path, "plain", w, h)
    opts = dict(cs=5, badpix=1, stripes=1)
    name, S, n, T = lc.looks()[1]
    name16, S16, n16, T16 = dp.looks()[1]
    full, _, res_full, _ = serve(gpu, path, opts, "dng")
    with look.Look(S, n, T) as lk, look.Look16(S16, n16, T16) as lk16:
        set_look = lambda m: m.set_look(lk)
        tiffs, _, res_rgb, gains = serve(gpu, path, opts, "rgb", resampled(size), setup=set_look)
        jpgs, flags, _, _ = serve(gpu, path, opts, "jpeg", resampled(size), setup=set_look)
        deep, _, res16, _ = serve(gpu, path, opts, "rgb", resampled(size, look16=lk16), setup=set_look)       # the handle's look does not touch these
    assert res_rgb == res_full == res16
    want = renderings(full, gains, w, h, "resampled", size, look=(S, n, T))
    check_tiffs(want, tiffs, size, name)
    check_jpegs(want, jpgs, flags, size, name, QUALITY)
    check_tiffs(renderings(full, gains, w, h, "resampled", size, look16=(S16, n16, T16)), deep, size, name16, bits=16)


def test_resampled_calls_interleave_with_every_other_kind(gpu, tmp_path):
    w, h = 416, 264
    path = make_clip(tmp_path, "plain", w, h, n=8)
    opts = dict(cs=5, badpix=1, stripes=1)
    order = ((0, 8, GAIN_A),)
    A, B = (300, 190), (416, 88)
    want_dng, _, _, _ = serve(gpu, path, opts, "dng", order=order, batch=4)
    want_half, _, _, _ = serve(gpu, path, opts, "rgb", order=order, batch=4)
    want_a, _, _, gains = serve(gpu, path, opts, "rgb", resampled(A), order=order, batch=4)
    want_b, _, _, _ = serve(gpu, path, opts, "rgb", resampled(B), order=order, batch=4)
    jpg_b, flags, _, _ = serve(gpu, path, opts, "jpeg", resampled(B), order=order, batch=4)
    check_tiffs(renderings(want_dng, gains, w, h, "resampled", A), want_a, A, "one size")
    check_tiffs(renderings(want_dng, gains, w, h, "resampled", B), want_b, B, "another")
    check_jpegs(renderings(want_dng, gains, w, h, "resampled", B), jpg_b, flags, B, "another", QUALITY)
    # the identity size is the full-size call's file
    ident, _, _, _ = serve(gpu, path, opts, "rgb", resampled((w, h)), order=((0, 2, GAIN_A),), batch=2)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        assert [f.tobytes() for f in m.rgb(0, 2, batch=2, full=True)] == ident
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        a = m.rgb(0, 1, batch=2)                                             # half size
        b = m.rgb(1, 2, batch=2, size=A, resample=True)
        c = m.dng(3, 1, batch=2)
        d, _ = m.jpeg(4, 1, quality=QUALITY, batch=2, size=B, resample=True)
        e = m.rgb(5, 1, batch=2, full=True)                                  # the same buffer at another size
        f = m.rgb(6, 1, batch=2, size=(52, 33))                              # the scaled route
        g = m.rgb(7, 1, batch=2, size=B, resample=True)
    assert a[0].tobytes() == want_half[0] and [x.tobytes() for x in b] == want_a[1:3] and c[0].tobytes() == want_dng[3]
    assert d == jpg_b[4:5] and g[0].tobytes() == want_b[7]
    assert np.array_equal(resample.split_file(e[0].tobytes(), w, h), renderings(want_dng[5:6], gains[5:6], w, h, "resampled", (w, h))[0])
    assert np.array_equal(resample.split_file(f[0].tobytes(), 52, 33), renderings(want_dng[6:7], gains[6:7], w, h, "scaled", (52, 33))[0])


def test_a_handle_without_resampled_calls_serves_what_a_fresh_one_does(gpu, tmp_path):
    path = make_clip(tmp_path, "plain", 64, 48, n=6)
    opts = dict(cs=5, stripes=1)

    def run(with_resampled):
        fresh(gpu)
        r, m = open_mount(path, opts)
        out = []
        with r, m:
            out.append(m.dng(0, 2, batch=2).tobytes())
            if with_resampled:
                m.rgb(0, 2, batch=2, size=(50, 40), resample=True)
                m.jpeg(2, 2, batch=2, size=(64, 16), resample=True)
            out.append(m.rgb(2, 2, batch=2).tobytes())
            out.append(b"".join(m.jpeg(4, 1, batch=2)[0]))
            out.append(m.rgb(4, 1, batch=2, full=True).tobytes())
            out.append(m.rgb(4, 1, batch=2, size=(20, 15)).tobytes())
            out.append(b"".join(m.dng_lossless(5, 1, batch=2)[0]))
        return out

    assert run(False) == run(True)


def test_mount_resampled_refusals_strides_and_a_failed_growth(gpu, tmp_path):
    w, h, size = 64, 48, (50, 40)
    path = make_clip(tmp_path, "plain", w, h, n=4)
    opts = dict(cs=5, stripes=1)
    order = ((0, 4, GAIN_A),)
    want, _, _, _ = serve(gpu, path, opts, "rgb", resampled(size), order=order)
    want_jpg, want_fl, _, _ = serve(gpu, path, opts, "jpeg", resampled(size), order=order)
    nbytes = HDR + 50 * 40 * 3
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        out = np.full(4 * (nbytes + 37) + 64, 0xA5, np.uint8)
        call = lambda first, count, stride, ow=50, oh=40: gpu.mlvfs_amd_mount_rgb_resampled(m.h, first, count, lib.ptr(out), stride, 256, ow, oh, 2, 0, None)
        assert call(0, 4, nbytes - 1) == lib.ERR_ARG and (out == 0xA5).all()
        for ow, oh in ((65, 48), (64, 49), (0, 15), (20, -1)):
            assert call(0, 4, 65536, ow, oh) == lib.ERR_ARG and b"resampled" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all(), (ow, oh)
            assert gpu.mlvfs_amd_mount_rgb_resampled_size(m.h, 0, ow, oh) == 0 and gpu.mlvfs_amd_mount_rgb16_resampled_size(m.h, 0, ow, oh) == 0
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), 65536, 0, 50, 40, 2, 0, None) == lib.ERR_ARG          # the gain
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 3, 2, lib.ptr(out), 65536, 256, 50, 40, 2, 0, None) == lib.ERR_ARG        # past the clip
        assert gpu.mlvfs_amd_mount_rgb16_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 50, 40, None, 2, 0, None) == lib.ERR_ARG  # no deep look
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 0, 50, 40, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), 65536, 256, 90, 50, 40, None, lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        with pytest.raises(ValueError):
            m.rgb(0, 1, resample=True)
        with pytest.raises(ValueError):
            m.rgb(0, 1, size=size, full=True, resample=True)
        with pytest.raises(ValueError):
            m.rgb(0, 1, size=size, full=True)                                # as before
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 1, size=(40, 30))                                       # the scaled route keeps refusing sizes above the half size
        # a failed growth of the full-size buffer: every other buffer has its size by now
        m.rgb(0, 2, batch=2)
        gpu.mlvfs_amd_test_fail_next(3)
        assert call(0, 2, nbytes) == lib.ERR_HIP and b"injected" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all()
        lib.check(call(0, 2, nbytes), "mount_rgb_resampled")                 # exactly the file's size
        assert [out[k * nbytes:(k + 1) * nbytes].tobytes() for k in range(2)] == want[:2] and (out[2 * nbytes:] == 0xA5).all()
        out[:] = 0xA5
        st = nbytes + 37                                          # and anything above; the bytes between the files stay
        lib.check(call(2, 2, st), "mount_rgb_resampled")
        assert [out[k * st:k * st + nbytes].tobytes() for k in range(2)] == want[2:]
        assert (out[nbytes:st] == 0xA5).all() and (out[st + nbytes:] == 0xA5).all()
        # a larger size grows the buffer again, a JPEG call puts its streams behind the renderings
        gpu.mlvfs_amd_test_fail_next(3)
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, batch=2, size=(64, 48), resample=True)
        assert m.jpeg(2, 2, quality=QUALITY, batch=2, size=size, resample=True)[0] == want_jpg[2:]
        # sizes[] as the C call reports them
        out[:] = 0xA5
        lib.check(gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), st, 256, QUALITY, 50, 40, lib.ptr(sizes), lib.ptr(fl), 2, 0, None), "mount_jpeg_resampled")
        assert list(sizes) == [len(f) for f in want_jpg[:2]] and list(fl) == want_fl[:2]
        for k in range(2):
            assert out[k * st:k * st + int(sizes[k])].tobytes() == want_jpg[k] and (out[k * st + int(sizes[k]):(k + 1) * st] == 0xA5).all(), k
    fresh(gpu)
    r, m = open_mount(path, opts, proxy=2)
    with r, m:
        out[:] = 0xA5
        sizes, fl = np.full(2, 7, np.uintp), np.full(2, 7, np.int32)
        assert gpu.mlvfs_amd_mount_rgb_resampled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 50, 40, 2, 0, None) == lib.ERR_ARG and b"prox" in gpu.mlvfs_amd_last_error()
        assert gpu.mlvfs_amd_mount_jpeg_resampled(m.h, 0, 2, lib.ptr(out), nbytes, 256, 90, 50, 40, lib.ptr(sizes), lib.ptr(fl), 2, 0, None) == lib.ERR_ARG
        assert b"prox" in gpu.mlvfs_amd_last_error() and (out == 0xA5).all() and list(sizes) == [7, 7] and list(fl) == [7, 7]
        with pytest.raises(lib.MlvfsAmdError):
            m.rgb(0, 2, size=size, resample=True)
        assert m.dng(0, 2, batch=2).shape == (2, 65536 + 32 * 24 * 2)        # the refusal served nothing and spoilt nothing


def test_the_render_tool_resamples(gpu, tmp_path, monkeypatch, capsys):
    """tools/mlv_render.py --resample --size and --fit (its main(), in this process), and what --resample excludes"""
    from PIL import Image
    tool = load_tool("mlv_render")
    path = make_clip(tmp_path, "plain", 64, 48, n=3)
    opts = dict(cs=5, stripes=1)
    want, _, _, _ = serve(gpu, path, opts, "rgb", resampled((50, 40)), order=((0, 3, 1.5),))
    fit = resample.fit(64, 48, 60, 36)
    assert fit == (48, 36)
    want_fit, _, _, _ = serve(gpu, path, opts, "jpeg", resampled(fit), order=((0, 3, 1.5),), quality=90)

    run = lambda out, extra: run_tool(gpu, monkeypatch, tool, [path, out, "--cs", "5", "--stripes", "--batch", "2", "--gain", "1.5"] + extra)
    assert run(tmp_path / "a", ["--resample", "--size", "50x40"]) == 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert [open(tmp_path / "a" / n, "rb").read() for n in names] == want
    with Image.open(tmp_path / "a" / names[0]) as im:
        assert im.mode == "RGB" and im.size == (50, 40)
    assert run(tmp_path / "b", ["--resample", "--fit", "60x36", "--jpeg"]) == 0
    assert [open(tmp_path / "b" / n, "rb").read() for n in sorted(os.listdir(tmp_path / "b"))] == want_fit
    for extra in (["--resample"], ["--resample", "--full"], ["--resample", "--size", "65x48"], ["--size", "50x40"]):
        with pytest.raises(SystemExit):
            run(tmp_path / "c", extra)
    assert not os.path.exists(tmp_path / "c")
    capsys.readouterr()
