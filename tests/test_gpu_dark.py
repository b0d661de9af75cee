"""Dark-frame subtraction and averaging on the GPU (csrc/cal.cpp, csrc/k_cal.hip): the kernels against numpy, and a dark frame in
the mount and in the transcoder against the reference's own process_frame text (oracle/_ref/ref_host_ref) on clips whose payloads
were subtracted beforehand with numpy (tests/dark_cases.py; tests/test_dark_cases.py shows on the CPU that those cases clamp both
ways, hit the rounding boundary and differ from their sources)."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import dark_cases as dc
from dark_cases import NAME
from lossless_cases import jpeg_view
from mount_harness import mount_opts
from test_gpu_mlv_transcode import PAD, device_buffer, lj92_payload_check, plain_payload_check, reference_stream, split
from test_gpu_mount import ORDER, compare
from test_gpu_ref_host import need_hosts, run_host, vpath
from test_mlv_transcode import check_container

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE
FULL = dict(cs=5, badpix=1, stripes=1)


# ---- 1. mlvfs_amd_dark_subtract_dev against numpy ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h,bpp,n,off", dc.SUB_CASES, ids=lambda v: str(v))
def test_subtract_dev_equals_numpy(gpu, w, h, bpp, n, off):
    """Frames at a padded stride; at byte offset 0 (16 x 2, 48 x 6 and 416 x 264 take the 16-pixel form) and 2 (the pixel-per-lane
    form); no byte outside the frames changes."""
    import torch
    black_d = dc.clip_black(bpp) + off
    frames, dark, want = dc.sub_case(w, h, bpp, n, black_d)
    size, stride = w * h * 2, w * h * 2 + 512
    geom = lib.Geom(w, h, bpp, 0, 0, 0, 0)
    with Dark.from_plane(dark, bpp, black_d) as d:
        for offset in (0, 2):
            buf = device_buffer(torch, frames, stride, offset)
            lib.check(gpu.mlvfs_amd_dark_subtract_dev(d.h, C.byref(geom), C.c_void_p(buf.data_ptr() + offset), stride, n, None), "dark_subtract")
            torch.cuda.synchronize()
            got, rest = split(buf, n, stride, size, offset)
            assert (rest == PAD).all(), offset                              # pad bytes between and around the frames
            for k in range(n):
                g = got[k].view(np.uint16).reshape(h, w)
                assert np.array_equal(g, want[k]), (offset, k, int((g != want[k]).sum()))


# ---- 2. averaging against numpy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("payload", ["plain", "lzma", "lj92"])
@pytest.mark.parametrize("w,h", dc.AVG_GEOMETRIES, ids=lambda v: str(v))
def test_mean_of_a_clip_equals_numpy(gpu, request, tmp_path, payload, w, h):
    """One clip: a lead frame, then the frames of the 1-, 2- and 7-frame cases; batches of 3, so 7 frames cross batch boundaries."""
    reference = request.getfixturevalue("reference") if payload == "lzma" else None
    lead = [synth.normal_frame(w, h, seed=4)]
    cases = [dc.avg_case(w, h, n) for n in dc.AVG_COUNTS]
    frames = lead + [f for fs, _ in cases for f in fs]
    d = dc.write_clip(tmp_path / "card", frames, payload, reference)
    with mlvfile.MlvReader(str(d / NAME)) as r:
        first = 1
        for (fs, want), n in zip(cases, dc.AVG_COUNTS):
            with Dark.from_clip(r, first, n, batch=3, io_threads=2) as dark:
                assert dark.info() == dict(width=w, height=h, bpp=14, black=2048, frames_averaged=n)
                got = dark.plane()
                assert np.array_equal(got, want), (n, int((got != want).sum()))
            first += n
        with Dark.from_clip(r, batch=4) as dark:                             # the whole clip, from frame 0
            assert dark.info()["frames_averaged"] == len(frames) and np.array_equal(dark.plane(), dc.mean(frames))
        for first, count in ((0, len(frames) + 1), (len(frames) - 1, 2), (0, 65537)):
            assert gpu.mlvfs_amd_dark_from_clip(r.h, first, count, 3, 2) is None, (first, count)


# ---- 3. the mount ---------------------------------------------------------------------------------------------------------
_cases = {}


def clip_case(kind, black_d=BLACK):
    if (kind, black_d) not in _cases:
        _cases[kind, black_d] = dc.clip_case(kind, black_d=black_d)
    return _cases[kind, black_d]


def serve(gpu, d, opts, dark, lossless=False):
    """frames 2..4, then 0..1, in batches of 2, through one fresh mount (test_gpu_mount.serve with a dark frame)"""
    gpu.free_focus_pixel_maps()
    gpu.mlvfs_amd_dualiso_reset()
    opt, defl, fps = mount_opts(opts)
    with mlvfile.MlvReader(str(d / NAME)) as r, Mount(r, opt, deflicker=defl, fps=fps, basename="/" + NAME, dark=dark) as m:
        if lossless:
            a, fa = m.dng_lossless(2, 3, batch=2)
            b, fb = m.dng_lossless(0, 2, batch=2)
            return a + b, fa + fb
        files = np.concatenate([m.dng(2, 3, batch=2), m.dng(0, 2, batch=2)])
    return [(f[65536:].tobytes(), f[:65536].tobytes()) for f in files]


MOUNT_CASES = [
    ("plain", "plain", BLACK, dict()),
    ("plain", "plain", BLACK, FULL),
    ("plain", "lzma", BLACK, FULL),
    ("plain", "lj92", BLACK, FULL),
    ("plain", "plain", BLACK - 48, FULL),
    ("plain", "plain", BLACK, dict(pnoise=1, deflicker=3000)),
    ("dual_iso", "plain", BLACK, dict(dual_iso=2)),
]


@pytest.mark.parametrize("kind,payload,black_d,opts", MOUNT_CASES,
                         ids=[f"{k}:{p}:{b}:" + ",".join(f"{a}={v}" for a, v in o.items()) for k, p, b, o in MOUNT_CASES])
def test_mount_with_a_dark_frame_serves_the_reference_files_of_the_subtracted_clip(gpu, request, tmp_path, kind, payload, black_d, opts):
    need_hosts()
    reference = request.getfixturevalue("reference") if payload == "lzma" else None
    frames, plane, pre = clip_case(kind, black_d)
    src = dc.write_clip(tmp_path / "card", frames, payload, reference)
    sub = dc.write_clip(tmp_path / "pre", pre)
    want, _ = run_host("ref", sub, tmp_path / "ref", opts, [vpath(k) for k in ORDER])
    with Dark.from_plane(plane, 14, black_d) as dark:
        compare("the reference on the subtracted clip", want, serve(gpu, src, opts, dark))


def test_mount_lossless_with_a_dark_frame_decodes_to_the_same_pixels(gpu, reference, tmp_path):
    need_hosts()
    frames, plane, pre = clip_case("plain")
    src = dc.write_clip(tmp_path / "card", frames)
    sub = dc.write_clip(tmp_path / "pre", pre)
    want, _ = run_host("ref", sub, tmp_path / "ref", FULL, [vpath(k) for k in ORDER])
    with Dark.from_plane(plane, 14, BLACK) as dark:
        files, flags = serve(gpu, src, FULL, dark, lossless=True)
    assert flags == [0] * 5
    for k, (f, (data, _)) in enumerate(zip(files, want)):
        st, back = reference.lj92_decode(f[65536:])
        assert len(f) < 65536 + len(data) and st == 0, k
        assert np.array_equal(back, jpeg_view(np.frombuffer(data, "<u2").reshape(dc.H, dc.W))), k


# ---- 4. the transcoder ----------------------------------------------------------------------------------------------------
def transcode(src_dir, out_dir, lj92, dark, batch=2):
    out_dir.mkdir()
    with mlvfile.MlvReader(str(src_dir / NAME)) as r:
        return r.transcode(str(out_dir / NAME), lj92=lj92, batch=batch, io_threads=3, dark=dark)


_streams = {}


@pytest.mark.parametrize("payload", ["plain", "lzma", "lj92"])
def test_lj92_output_with_a_dark_frame(gpu, reference, tmp_path, payload):
    """every payload: [u32 w * h * 2][the reference encoder's stream of the quadrant-tiled SUBTRACTED frame]"""
    frames, plane, pre = clip_case("plain")
    if not _streams:
        _streams["s"] = [reference_stream(reference, p, 14) for p in pre]
    src = dc.write_clip(tmp_path / "card", frames, payload, reference)
    with Dark.from_plane(plane, 14, BLACK) as dark:
        stats = transcode(src, tmp_path / "out", True, dark)
    seen = check_container(str(src / NAME), str(tmp_path / "out" / NAME), 2, 0x101, lj92_payload_check(pre, _streams["s"]))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)


@pytest.mark.parametrize("payload,black_d", [("plain", BLACK), ("plain", BLACK - 48), ("lzma", BLACK), ("lj92", BLACK)])
def test_plain_output_with_a_dark_frame_is_the_packed_subtracted_frame(gpu, request, tmp_path, payload, black_d):
    reference = request.getfixturevalue("reference") if payload == "lzma" else None
    frames, plane, pre = clip_case("plain", black_d)
    src = dc.write_clip(tmp_path / "card", frames, payload, reference)
    with Dark.from_plane(plane, 14, black_d) as dark:
        stats = transcode(src, tmp_path / "out", False, dark, batch=3)
    seen = check_container(str(src / NAME), str(tmp_path / "out" / NAME), 2, 1, plain_payload_check(pre))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)


@pytest.mark.parametrize("lj92", [True, False], ids=["lj92", "plain"])
def test_the_reference_text_serves_the_output_as_it_serves_the_subtracted_clip(gpu, tmp_path, lj92):
    need_hosts()
    frames, plane, pre = clip_case("plain")
    src = dc.write_clip(tmp_path / "card", frames)
    sub = dc.write_clip(tmp_path / "pre", pre)
    with Dark.from_plane(plane, 14, BLACK) as dark:
        transcode(src, tmp_path / "out", lj92, dark, batch=8)
    order = [vpath(2), vpath(0), vpath(4), vpath(1), vpath(3)]
    want, _ = run_host("ref", sub, tmp_path / "a", FULL, order)
    got, _ = run_host("ref", tmp_path / "out", tmp_path / "b", FULL, order)
    assert got == want


# ---- 4b. other bit depths and the two-pass fallback, through the reader's load ------------------------------------------------
@pytest.mark.parametrize("w,h,bpp", dc.DEPTH_CASES, ids=lambda v: str(v))
def test_plain_output_with_a_dark_frame_at_other_depths_and_sizes(gpu, tmp_path, w, h, bpp):
    """12 and 10 bits: k_cal_unpack_x16<12 | 10, true, false>; 16 bits and 30 x 12: k_unpack_generic, then k_cal_apply.  Every payload is the
    packed numpy-subtracted frame."""
    frames, plane, black_d, pre = dc.depth_case(w, h, bpp)
    src = dc.write_clip(tmp_path / "card", frames, bpp=bpp)
    with Dark.from_plane(plane, bpp, black_d) as dark:
        stats = transcode(src, tmp_path / "out", False, dark, batch=2)
    seen = check_container(str(src / NAME), str(tmp_path / "out" / NAME), 2, 1, plain_payload_check(pre, bpp))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)


@pytest.mark.parametrize("w,h,bpp", [c for c in dc.DEPTH_CASES if c[2] != 16], ids=lambda v: str(v))
def test_mount_with_a_dark_frame_at_other_depths_and_sizes(gpu, tmp_path, w, h, bpp):
    """the mount without options against the reference's process_frame text on the pre-subtracted clip, header and pixels"""
    need_hosts()
    frames, plane, black_d, pre = dc.depth_case(w, h, bpp)
    src = dc.write_clip(tmp_path / "card", frames, bpp=bpp)
    sub = dc.write_clip(tmp_path / "pre", pre, bpp=bpp)
    order = [1, 2, 0]
    want, _ = run_host("ref", sub, tmp_path / "ref", {}, [vpath(k) for k in order])
    gpu.free_focus_pixel_maps()
    with Dark.from_plane(plane, bpp, black_d) as dark, mlvfile.MlvReader(str(src / NAME)) as r, \
            Mount(r, MlvfsOptions(), basename="/" + NAME, dark=dark) as m:
        files = np.concatenate([m.dng(1, 2, batch=2), m.dng(0, 1)])
    for k, f, (data, hdr) in zip(order, files, want):
        g = f[65536:].view("<u2").reshape(h, w)
        assert np.array_equal(g, pre[k]), (k, int((g != pre[k]).sum()))     # numpy's subtraction ...
        assert f[65536:].tobytes() == data and f[:65536].tobytes() == hdr, k  # ... and the reference's file of the subtracted clip


# ---- 5. refusals and state ------------------------------------------------------------------------------------------------
def test_set_dark_refusals_and_clearing(gpu, tmp_path):
    frames, plane, pre = clip_case("plain")
    src = dc.write_clip(tmp_path / "card", frames)
    opt = MlvfsOptions(chroma_smooth=2)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(src / NAME)) as r, Dark.from_plane(plane, 14, BLACK) as dark:
        with Mount(r, opt, basename="/" + NAME) as m:
            plain = m.dng(0, 2, batch=2)
            with pytest.raises(lib.MlvfsAmdError, match="served"):            # after a frame was served
                m.set_dark(dark)
            assert gpu.mlvfs_amd_mount_set_dark(m.h, None) == lib.ERR_ARG
            assert np.array_equal(m.dng(0, 2, batch=2), plain)
        with Mount(r, opt, basename="/" + NAME, dark=dark) as m:
            m.set_dark(None)                                                 # NULL on a fresh mount: a mount without a dark frame
            assert np.array_equal(m.dng(0, 2, batch=2), plain)
        with Mount(r, opt, basename="/" + NAME, dark=dark) as m:
            assert not np.array_equal(m.dng(0, 2, batch=2), plain)
        for shape, bpp in (((dc.H, dc.W - 16), 14), ((dc.H - 2, dc.W), 14), ((dc.H, dc.W), 12)):
            with Dark.from_plane(np.full(shape, 2048, np.uint16), bpp, BLACK) as other:
                with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                    Mount(r, opt, dark=other)
                with Mount(r, opt) as m:
                    assert gpu.mlvfs_amd_mount_set_dark(m.h, other.h) == lib.ERR_ARG
                    assert np.array_equal(m.dng(0, 2, batch=2)[:, 65536:], plain[:, 65536:])     # the mount stays what it was
                for lj92 in (True, False):
                    with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                        r.transcode(str(out / NAME), lj92=lj92, dark=other)
                    assert os.listdir(out) == []


# ---- 6. full size ---------------------------------------------------------------------------------------------------------
def test_full_size_frames(gpu, oracle, tmp_path):
    """3584 x 1320, two frames, the 16-pixel forms: subtract_dev against numpy, and one mount call with cs5x5 + stripes against the
    oracle applied to the subtracted frames."""
    import torch
    w, h = 3584, 1320
    frames, plane, pre = dc.clip_case("plain", n=2, w=w, h=h)
    for f, p in zip(frames, pre):
        lo, hi, mid = dc.clamp_classes(f, plane, BLACK, 14)
        assert lo > 0 and hi > 0 and mid > 0
    size, stride = w * h * 2, w * h * 2 + 256
    geom = lib.Geom(w, h, 14, 0, 0, 0, 0)
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)
    with Dark.from_plane(plane, 14, BLACK) as dark:
        buf = device_buffer(torch, frames, stride)
        lib.check(gpu.mlvfs_amd_dark_subtract_dev(dark.h, C.byref(geom), C.c_void_p(buf.data_ptr()), stride, 2, None), "dark_subtract")
        torch.cuda.synchronize()
        got, rest = split(buf, 2, stride, size)
        assert (rest == PAD).all()
        for k in range(2):
            assert np.array_equal(got[k].view(np.uint16).reshape(h, w), pre[k]), k
        gpu.free_focus_pixel_maps()
        with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions(chroma_smooth=5, fix_stripes=1), basename="/B.MLV", dark=dark) as m:
            files = m.dng(0, 2, batch=2)
    corr = None
    for k in range(2):
        img = oracle.chroma_smooth(pre[k], BLACK, 5)
        if corr is None:
            corr = oracle.stripes_compute(img, BLACK, WHITE, frame_size=w * h * 14 // 8)
        want = oracle.stripes_apply(img, BLACK, WHITE, *corr)
        g = files[k, 65536:].view(np.uint16).reshape(h, w)
        assert np.array_equal(g, want), (k, int((g != want).sum()))
