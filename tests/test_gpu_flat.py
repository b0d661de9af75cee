"""Flat-field correction on the GPU (csrc/cal.cpp, csrc/k_cal.hip): the gain kernels and the apply kernels against
numpy (tests/flat_cases.py), and a flat field -- with and without a dark frame -- in the mount and in the transcoder against the
reference's own process_frame text (oracle/_ref/ref_host_ref) and the reference's encoder on clips whose payloads were corrected
beforehand with numpy.  tests/test_flat_cases.py shows on the CPU that those cases reach the cap, s = 1, both roundings, both clamps,
floor against truncation and products and sums beyond 32 bits, and that the corrected clips differ from their sources."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.flat import Flat
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import bits_cases as bc
import dark_cases as dc
import flat_cases as fc
from flat_cases import NAME
from lossless_cases import jpeg_view
from mount_harness import mount_opts
from test_gpu_bits import check_output, files_of
from test_gpu_mlv_transcode import PAD, device_buffer, lj92_payload_check, plain_payload_check, reference_stream, split
from test_gpu_mount import ORDER, compare
from test_gpu_ref_host import need_hosts, run_host, vpath
from test_mlv_transcode import blocks_of, check_container

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE
FULL = dict(cs=5, badpix=1, stripes=1)


def source_clip(d, frames, payload="plain", reference=None, bpp=14, black=None):
    """dark_cases.write_clip's clip (the levels of 14 bits scaled to bpp, or `black`), its LJ92 payloads encoded once per material"""
    shift = 14 - bpp
    b, w = (BLACK >> shift, WHITE >> shift) if shift >= 0 else (BLACK << -shift, WHITE << -shift)
    return bc.write_clip(d, frames, bpp, payload, reference, black=b if black is None else black, white=w)


# ---- 1. the gain plane on the GPU ----------------------------------------------------------------------------------------------
GAIN_CASES = [(3, 16, 14, None, "plain", 1), (30, 12, 14, None, "plain", 3), (64, 48, 14, None, "plain", 1), (64, 48, 14, None, "plain", 3),
              (64, 48, 14, None, "lzma", 1), (64, 48, 14, None, "lzma", 3), (64, 48, 14, None, "lj92", 1), (64, 48, 14, None, "lj92", 3),
              (640, 480, 16, 0, "plain", 1)]


@pytest.mark.parametrize("dark", [False, True], ids=["flat", "dark+flat"])
@pytest.mark.parametrize("w,h,bpp,black,payload,n", GAIN_CASES, ids=lambda v: str(v))
def test_gain_of_a_clip_equals_the_host_and_numpy(gpu, request, tmp_path, w, h, bpp, black, payload, n, dark):
    """3 x 16: an odd width with w * h a multiple of 16 (the channel pattern changes inside a lane's 16 pixels); 30 x 12: a short last
    group; 640 x 480 at 16 bits with black_f = 0: a channel sum beyond 2^32.  One frame: the tuned plane itself (both roundings of both
    divisions); three: their rounded mean.  With a dark frame: subtracted from the mean plane first."""
    reference = request.getfixturevalue("reference") if payload == "lzma" else None
    black_f = dc.clip_black(bpp) if black is None else black
    if (w, h, bpp) == (640, 480, 16):
        frames = [fc.overflow_plane()]
    else:
        frames = [fc.flat_plane(w, h, bpp, black_f, seed=5 + k) for k in range(n)]
    src = source_clip(tmp_path / "flat", frames, payload, reference, bpp, black_f)
    mean = dc.mean(frames)
    assert n > 1 or np.array_equal(mean, frames[0])
    rng = np.random.default_rng(w + h)
    black_d = black_f + 9
    plane_d = np.clip(black_d + rng.integers(-6, 7, (h, w)), 0, (1 << bpp) - 1).astype(np.uint16)
    if dark:
        plane_d[0, 0], plane_d[-1, -1] = (1 << bpp) - 5, black_d // 4       # a mean entry that clamps at 0 -> s = 1; one lifted
        mean = dc.subtract(mean, plane_d, black_d, bpp)
    want = fc.gains(mean, black_f)
    with mlvfile.MlvReader(str(src / NAME)) as r, Dark.from_plane(plane_d, bpp, black_d) as d:
        with Flat.from_clip(r, dark=d if dark else None, batch=2, io_threads=2) as f, Flat.from_plane(mean, bpp, black_f) as host:
            assert f.info() == dict(width=w, height=h, bpp=bpp, black=black_f, frames_averaged=n, means=fc.channel_means(mean, black_f))
            got = f.gain()
            assert np.array_equal(got, want), int((got != want).sum())
            assert np.array_equal(host.gain(), got) and host.info()["means"] == f.info()["means"]
    if (w, h, bpp) == (640, 480, 16):
        assert max(fc.channel_sums(mean, black_f)[0]) >= 1 << 32


# ---- 2. mlvfs_amd_flat_apply_dev against numpy --------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,bpp,n,dark", fc.APPLY_CASES, ids=lambda v: str(v))
def test_apply_dev_equals_numpy(gpu, w, h, bpp, n, dark):
    """Frames at a padded stride; at byte offset 0 (16 x 2, 48 x 6 and 416 x 264 up to 14 bits take k_cal_apply_x16<DARK, true>) and 2,
    2 x 2, 30 x 10 and every 16-bit case (k_cal_apply_generic: 64-bit products); the flat plane is a 14-bit one whatever the
    frames' depth; no byte outside the frames changes."""
    import torch
    c = fc.apply_case(w, h, bpp, n, dark)
    size, stride = w * h * 2, w * h * 2 + 512
    geom = lib.Geom(w, h, bpp, c["black"], 0, 0, 0)
    with Flat.from_plane(c["F"], 14, c["black_f"]) as f, Dark.from_plane(c["dark"] if dark else np.zeros((h, w), np.uint16), bpp, c["black_d"] or 0) as d:
        assert f.info()["bpp"] == 14
        for offset in (0, 2):
            buf = device_buffer(torch, c["frames"], stride, offset)
            lib.check(gpu.mlvfs_amd_flat_apply_dev(f.h, d.h if dark else None, C.byref(geom), C.c_void_p(buf.data_ptr() + offset), stride, n, None),
                      "flat_apply")
            torch.cuda.synchronize()
            got, rest = split(buf, n, stride, size, offset)
            assert (rest == PAD).all(), offset                              # pad bytes between and around the frames
            for k in range(n):
                g = got[k].view(np.uint16).reshape(h, w)
                assert np.array_equal(g, c["want"][k]), (offset, k, int((g != c["want"][k]).sum()))


def test_apply_dev_takes_values_above_the_depth_as_the_top(gpu):
    """12-bit frames that hold values up to 65535, as a damaged LJ92 stream can decode to: every form gives the oracle's result for
    min(px, 4095) -- the 16-pixel form's 32-bit products included (offset 0), where 65535 * a gain near 4.0 would wrap --, with a
    dark frame (whose clamp does it) and without."""
    import torch
    w, h, bpp, n = 48, 6, 12, 2
    for dark in (False, True):
        c = fc.apply_case(w, h, bpp, n, dark)
        rng = np.random.default_rng(8)
        frames = [f.copy() for f in c["frames"]]
        for f in frames:
            at = rng.choice(w * h, 60, replace=False)
            f.reshape(-1)[at] = rng.integers(4096, 65536, 60)
            f[-1, -1], f[0, 0] = 65535, 65535                                # under the gain cap and under a gain of 2
        want = [fc.correct(f, c["gain"], c["black"], bpp, c["dark"], c["black_d"]) for f in frames]
        assert all(np.array_equal(wnt, fc.correct(np.minimum(f, 4095), c["gain"], c["black"], bpp)) for f, wnt in zip(frames, want)) or dark
        size, stride = w * h * 2, w * h * 2 + 512
        geom = lib.Geom(w, h, bpp, c["black"], 0, 0, 0)
        with Flat.from_plane(c["F"], 14, c["black_f"]) as f, Dark.from_plane(c["dark"] if dark else np.zeros((h, w), np.uint16), bpp, c["black_d"] or 0) as d:
            for offset in (0, 2):
                buf = device_buffer(torch, frames, stride, offset)
                lib.check(gpu.mlvfs_amd_flat_apply_dev(f.h, d.h if dark else None, C.byref(geom), C.c_void_p(buf.data_ptr() + offset), stride, n, None),
                          "flat_apply")
                torch.cuda.synchronize()
                got, rest = split(buf, n, stride, size, offset)
                assert (rest == PAD).all()
                for k in range(n):
                    g = got[k].view(np.uint16).reshape(h, w)
                    assert np.array_equal(g, want[k]), (dark, offset, k, int((g != want[k]).sum()))


# ---- 3. the load, through the mount and the plain transcode: other depths, sizes and the two-pass fallback --------------------
def planes_of(plane_d, bpp, black_d):
    """-> a Dark for the plane, or one that is never used"""
    return Dark.from_plane(plane_d if plane_d is not None else np.zeros((1, 1), np.uint16), bpp, black_d)


@pytest.mark.parametrize("dark", [False, True], ids=["flat", "dark+flat"])
@pytest.mark.parametrize("w,h,bpp", fc.DEPTH_CASES, ids=lambda v: str(v))
def test_the_load_at_other_depths_and_sizes(gpu, tmp_path, w, h, bpp, dark):
    """12 and 10 bits at 416 x 264: k_cal_unpack_x16<12 | 10, DARK, true>; 16 bits and 30 x 12: k_unpack_generic, then the apply pass.  The
    flat is a 14-bit one.  The mount without options against the reference's process_frame text on the pre-corrected clip (header and
    pixels), and the plain transcode against the packed corrected frames."""
    need_hosts()
    frames, F, plane_d, black_d, pre = fc.depth_case(w, h, bpp, dark)
    src = source_clip(tmp_path / "card", frames, bpp=bpp)
    cor = source_clip(tmp_path / "pre", pre, bpp=bpp)
    order = [1, 2, 0]
    want, _ = run_host("ref", cor, tmp_path / "ref", {}, [vpath(k) for k in order])
    gpu.free_focus_pixel_maps()
    with Flat.from_plane(F, 14, BLACK) as flat, planes_of(plane_d, bpp, black_d) as d, mlvfile.MlvReader(str(src / NAME)) as r:
        with Mount(r, MlvfsOptions(), basename="/" + NAME, dark=d if dark else None, flat=flat) as m:
            files = np.concatenate([m.dng(1, 2, batch=2), m.dng(0, 1)])
        (tmp_path / "out").mkdir()
        stats = r.transcode(str(tmp_path / "out" / NAME), lj92=False, batch=2, io_threads=3, dark=d if dark else None, flat=flat)
    for k, f, (data, hdr) in zip(order, files, want):
        g = f[65536:].view("<u2").reshape(h, w)
        assert np.array_equal(g, pre[k]), (k, int((g != pre[k]).sum()))      # numpy's correction ...
        assert f[65536:].tobytes() == data and f[:65536].tobytes() == hdr, k  # ... and the reference's file of the corrected clip
    seen = check_container(str(src / NAME), str(tmp_path / "out" / NAME), 2, 1, plain_payload_check(pre, bpp))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)


# ---- 4. the mount at 416 x 264 ------------------------------------------------------------------------------------------------
_cases = {}


def clip_case(kind, dark=False):
    if (kind, dark) not in _cases:
        _cases[kind, dark] = fc.clip_case(kind, dark=dark)
    return _cases[kind, dark]


def serve(gpu, d, opts, dark, flat, lossless=False):
    """frames 2..4, then 0..1, in batches of 2, through one fresh mount (test_gpu_mount.serve with a flat field)"""
    gpu.free_focus_pixel_maps()
    gpu.mlvfs_amd_dualiso_reset()
    opt, defl, fps = mount_opts(opts)
    with mlvfile.MlvReader(str(d / NAME)) as r, Mount(r, opt, deflicker=defl, fps=fps, basename="/" + NAME, dark=dark, flat=flat) as m:
        if lossless:
            a, fa = m.dng_lossless(2, 3, batch=2)
            b, fb = m.dng_lossless(0, 2, batch=2)
            return a + b, fa + fb
        files = np.concatenate([m.dng(2, 3, batch=2), m.dng(0, 2, batch=2)])
    return [(f[65536:].tobytes(), f[:65536].tobytes()) for f in files]


MOUNT_CASES = [
    ("plain", "plain", False, dict()),
    ("plain", "plain", False, FULL),
    ("plain", "lzma", False, FULL),
    ("plain", "lj92", False, FULL),
    ("plain", "plain", True, FULL),
    ("plain", "lj92", True, FULL),                                           # dark and flat in ONE pass behind the decoder
    ("plain", "lzma", True, FULL),
    ("plain", "plain", False, dict(pnoise=1, deflicker=3000)),
    ("dual_iso", "plain", False, dict(dual_iso=2)),
]


@pytest.mark.parametrize("kind,payload,dark,opts", MOUNT_CASES,
                         ids=[f"{k}:{p}:{'dark+flat' if d else 'flat'}:" + ",".join(f"{a}={v}" for a, v in o.items()) for k, p, d, o in MOUNT_CASES])
def test_mount_with_a_flat_field_serves_the_reference_files_of_the_corrected_clip(gpu, request, tmp_path, kind, payload, dark, opts):
    need_hosts()
    reference = request.getfixturevalue("reference") if payload == "lzma" else None
    frames, F, plane_d, pre = clip_case(kind, dark)
    src = source_clip(tmp_path / "card", frames, payload, reference)
    cor = source_clip(tmp_path / "pre", pre)
    want, _ = run_host("ref", cor, tmp_path / "ref", opts, [vpath(k) for k in ORDER])
    with Flat.from_plane(F, 14, BLACK) as flat, planes_of(plane_d, 14, BLACK) as d:
        compare("the reference on the corrected clip", want, serve(gpu, src, opts, d if dark else None, flat))


def test_mount_lossless_with_a_flat_field_decodes_to_the_same_pixels(gpu, reference, tmp_path):
    need_hosts()
    frames, F, _, pre = clip_case("plain")
    src = source_clip(tmp_path / "card", frames)
    cor = source_clip(tmp_path / "pre", pre)
    want, _ = run_host("ref", cor, tmp_path / "ref", FULL, [vpath(k) for k in ORDER])
    with Flat.from_plane(F, 14, BLACK) as flat:
        files, flags = serve(gpu, src, FULL, None, flat, lossless=True)
    assert flags == [0] * 5
    for k, (f, (data, _)) in enumerate(zip(files, want)):
        st, back = reference.lj92_decode(f[65536:])
        assert len(f) < 65536 + len(data) and st == 0, k
        assert np.array_equal(back, jpeg_view(np.frombuffer(data, "<u2").reshape(fc.H, fc.W))), k


# ---- 5. the transcoder --------------------------------------------------------------------------------------------------------
_streams, _served, _small = {}, {}, {}
TIE_ORDER = [vpath(2), vpath(0), vpath(4), vpath(1), vpath(3)]


def transcode_case(size, dark):
    """-> (frames, F, dark plane or None, the corrected frames) with the levels of bits_cases (black 2047), 416 x 264 or 64 x 48"""
    if (size, dark) not in _small:
        w, h = size
        frames = dc.clip_frames("plain", 5, w, h)
        F = fc.clip_flat(w, h)
        plane_d = dc.dark_plane(w, h) if dark else None
        g = fc.gains(F, BLACK)
        _small[size, dark] = (frames, F, plane_d, [fc.correct(f, g, bc.BLACK14, 14, plane_d, BLACK - 48) for f in frames])
    return _small[size, dark]


def transcode(src_dir, out_dir, lj92_out, bits, dark, flat, batch=2):
    out_dir.mkdir()
    with mlvfile.MlvReader(str(src_dir / NAME)) as r:
        return r.transcode(str(out_dir / NAME), lj92=lj92_out, batch=batch, io_threads=3, dark=dark, bits=bits, flat=flat)


ROUTES = [("plain", True), ("lj92", True), ("plain", False), ("lj92", False)]


@pytest.mark.parametrize("bits_dark", [False, True], ids=["own-depth", "dark+flat->12"])
@pytest.mark.parametrize("kind,lj92_out", ROUTES, ids=[f"{k}->{'lj92' if l else 'plain'}" for k, l in ROUTES])
@pytest.mark.parametrize("size", [(64, 48), (416, 264)], ids=lambda v: str(v))
def test_the_transcoder_with_a_flat_field(gpu, reference, tmp_path, size, kind, lj92_out, bits_dark):
    """LJ92 output: [u32 w * h * 2][the reference encoder's stream of the quadrant-tiled CORRECTED frame]; plain output: the packed
    corrected frame.  With out_bpp = 12 and a dark frame (pedestal 48 below the clip's black level) the order is dark, flat, shift:
    bits_cases.convert of the corrected frames, the RAWI block rewritten.  And the reference's reader and process_frame text serve the
    output as they serve the expected clip."""
    need_hosts()
    frames, F, plane_d, pre = transcode_case(size, bits_dark)
    out_bpp = 12 if bits_dark else 14
    src = bc.write_clip(tmp_path / "card", frames, 14, kind)
    with Flat.from_plane(F, 14, BLACK) as flat, planes_of(plane_d, 14, BLACK - 48) as d:
        stats = transcode(src, tmp_path / "out", lj92_out, 12 if bits_dark else None, d if bits_dark else None, flat, batch=3)
    assert any(not np.array_equal(p, f) for p, f in zip(pre, frames))
    check_output(reference, tmp_path, src, tmp_path / "out", stats, pre, 14, out_bpp, lj92_out, ("flat", size, bits_dark))
    key = (size, bits_dark)
    if key not in _served:
        _served[key] = run_host("ref", tmp_path / "want_out", tmp_path / "a", FULL, TIE_ORDER)[0]     # check_output's expected clip
    got, _ = run_host("ref", tmp_path / "out", tmp_path / "b", FULL, TIE_ORDER)
    assert got == _served[key]


# ---- 6. unchanged behaviour without a flat field ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,lj92_out,bits,dark", [("plain", False, None, False), ("plain", True, None, False), ("plain", False, 12, True),
                                                    ("lj92", True, 12, True), ("lj92", False, None, True)],
                         ids=["plain->plain", "plain->lj92", "plain->plain:dark:12", "lj92->lj92:dark:12", "lj92->plain:dark"])
def test_no_flat_is_transcode_bits_and_a_constant_flat_changes_nothing(gpu, tmp_path, kind, lj92_out, bits, dark):
    frames, plane_d, _ = dc.clip_case("plain", w=64, h=48)
    src = bc.write_clip(tmp_path / "card", frames, 14, kind)
    payload = lib.MLV_LJ92 if lj92_out else lib.MLV_PLAIN
    for name in ("bits", "null", "const"):
        (tmp_path / name).mkdir()
    st = [(C.c_longlong * 4)() for _ in range(2)]
    with mlvfile.MlvReader(str(src / NAME)) as r, Dark.from_plane(plane_d, 14, BLACK) as d, \
            Flat.from_plane(fc.constant_plane(64, 48, 4321), 12, 512) as const:
        dh = d.h if dark else None
        assert (const.gain() == fc.ONE).all()
        lib.check(gpu.mlvfs_amd_mlv_transcode_bits(r.h, os.fsencode(str(tmp_path / "bits" / NAME)), payload, bits or 0, dh, 2, 2, st[0]), "bits")
        lib.check(gpu.mlvfs_amd_mlv_transcode_cal(r.h, os.fsencode(str(tmp_path / "null" / NAME)), payload, bits or 0, dh, None, 2, 2, st[1]), "cal")
        stats = r.transcode(str(tmp_path / "const" / NAME), lj92=lj92_out, batch=2, io_threads=2, dark=d if dark else None, bits=bits, flat=const)
    assert list(st[0]) == list(st[1]) == [stats["frames"], stats["bytes_in"], stats["bytes_out"], stats["files"]]
    assert files_of(tmp_path / "bits") == files_of(tmp_path / "null") == files_of(tmp_path / "const")


# ---- 7. refusals and state ----------------------------------------------------------------------------------------------------
def test_set_flat_refusals_and_clearing(gpu, tmp_path):
    frames, F, _, pre = clip_case("plain")
    src = source_clip(tmp_path / "card", frames)
    opt = MlvfsOptions(chroma_smooth=2)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(src / NAME)) as r, Flat.from_plane(F, 14, BLACK) as flat:
        with Mount(r, opt, basename="/" + NAME) as m:
            plain = m.dng(0, 2, batch=2)
            with pytest.raises(lib.MlvfsAmdError, match="served"):            # after a frame was served
                m.set_flat(flat)
            assert gpu.mlvfs_amd_mount_set_flat(m.h, None) == lib.ERR_ARG
            assert np.array_equal(m.dng(0, 2, batch=2), plain)
        with Mount(r, opt, basename="/" + NAME, flat=flat) as m:
            m.set_flat(None)                                                 # NULL on a fresh mount: a mount without a flat field
            assert np.array_equal(m.dng(0, 2, batch=2), plain)
        with Mount(r, opt, basename="/" + NAME, flat=flat) as m:
            assert not np.array_equal(m.dng(0, 2, batch=2), plain)
        for shape in ((fc.H, fc.W - 16), (fc.H - 2, fc.W)):
            with Flat.from_plane(np.full(shape, 5000, np.uint16), 14, BLACK) as other:
                with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                    Mount(r, opt, flat=other)
                with Mount(r, opt) as m:
                    assert gpu.mlvfs_amd_mount_set_flat(m.h, other.h) == lib.ERR_ARG
                    assert np.array_equal(m.dng(0, 2, batch=2)[:, 65536:], plain[:, 65536:])     # the mount stays what it was
                for lj92 in (True, False):
                    with pytest.raises(lib.MlvfsAmdError, match="geometry"):
                        r.transcode(str(out / NAME), lj92=lj92, flat=other)
                    assert os.listdir(out) == []
        for bits in (7, 17):
            with pytest.raises(lib.MlvfsAmdError, match="bits per pixel"):
                r.transcode(str(out / NAME), lj92=False, flat=flat, bits=bits)
            assert os.listdir(out) == []


# ---- 7b. a clip whose black level changes in the middle -------------------------------------------------------------------------
@pytest.mark.parametrize("payload", ["plain", "lj92"])
def test_a_batch_ends_where_the_black_level_changes(gpu, tmp_path, payload):
    """64 x 48, five frames; a second RAWI block, stamped just before frame 3, says black 1900 where the first says 2048.  One mount
    call and one transcoder call, each with room for all five frames in a batch: every frame is corrected around ITS black level."""
    w, h, blacks = 64, 48, [2048, 2048, 2048, 1900, 1900]
    frames = dc.clip_frames("plain", 5, w, h)
    F = fc.clip_flat(w, h)
    g = fc.gains(F, BLACK)
    pl, vc = bc.payloads(frames, 14, payload)
    path = str(tmp_path / NAME)
    mlvfile.write_clip(path, pl, w, h, video_class=vc)
    stamps = [int.from_bytes(b[8:16], "little") for tag, b in blocks_of(path) if tag == b"VIDF"]
    late = bytearray(bc.rawi_of(path))
    late[8:16] = (sorted(stamps)[3] - 1).to_bytes(8, "little")
    late[20 + 8 + 20: 20 + 8 + 24] = (1900).to_bytes(4, "little", signed=True)
    open(path, "ab").write(bytes(late))
    pre = [fc.apply(f, g, b, 14) for f, b in zip(frames, blacks)]
    assert not np.array_equal(pre[3], fc.apply(frames[3], g, 2048, 14))
    out = tmp_path / "out"
    out.mkdir()
    gpu.free_focus_pixel_maps()
    with Flat.from_plane(F, 14, BLACK) as flat, mlvfile.MlvReader(path) as r:
        with Mount(r, MlvfsOptions(), basename="/" + NAME, flat=flat) as m:
            files = m.dng(0, 5, batch=8)
        stats = r.transcode(str(out / NAME), lj92=False, batch=8, flat=flat)
    assert stats["frames"] == 5
    nbytes = w * h * 14 // 8
    with mlvfile.MlvReader(str(out / NAME)) as r:
        packed = r.read_frames(0, 5, nbytes)
    for k in range(5):
        got = files[k, 65536:].view("<u2").reshape(h, w)
        assert np.array_equal(got, pre[k]), ("mount", k, int((got != pre[k]).sum()))
        assert packed[k].tobytes() == synth.pack_bits(pre[k], 14).tobytes()[:nbytes], ("transcode", k)


# ---- 8. full size -------------------------------------------------------------------------------------------------------------
def test_full_size_frames(gpu, tmp_path):
    """3584 x 1320, two frames, the 16-pixel forms: flat_apply_dev (with the dark frame in the same pass) against numpy, and the load
    (k_cal_unpack_x16<14, true, true>) through one mount call without options against the same frames."""
    import torch
    w, h = 3584, 1320
    frames, F, plane_d, pre = fc.clip_case("plain", n=2, w=w, h=h, dark=True)
    size, stride = w * h * 2, w * h * 2 + 256
    geom = lib.Geom(w, h, 14, BLACK, 0, 0, 0)
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], w, h)
    with Flat.from_plane(F, 14, BLACK) as flat, Dark.from_plane(plane_d, 14, BLACK) as dark:
        buf = device_buffer(torch, frames, stride)
        lib.check(gpu.mlvfs_amd_flat_apply_dev(flat.h, dark.h, C.byref(geom), C.c_void_p(buf.data_ptr()), stride, 2, None), "flat_apply")
        torch.cuda.synchronize()
        got, rest = split(buf, 2, stride, size)
        assert (rest == PAD).all()
        for k in range(2):
            assert np.array_equal(got[k].view(np.uint16).reshape(h, w), pre[k]), k
        gpu.free_focus_pixel_maps()
        with mlvfile.MlvReader(path) as r, Mount(r, MlvfsOptions(), basename="/B.MLV", dark=dark, flat=flat) as m:
            files = m.dng(0, 2, batch=2)
    for k in range(2):
        g = files[k, 65536:].view(np.uint16).reshape(h, w)
        assert np.array_equal(g, pre[k]), (k, int((g != pre[k]).sum()))
