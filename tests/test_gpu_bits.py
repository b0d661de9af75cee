"""A clip rewritten at another bit depth on the GPU (mlvfs_amd_mlv_transcode_bits, mlvfs_amd_repack_dev: csrc/mlvwriter.cpp,
csrc/k_mlvpack.hip): the packed-to-packed kernels against numpy, and whole clips of every payload kind rewritten to
plain and to LJ92 payloads at 12, 10 and 14 bits.

Yardsticks for a rewritten clip: numpy's conversion (bits_cases.convert) packed by synth.pack_bits, or encoded by the reference's own
encoder at the new depth; the RAWI block mlvfile.write_clip writes for a clip of that depth with the shifted levels; and the
reference's own reader + process_frame text (oracle/_ref/ref_host_ref), which must serve the output exactly as it serves the EXPECTED
clip, written from numpy-converted frames.  tests/test_bits_cases.py shows on the CPU that the cases truncate, reach both ends of the
range and hand the reference's encoder only frames it encodes inside the JPEG standard."""
import ctypes as C
import os

import numpy as np
import pytest

from mlvfs_amd import lib, lj92, mlvfile, synth
from mlvfs_amd.dark import Dark
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

import bits_cases as bc
import dark_cases as dc
from bits_cases import NAME
from test_gpu_mlv_transcode import PAD, device_buffer, lj92_payload_check, plain_payload_check, reference_stream, split
from test_gpu_ref_host import need_hosts, run_host, vpath
from test_mlv_transcode import blocks_of, check_container, chunk_names, vidf_fields

pytestmark = pytest.mark.gpu
FULL = dict(cs=5, badpix=1, stripes=1)


# ---- 1. mlvfs_amd_repack_dev against numpy -----------------------------------------------------------------------------------
def words_of(w, h, bpp):
    return (w * h * bpp + 15) // 16


def run_repack(gpu, torch, frames, bpp, out_bpp, dark, want, offset):
    """The packed frames at a padded stride into a PAD-filled buffer, `offset` bytes in; every payload must be pack_bits(want[k]) and
    no other byte may change."""
    h, w = frames[0].shape
    n, win, wout = len(frames), words_of(w, h, bpp), words_of(w, h, out_bpp)
    packed = [np.ascontiguousarray(synth.pack_bits(f, bpp)[:win], "<u2") for f in frames]
    in_stride, out_stride = win * 2 + 36, wout * 2 + 60                      # multiples of 4: the fast form's strides
    src = device_buffer(torch, packed, in_stride)
    dst = torch.full((offset + n * out_stride + 64,), PAD, dtype=torch.uint8, device="cuda")
    geom = lib.Geom(w, h, bpp, 0, 0, 0, 0)
    lib.check(gpu.mlvfs_amd_repack_dev(C.byref(geom), out_bpp, None if dark is None else dark.h, C.c_void_p(src.data_ptr()), in_stride,
                                       C.c_void_p(dst.data_ptr() + offset), out_stride, n, None), "repack")
    torch.cuda.synchronize()
    got, rest = split(dst, n, out_stride, wout * 2, offset)
    assert (rest == PAD).all(), offset                                       # exactly ceil(w * h * out_bpp / 16) words per frame
    for k in range(n):
        g, wanted = got[k].view("<u2"), synth.pack_bits(want[k], out_bpp)[:wout]
        assert np.array_equal(g, wanted), (offset, k, int((g != wanted).sum()))
        if (w * h * out_bpp) % 16:
            assert int(g[-1]) & ((1 << (16 - (w * h * out_bpp) % 16)) - 1) == 0                # the unused low bits
    assert np.array_equal(src.cpu().numpy()[:win * 2].view("<u2"), packed[0])                  # the source is read only


@pytest.mark.parametrize("w,h,bpp,out_bpp,n", bc.REPACK_CASES, ids=lambda v: str(v))
def test_repack_dev_equals_numpy(gpu, w, h, bpp, out_bpp, n):
    """16 x 2, 48 x 6 and 416 x 264 between 14, 12 and 10 bits at offset 0: k_mlv_repack_x16; offset 2, 2 x 2, 30 x 10, 14 -> 16 and
    16 -> 12: the word-per-lane kernel."""
    import torch
    frames = bc.repack_frames(w, h, bpp, n)
    want = [bc.convert(f, bpp, out_bpp) for f in frames]
    for offset in (0, 2):
        run_repack(gpu, torch, frames, bpp, out_bpp, None, want, offset)


@pytest.mark.parametrize("w,h,bpp,out_bpp,n", [(w, h, i, o, n) for (w, h) in bc.REPACK_GEOMETRIES for (i, o) in ((14, 12), (12, 14), (10, 12), (16, 12), (14, 14), (12, 12), (10, 10))
                                               for n in (1, 3)], ids=lambda v: str(v))
def test_repack_dev_with_a_dark_plane_equals_numpy(gpu, w, h, bpp, out_bpp, n):
    """dark_cases.sub_case: both clamps of the subtraction, then the shift; bpp == out_bpp: the subtraction alone"""
    import torch
    black_d = dc.clip_black(bpp) - 37
    frames, dark, sub = dc.sub_case(w, h, bpp, n, black_d)
    want = [bc.convert(s, bpp, out_bpp) for s in sub]
    if bpp == out_bpp:
        assert all(np.array_equal(a, b) for a, b in zip(want, sub))
    with Dark.from_plane(dark, bpp, black_d) as d:
        for offset in (0, 2):
            run_repack(gpu, torch, frames, bpp, out_bpp, d, want, offset)


def test_python_wrapper(gpu):
    import torch
    w, h = 48, 6
    frames = bc.repack_frames(w, h, 14, 3)
    packed = [synth.pack_bits(f, 14)[:words_of(w, h, 14)] for f in frames]
    want = np.stack([synth.pack_bits(bc.convert(f, 14, 10), 10)[:words_of(w, h, 10)] for f in frames])
    got = lj92.repack_frames(packed, w, h, 14, 10)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint16), want)
    wide = torch.full((3, 2, want.shape[1]), 7, dtype=torch.int16, device="cuda")
    lj92.repack_frames(packed, w, h, 14, 10, out=wide[:, 1])
    torch.cuda.synchronize()
    assert np.array_equal(wide[:, 1].cpu().numpy().view(np.uint16), want) and bool((wide[:, 0] == 7).all())
    with pytest.raises(ValueError):
        lj92.repack_frames(packed, w, h, 12, 10)                              # not the words of a 12-bit payload


# ---- 2. whole clips ------------------------------------------------------------------------------------------------------------
_streams = {}


def streams_of(reference, key, frames, bits):
    if key not in _streams:
        _streams[key] = [reference_stream(reference, f, bits) for f in frames]
    return _streams[key]


def source_payload_bytes(first, nchunks=2):
    total = 0
    for name in chunk_names(first, nchunks):
        for tag, b in blocks_of(name):
            if tag == b"VIDF":
                total += len(b) - 32 - vidf_fields(b)[1]
    return total


def transcode(src_dir, out_dir, lj92_out, bits, batch=2, dark=None):
    out_dir.mkdir()
    with mlvfile.MlvReader(str(src_dir / NAME)) as r:
        return r.transcode(str(out_dir / NAME), lj92=lj92_out, batch=batch, io_threads=3, dark=dark, bits=bits)


def check_output(reference, tmp_path, src, out, stats, frames, bpp, out_bpp, lj92_out, key):
    """frames: what the source holds (after the dark frame, if any) at bpp bits.  Against the expected clip: RAWI byte for byte, every
    other block as check_container checks it against a source, payloads against numpy's conversion."""
    conv = [bc.convert(f, bpp, out_bpp) for f in frames]
    want = bc.expected_clip(tmp_path / ("want_" + out.name), frames, bpp, out_bpp)
    payload_of = lj92_payload_check(conv, streams_of(reference, key, conv, out_bpp)) if lj92_out else plain_payload_check(conv, out_bpp)
    seen = check_container(str(want / NAME), str(out / NAME), 2, 0x101 if lj92_out else 1, payload_of)
    assert bc.rawi_of(str(out / NAME)) == bc.rawi_of(str(want / NAME))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=source_payload_bytes(str(src / NAME)), bytes_out=seen[2], files=2)
    assert sorted(os.listdir(out)) == [NAME[:-2] + "00", NAME]


CLIP_CASES = [(kind, lj92_out, 14, out_bpp, batch) for kind in ("plain", "lzma", "lj92") for lj92_out in (False, True)
              for out_bpp, batch in ((12, 2), (10, 8))]
CLIP_CASES += [("plain", False, 12, 14, 8), ("plain", True, 12, 14, 2), ("lj92", True, 12, 14, 8), ("lj92", False, 12, 14, 2)]


@pytest.mark.parametrize("kind,lj92_out,bpp,out_bpp,batch", CLIP_CASES,
                         ids=[f"{k}->{'lj92' if l else 'plain'}:{b}->{o}:batch{n}" for k, l, b, o, n in CLIP_CASES])
def test_clips_at_another_depth(gpu, request, tmp_path, kind, lj92_out, bpp, out_bpp, batch):
    """416 x 264, five frames in two chunks"""
    reference = request.getfixturevalue("reference") if kind == "lzma" or lj92_out else None
    frames = bc.source_frames(bpp)
    src = bc.write_clip(tmp_path / "card", frames, bpp, kind, reference)
    stats = transcode(src, tmp_path / "out", lj92_out, out_bpp, batch)
    check_output(reference, tmp_path, src, tmp_path / "out", stats, frames, bpp, out_bpp, lj92_out, ("clip", bpp, out_bpp))


@pytest.mark.parametrize("kind", ["plain", "lj92"])
@pytest.mark.parametrize("lj92_out", [False, True], ids=["plain", "lj92"])
def test_a_30x12_clip(gpu, request, tmp_path, kind, lj92_out):
    """no multiple of 16 pixels: the generic kernels and one in-place shift"""
    reference = request.getfixturevalue("reference") if lj92_out else None
    frames = bc.small_frames(14)
    src = bc.write_clip(tmp_path / "card", frames, 14, kind)
    stats = transcode(src, tmp_path / "out", lj92_out, 12)
    check_output(reference, tmp_path, src, tmp_path / "out", stats, frames, 14, 12, lj92_out, ("small", 14, 12))


@pytest.mark.parametrize("kind,bpp,out_bpp", bc.SMALL_X8_CLIPS, ids=[f"{k}:{b}->{o}" for k, b, o in bc.SMALL_X8_CLIPS])
def test_a_40x12_clip_to_lj92(gpu, reference, tmp_path, kind, bpp, out_bpp):
    """whole groups of 16 pixels in rows of 8k + 8.  An LJ92 source: the tiling's 8-pixel form with the shift inside, to the right
    (14 -> 12) and to the left (12 -> 14).  A 10-bit plain source: k_mlv_unpack_shift_x16<10>, then the 8-pixel form without a shift.
    (the instantiations no other case selects)"""
    frames = bc.small_frames(bpp, 3, *bc.SMALL_X8)
    src = bc.write_clip(tmp_path / "card", frames, bpp, kind)
    stats = transcode(src, tmp_path / "out", True, out_bpp)
    check_output(reference, tmp_path, src, tmp_path / "out", stats, frames, bpp, out_bpp, True, ("40x12", bpp, out_bpp))


TIES = [("plain", True, 14, 12), ("plain", False, 14, 10), ("lj92", False, 14, 12), ("plain", True, 12, 14)]


@pytest.mark.parametrize("kind,lj92_out,bpp,out_bpp", TIES, ids=[f"{k}->{'lj92' if l else 'plain'}:{b}->{o}" for k, l, b, o in TIES])
def test_the_reference_text_serves_the_output_as_it_serves_the_expected_clip(gpu, tmp_path, kind, lj92_out, bpp, out_bpp):
    need_hosts()
    frames = bc.source_frames(bpp)
    src = bc.write_clip(tmp_path / "card", frames, bpp, kind)
    want_dir = bc.expected_clip(tmp_path / "expected", frames, bpp, out_bpp)
    transcode(src, tmp_path / "out", lj92_out, out_bpp, 8)
    order = [vpath(2), vpath(0), vpath(4), vpath(1), vpath(3), "/" + NAME + "/_PREVIEW.gif"]
    want, _ = run_host("ref", want_dir, tmp_path / "a", FULL, order)
    got, _ = run_host("ref", tmp_path / "out", tmp_path / "b", FULL, order)
    assert got == want


@pytest.mark.parametrize("lj92_out", [False, True], ids=["plain", "lj92"])
def test_the_mount_serves_the_output_as_it_serves_the_expected_clip(gpu, tmp_path, lj92_out):
    frames = bc.source_frames(14)
    src = bc.write_clip(tmp_path / "card", frames, 14)
    want_dir = bc.expected_clip(tmp_path / "expected", frames, 14, 12)
    transcode(src, tmp_path / "out", lj92_out, 12, 8)
    files = []
    for where in (want_dir, tmp_path / "out"):
        gpu.free_focus_pixel_maps()
        with mlvfile.MlvReader(str(where / NAME)) as r, Mount(r, MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1), basename="/" + NAME) as m:
            files.append(m.dng(0, len(frames), batch=4))
    assert files[0].shape == (len(frames), 65536 + bc.W * bc.H * 2) == files[1].shape and np.array_equal(files[0], files[1])


# ---- 3. with a dark frame: convert(subtract(...)) ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,lj92_out", [("plain", False), ("plain", True), ("lzma", False), ("lj92", False), ("lj92", True)],
                         ids=["plain->plain", "plain->lj92", "lzma->plain", "lj92->plain", "lj92->lj92"])
def test_the_dark_frame_is_subtracted_before_the_shift(gpu, request, tmp_path, kind, lj92_out):
    reference = request.getfixturevalue("reference") if kind == "lzma" or lj92_out else None
    frames, plane, pre = bc.dark_case()
    src = bc.write_clip(tmp_path / "card", frames, 14, kind, reference)
    with Dark.from_plane(plane, 14, dc.BLACK) as dark:
        stats = transcode(src, tmp_path / "out", lj92_out, 12, 3, dark)
    assert any(not np.array_equal(bc.convert(p, 14, 12), bc.convert(f, 14, 12)) for p, f in zip(pre, frames))
    check_output(reference, tmp_path, src, tmp_path / "out", stats, pre, 14, 12, lj92_out, ("dark", 14, 12))


@pytest.mark.parametrize("kind", ["plain", "lj92"])
@pytest.mark.parametrize("lj92_out", [False, True], ids=["plain", "lj92"])
def test_a_30x12_clip_with_a_dark_frame(gpu, request, tmp_path, kind, lj92_out):
    """no multiple of 16 pixels, the subtraction in every pixel-per-lane form: inside k_mlv_repack_generic (plain -> plain), behind the
    generic unpack and in front of the in-place shift (plain -> lj92), and in place behind the LJ92 decoder (lj92 -> both)"""
    reference = request.getfixturevalue("reference") if lj92_out else None
    frames, plane, black_d, pre = dc.depth_case(30, 12, 14)
    src = bc.write_clip(tmp_path / "card", frames, 14, kind)
    with Dark.from_plane(plane, 14, black_d) as dark:
        stats = transcode(src, tmp_path / "out", lj92_out, 12, 2, dark)
    assert any(not np.array_equal(bc.convert(p, 14, 12), bc.convert(f, 14, 12)) for p, f in zip(pre, frames))
    check_output(reference, tmp_path, src, tmp_path / "out", stats, pre, 14, 12, lj92_out, ("small dark", 14, 12))


def files_of(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("kind,lj92_out", [("plain", False), ("plain", True), ("lj92", False)], ids=["plain->plain", "plain->lj92", "lj92->plain"])
def test_the_clips_own_depth_is_transcode_dark(gpu, tmp_path, kind, lj92_out):
    frames, plane, _ = bc.dark_case()
    src = bc.write_clip(tmp_path / "card", frames, 14, kind)
    with Dark.from_plane(plane, 14, dc.BLACK) as dark:
        a = transcode(src, tmp_path / "dark", lj92_out, None, 2, dark)
        b = transcode(src, tmp_path / "same", lj92_out, 14, 2, dark)
    c = transcode(src, tmp_path / "plain", lj92_out, None, 2)
    d = transcode(src, tmp_path / "same_plain", lj92_out, 14, 2)
    assert a == b and files_of(tmp_path / "dark") == files_of(tmp_path / "same")
    assert c == d and files_of(tmp_path / "plain") == files_of(tmp_path / "same_plain")
    assert files_of(tmp_path / "plain") != files_of(tmp_path / "dark")


# ---- 4. what cannot be encoded at the new depth ---------------------------------------------------------------------------------
def test_widening_to_16_bits_can_meet_class_16(gpu, tmp_path):
    frames = bc.hot16_frames()
    src = bc.write_clip(tmp_path / "card", frames, 14)
    out = tmp_path / "out"
    out.mkdir()
    L = lib.load()
    with mlvfile.MlvReader(str(src / NAME)) as r:
        st = (C.c_longlong * 4)(-1, -1, -1, -1)
        rc = L.mlvfs_amd_mlv_transcode_bits(r.h, os.fsencode(str(out / NAME)), lib.MLV_LJ92, 16, None, 2, 2, st)
        err = L.mlvfs_amd_last_error().decode()
        assert rc == lib.ERR_ARG and "frame 1 " in err and "class 16" in err and list(st) == [0, 0, 0, 0], err
        assert os.listdir(out) == []
        assert r.transcode(str(out / NAME), lj92=True)["frames"] == 3        # at its own depth the clip encodes
        stats = r.transcode(str(out / "P.MLV"), lj92=False, bits=16)          # and plain payloads at 16 bits have nothing to refuse
    assert stats["frames"] == 3
    conv = [bc.convert(f, 14, 16) for f in frames]
    want = bc.expected_clip(tmp_path / "want", frames, 14, 16, name="P.MLV")
    check_container(str(want / "P.MLV"), str(out / "P.MLV"), 2, 1, plain_payload_check(conv, 16))


# ---- 5. full size ---------------------------------------------------------------------------------------------------------------
def test_full_size_frames(gpu, reference, tmp_path):
    """3584 x 1320, two frames, 14 -> 12 bits, to LJ92"""
    frames = bc.full_size_frames()
    src = bc.write_clip(tmp_path / "card", frames, 14)
    stats = transcode(src, tmp_path / "out", True, 12, 0)
    check_output(reference, tmp_path, src, tmp_path / "out", stats, frames, 14, 12, True, ("full", 14, 12))
