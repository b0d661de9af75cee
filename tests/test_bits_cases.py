"""A clip at another bit depth, the part that needs no GPU (csrc/mlvwriter.cpp): the three symbols,
mlvfs_amd_rawi_set_bits against the rule, out_bpp = 0 (and the clip's own depth) as the plain transcode it must be, the refusals --
and that the cases of tests/bits_cases.py, which tests/test_gpu_bits.py runs on the GPU, really test something: a conversion that
rounded, dithered, saturated or did nothing would be caught, and every frame handed to the reference's encoder there is one it
encodes inside the JPEG standard."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth

import bits_cases as bc
from test_gpu_mlv_transcode import class_of, classes_of
from test_lj92 import quadrants
from test_mlv_transcode import blocks_of, chunk_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mlvfs_amd_rawi_set_bits", "mlvfs_amd_repack_dev", "mlvfs_amd_mlv_transcode_bits"]
DEPTHS = (14, 12, 10, 16)


def test_the_three_symbols_are_declared_and_exported(amd):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlvfs_amd.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in lib.DEVICE_SYMBOLS and hasattr(amd, name), name
        assert getattr(amd, name).argtypes, name


def small_clip(d, bpp, n=3, w=64, h=48):
    frames = bc.source_frames(bpp, n, w, h)
    return bc.write_clip(d, frames, bpp), frames


@pytest.mark.parametrize("bpp", DEPTHS)
@pytest.mark.parametrize("out_bpp", DEPTHS)
def test_rawi_set_bits_writes_the_expected_clips_block(amd, tmp_path, bpp, out_bpp):
    src, frames = small_clip(tmp_path / "src", bpp)
    want = bc.rawi_of(str(bc.expected_clip(tmp_path / "want", frames, bpp, out_bpp) / bc.NAME))
    block = bc.rawi_of(str(src / bc.NAME))
    buf = C.create_string_buffer(block, len(block))
    assert amd.mlvfs_amd_rawi_set_bits(buf, out_bpp) == 0, amd.mlvfs_amd_last_error()
    assert buf.raw == want
    if bpp != out_bpp:
        assert block != want
    # the rule itself, field by field (struct raw_info behind the 16-byte prefix and xRes, yRes)
    h, w, pitch, frame_size, bits, black, white = np.frombuffer(buf.raw, "<i4", 7, 20 + 8)
    xres, yres = np.frombuffer(buf.raw, "<u2", 2, 16)
    b0, w0 = bc.levels(bpp)
    assert (bits, black, white) == (out_bpp, bc.shift(b0, out_bpp - bpp), bc.shift(w0, out_bpp - bpp))
    assert pitch == w * out_bpp // 8 and frame_size == int(xres) * int(yres) * out_bpp // 8
    if out_bpp < bpp <= 14:                                                                     # (a 16-bit source's levels are multiples of 4)
        assert black << (bpp - out_bpp) != b0 and white << (bpp - out_bpp) != w0                # both levels truncate


def test_rawi_set_bits_refusals_leave_the_block_untouched(amd, tmp_path):
    src, _ = small_clip(tmp_path / "src", 14)
    block = bc.rawi_of(str(src / bc.NAME))
    assert amd.mlvfs_amd_rawi_set_bits(None, 12) == lib.ERR_ARG
    for out_bpp in (7, 17, 0, -12):
        buf = C.create_string_buffer(block, len(block))
        assert amd.mlvfs_amd_rawi_set_bits(buf, out_bpp) == lib.ERR_ARG and buf.raw == block, out_bpp
    for bad in (0, 17, -14):
        damaged = bytearray(block)
        damaged[20 + 8 + 16: 20 + 8 + 20] = int(bad).to_bytes(4, "little", signed=True)         # raw_info.bits_per_pixel
        buf = C.create_string_buffer(bytes(damaged), len(damaged))
        assert amd.mlvfs_amd_rawi_set_bits(buf, 12) == lib.ERR_ARG and buf.raw == bytes(damaged), bad


def raw_transcode_bits(reader, out_path, payload, out_bpp, batch=0):
    L = lib.load()
    st = (C.c_longlong * 4)(-1, -1, -1, -1)
    rc = L.mlvfs_amd_mlv_transcode_bits(reader, os.fsencode(out_path), payload, out_bpp, None, batch, 2, st)
    return rc, list(st), L.mlvfs_amd_last_error().decode()


def files_of(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("kind", ["plain", "lzma"])
def test_out_bpp_0_and_the_clips_own_depth_are_the_plain_transcode_without_a_device(request, tmp_path, kind):
    reference = request.getfixturevalue("reference") if kind == "lzma" else None
    frames = bc.source_frames(14, 5, 64, 48)
    src = bc.write_clip(tmp_path / "src", frames, 14, kind, reference)
    for d in ("plain", "zero", "same"):
        (tmp_path / d).mkdir()
    with mlvfile.MlvReader(str(src / bc.NAME)) as r:
        want = r.transcode(str(tmp_path / "plain" / bc.NAME), lj92=False, batch=2)
        for d, out_bpp in (("zero", 0), ("same", 14)):
            rc, stats, err = raw_transcode_bits(r.h, str(tmp_path / d / bc.NAME), lib.MLV_PLAIN, out_bpp, batch=2)
            assert rc == 0, err
            assert stats == [want["frames"], want["bytes_in"], want["bytes_out"], want["files"]]
        assert r.transcode(str(tmp_path / "zero" / "B.MLV"), lj92=False, batch=2, bits=0) == want     # the Python face: mlvfs_amd_mlv_transcode
    plain = files_of(tmp_path / "plain")
    assert len(plain) == 2 and files_of(tmp_path / "same") == plain
    zero = files_of(tmp_path / "zero")
    assert {n: zero[n] for n in plain} == plain and [zero["B.MLV"], zero["B.M00"]] == [plain[bc.NAME], plain[bc.NAME[:-2] + "00"]]


def test_depths_outside_8_to_16_are_refused_and_leave_nothing(tmp_path):
    src, _ = small_clip(tmp_path / "src", 14)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(src / bc.NAME)) as r:
        for out_bpp in (7, 17, 1, -1, 32):
            for payload in (lib.MLV_PLAIN, lib.MLV_LJ92):
                rc, stats, err = raw_transcode_bits(r.h, str(out / bc.NAME), payload, out_bpp)
                assert rc == lib.ERR_ARG and "bits per pixel" in err and stats == [0, 0, 0, 0], (out_bpp, err)
                assert os.listdir(out) == []
        with pytest.raises(lib.MlvfsAmdError):
            r.transcode(str(out / bc.NAME), lj92=False, bits=7)
    assert os.listdir(out) == []


def test_repack_dev_checks_its_arguments_before_any_device_work(amd):
    """No HIP device is needed for a refusal; the pointers are never followed."""
    a, b = np.zeros(4096, np.uint16), np.full(4096, 7, np.uint16)
    pa, pb = lib.ptr(a), lib.ptr(b)
    rp = amd.mlvfs_amd_repack_dev
    g = C.byref(lib.Geom(16, 4, 14, 0, 0, 0, 0))
    for w, h, bpp, out_bpp in ((16, 4, 0, 12), (16, 4, 17, 12), (16, 4, 14, 7), (16, 4, 14, 17), (16, 4, 14, 0), (0, 4, 14, 12), (16, -1, 14, 12),
                               (1 << 14, 1 << 13, 14, 12)):
        assert rp(C.byref(lib.Geom(w, h, bpp, 0, 0, 0, 0)), out_bpp, None, pa, 0, pb, 0, 1, None) == lib.ERR_ARG, (w, h, bpp, out_bpp)
    assert rp(None, 12, None, pa, 0, pb, 0, 1, None) == lib.ERR_ARG and rp(g, 12, None, None, 0, pb, 0, 1, None) == lib.ERR_ARG
    assert rp(g, 12, None, pa, 0, None, 0, 1, None) == lib.ERR_ARG and rp(g, 12, None, pa, 0, pa, 0, 1, None) == lib.ERR_ARG
    # 16 x 4: 112 bytes at 14 bits, 96 at 12
    assert rp(g, 12, None, pa, 110, pb, 96, 2, None) == lib.ERR_ARG and rp(g, 12, None, pa, 112, pb, 94, 2, None) == lib.ERR_ARG
    assert rp(g, 12, None, pa, 113, pb, 96, 2, None) == lib.ERR_ARG
    assert rp(g, 12, None, C.c_void_p(a.ctypes.data + 1), 0, pb, 0, 1, None) == lib.ERR_ARG
    assert rp(g, 12, None, pa, 112, pb, 96, -1, None) == lib.ERR_ARG and rp(g, 12, None, pa, 112, pb, 96, 0, None) == 0
    from mlvfs_amd.dark import Dark
    with Dark.from_plane(np.full((4, 16), 512, np.uint16), 12, 512) as other:                 # a dark frame of another depth
        assert rp(g, 12, other.h, pa, 112, pb, 96, 1, None) == lib.ERR_ARG and b"dark" in amd.mlvfs_amd_last_error()
    assert not a.any() and (b == 7).all()


# ---- the cases are non-vacuous ------------------------------------------------------------------------------------------------
def dropped(frames, bpp, out_bpp):
    low = np.concatenate([f.reshape(-1) for f in frames]).astype(np.int64) & ((1 << (bpp - out_bpp)) - 1)
    return low


def assert_narrowing_material(frames, bpp, out_bpp, what):
    allpx = np.concatenate([f.reshape(-1) for f in frames])
    low, half = dropped(frames, bpp, out_bpp), 1 << (bpp - out_bpp - 1)
    assert int(allpx.max()) == (1 << bpp) - 1 and int(allpx.min()) == 0, what
    assert (low != 0).any() and (low >= half).any() and (low < half).any(), what
    for f in frames:
        conv = bc.convert(f, bpp, out_bpp)
        assert int(conv.max()) == (1 << out_bpp) - 1 and int(conv.min()) == 0, what
        rounded = np.minimum((f.astype(np.int64) + half) >> (bpp - out_bpp), (1 << out_bpp) - 1)
        assert (rounded != conv).any(), what                                # rounding would give another frame
        assert np.array_equal(conv.astype(np.int64) << (bpp - out_bpp), f.astype(np.int64) - (f.astype(np.int64) & ((1 << (bpp - out_bpp)) - 1))), what


@pytest.mark.parametrize("bpp,out_bpp", [c for c in bc.CLIP_DEPTHS if c[1] < c[0]])
def test_the_clip_cases_truncate_and_change_what_is_served(oracle, bpp, out_bpp):
    frames = bc.source_frames(bpp)
    assert_narrowing_material(frames, bpp, out_bpp, "clip")
    assert_narrowing_material(bc.small_frames(bpp), bpp, out_bpp, "30x12")
    (b0, _), (b1, _) = bc.levels(bpp), bc.out_levels(bpp, out_bpp)
    for f in frames[:2]:
        src5, out5 = oracle.chroma_smooth(f, b0, 5), oracle.chroma_smooth(bc.convert(f, bpp, out_bpp), b1, 5)
        assert not np.array_equal(out5, src5)
        assert not np.array_equal(out5, bc.convert(src5, bpp, out_bpp))     # nor is it the source's cs5x5 shifted: the stages see new pixels


def test_the_dark_case_truncates():
    _, _, pre = bc.dark_case()
    for out_bpp in (12, 10):
        low, half = dropped(pre, 14, out_bpp), 1 << (14 - out_bpp - 1)
        allpx = np.concatenate([p.reshape(-1) for p in pre])
        assert int(allpx.max()) == 16383 and int(allpx.min()) == 0                            # both clamps of the subtraction
        assert (low != 0).any() and (low >= half).any()


@pytest.mark.parametrize("w,h,bpp,out_bpp,n", [c for c in bc.REPACK_CASES if c[3] < c[2]], ids=lambda v: str(v))
def test_the_repack_cases_truncate(w, h, bpp, out_bpp, n):
    frames = bc.repack_frames(w, h, bpp, n)
    allpx = np.concatenate([f.reshape(-1) for f in frames])
    low, half = dropped(frames, bpp, out_bpp), 1 << (bpp - out_bpp - 1)
    assert int(allpx.max()) == (1 << bpp) - 1 and int(allpx.min()) == 0
    assert (low != 0).any() and (low >= half).any()


def test_widening_cases_use_the_whole_range():
    for bpp, out_bpp in [c for c in bc.CLIP_DEPTHS if c[1] > c[0]]:
        for f in bc.source_frames(bpp):
            conv = bc.convert(f, bpp, out_bpp)
            assert int(f.max()) == (1 << bpp) - 1 and int(conv.max()) == ((1 << bpp) - 1) << (out_bpp - bpp) and int(conv.min()) == 0


@pytest.mark.parametrize("kind,bpp,out_bpp", bc.SMALL_X8_CLIPS, ids=[f"{k}:{b}->{o}" for k, b, o in bc.SMALL_X8_CLIPS])
def test_the_40x12_cases_truncate_or_use_the_whole_range_and_encode(kind, bpp, out_bpp):
    """what the 416 x 264 and 30 x 12 material shows above, for the 40 x 12 frames"""
    frames = bc.small_frames(bpp, 3, *bc.SMALL_X8)
    assert frames[0].shape == (12, 40)
    if out_bpp < bpp:
        assert_narrowing_material(frames, bpp, out_bpp, "40x12")
    for f in frames:
        conv = bc.convert(f, bpp, out_bpp)
        assert int(f.max()) == (1 << bpp) - 1 and int(f.min()) == 0
        assert int(conv.max()) == bc.shift((1 << bpp) - 1, out_bpp - bpp) and int(conv.min()) == 0
        assert class_of(quadrants(conv), out_bpp) <= 15                     # the reference's encoder gets this frame


# ---- what the GPU file hands to the reference's encoder -----------------------------------------------------------------------
def test_every_frame_handed_to_the_reference_encoder_is_one_it_encodes():
    for bpp, out_bpp in bc.CLIP_DEPTHS:
        for f in bc.source_frames(bpp) + bc.small_frames(bpp):
            assert class_of(quadrants(bc.convert(f, bpp, out_bpp)), out_bpp) <= 15, (bpp, out_bpp)
    for p in bc.dark_case()[2]:
        assert class_of(quadrants(bc.convert(p, 14, 12)), 12) <= 15
    for f in bc.full_size_frames():
        assert class_of(quadrants(bc.convert(f, 14, 12)), 12) <= 15


def test_the_16_bit_case_meets_class_16_and_nothing_else():
    frames = bc.hot16_frames()
    for k, f in enumerate(frames):
        assert class_of(quadrants(f), 14) <= 15, k                            # the source encodes at its own depth
        used = classes_of(quadrants(bc.convert(f, 14, 16)), 16)
        assert max(used) == (16 if k == 1 else max(used)) and (k == 1 or max(used) <= 15), (k, used)
        assert len(used) < 17, (k, used)                                      # not the encoder's other refusal (17 classes in use)


def test_sources_other_blocks_are_the_expected_clips(tmp_path):
    """check_container against the EXPECTED clip checks an output's blocks against the source's: RAWI aside, the two clips' blocks
    outside VIDF are the same bytes."""
    frames = bc.source_frames(14, 5, 64, 48)
    src = bc.write_clip(tmp_path / "src", frames, 14)
    want = bc.expected_clip(tmp_path / "want", frames, 14, 12)
    seen = 0
    for a, b in zip(chunk_names(str(src / bc.NAME), 2), chunk_names(str(want / bc.NAME), 2)):
        ba, bb = blocks_of(a), blocks_of(b)
        assert [t for t, _ in ba] == [t for t, _ in bb]
        for (tag, x), (_, y) in zip(ba, bb):
            if tag == b"RAWI":
                assert x != y
                seen += 1
            elif tag == b"VIDF":
                assert x[8:32] == y[8:32]                                     # timestamp, number, crop, pan, frameSpace
            else:
                assert x == y, tag
    assert seen == 1


def late_rawi(block, bits, black):
    """a copy of a RAWI block with another depth and black level, stamped behind every frame of the clip"""
    b = bytearray(block)
    b[8:16] = (10 ** 9).to_bytes(8, "little")
    b[20 + 8 + 16: 20 + 8 + 20] = int(bits).to_bytes(4, "little", signed=True)
    b[20 + 8 + 20: 20 + 8 + 24] = int(black).to_bytes(4, "little", signed=True)
    return bytes(b)


def test_every_rawi_block_is_rewritten_from_its_own_content(amd, tmp_path):
    """A second RAWI block, at 12 bits, at the end of the second chunk of a 14-bit clip: at out_bpp = 14 the frames keep their depth
    (the host-only route: no device here), the first RAWI block is copied, and the late one comes out at 14 bits by the rule."""
    src, _ = small_clip(tmp_path / "src", 14, n=4)
    names = chunk_names(str(src / bc.NAME), 2)
    first = bc.rawi_of(names[0])
    late = late_rawi(first, 12, 511)
    open(names[1], "ab").write(late)
    (tmp_path / "out").mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        rc, stats, err = raw_transcode_bits(r.h, str(tmp_path / "out" / bc.NAME), lib.MLV_PLAIN, 14, batch=2)
    assert rc == 0 and stats[0] == 4, err
    out = chunk_names(str(tmp_path / "out" / bc.NAME), 2)
    assert bc.rawi_of(out[0]) == first
    tag, got = blocks_of(out[1])[-1]
    want = C.create_string_buffer(late, len(late))
    assert amd.mlvfs_amd_rawi_set_bits(want, 14) == 0
    assert tag == b"RAWI" and got == want.raw and got != late
    bits, black = np.frombuffer(got, "<i4", 2, 20 + 8 + 16)
    assert (bits, black) == (14, 511 << 2)


def test_a_rawi_block_without_a_usable_depth_fails_the_call_and_leaves_nothing(tmp_path):
    src, _ = small_clip(tmp_path / "src", 14, n=4)
    names = chunk_names(str(src / bc.NAME), 2)
    open(names[1], "ab").write(late_rawi(bc.rawi_of(names[0]), 0, 0))
    (tmp_path / "out").mkdir()
    with mlvfile.MlvReader(names[0]) as r:
        rc, stats, err = raw_transcode_bits(r.h, str(tmp_path / "out" / bc.NAME), lib.MLV_PLAIN, 14)
        assert rc == lib.ERR_ARG and "RAWI" in err and stats == [0, 0, 0, 0], err
        assert os.listdir(tmp_path / "out") == []
        rc, _, err = raw_transcode_bits(r.h, str(tmp_path / "out" / bc.NAME), lib.MLV_PLAIN, 0)      # without a conversion the block is copied
        assert rc == 0, err
