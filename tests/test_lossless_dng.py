"""Losslessly compressed .dng files, the parts that need no GPU: the header variant (csrc/dngheader.cpp), the argument checks of
mlvfs_amd_lj92_encode_batch_dev (csrc/lj92enc.cpp) and mlvfs_amd_mount_dng_lossless (csrc/mount.cpp), which refuse before any
device work, and the CPU-side proof for the GPU tests' "no frame falls back" assertions: on every synthetic clip they serve, the
reference's own encoder (restated by the oracle) never uses difference class 16 on the 2w x h/2 view, and its streams decode back."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import abi, lib, mlvfile, synth

from lossless_cases import (H, LONG_K, W, assert_lossless_header, big_frames, clip_frames, fallback_frames, ifd0, jpeg_view, long_stream_frames,
                            max_class, mount_stream_room)


def _headers(L, k, length, offset=0, max_size=65536):
    fh, fps, base = synth.header_case(k)
    blob = bytes(fh)
    a, b = abi.FrameHeaders.from_buffer_copy(blob), abi.FrameHeaders.from_buffer_copy(blob)
    plain = np.full(max_size + 8, 0xA5, np.uint8)
    got = np.full(max_size + 8, 0xA5, np.uint8)
    n0 = L.dng_get_header_data(C.byref(a), lib.ptr(plain), offset, max_size, float(fps), base)
    n1 = L.mlvfs_amd_dng_header_lossless(C.byref(b), lib.ptr(got), offset, max_size, float(fps), base, length)
    assert n0 == n1 and bytes(a) == bytes(b), "the same return value and the same active-area rewrite"
    assert (got[max_size:] == 0xA5).all(), "wrote past max_size"
    return got[:max_size], plain[:max_size]


def test_lossless_header_differs_from_the_plain_one_in_two_value_fields(amd):
    """camera rows, white-balance modes, geometries and fps overrides of the header test's generated cases; stream lengths from
    tiny to beyond 16 bits"""
    lengths = [1, 66, 65535, 65536, 4812345, 0x7FFFFFF0]
    for i, k in enumerate(range(0, 390, 7)):
        got, plain = _headers(amd, k, lengths[i % len(lengths)])
        assert_lossless_header(got, plain, lengths[i % len(lengths)])


def test_lossless_header_of_converted_levels_and_partial_reads(amd):
    """levels x 4 (what a converted dual-ISO frame gets, hdr.c:223-224) and the partial copies dng_get_header_data allows"""
    fh, fps, base = synth.header_case(11)
    fh.rawi_hdr.raw_info.black_level *= 4
    fh.rawi_hdr.raw_info.white_level *= 4
    blob = bytes(fh)
    a, b = abi.FrameHeaders.from_buffer_copy(blob), abi.FrameHeaders.from_buffer_copy(blob)
    plain, got = np.zeros(65536, np.uint8), np.zeros(65536, np.uint8)
    amd.dng_get_header_data(C.byref(a), lib.ptr(plain), 0, 65536, float(fps), base)
    amd.mlvfs_amd_dng_header_lossless(C.byref(b), lib.ptr(got), 0, 65536, float(fps), base, 123457)
    assert_lossless_header(got, plain, 123457)
    assert ifd0(bytes(got))[50717][2] == fh.rawi_hdr.raw_info.white_level
    full, _ = _headers(amd, 3, 777)
    for offset, size in ((0, 1), (0, 700), (8, 512), (100, 65436)):
        part, _ = _headers(amd, 3, 777, offset, size)
        assert np.array_equal(part, full[offset:offset + size]), (offset, size)


def _err(L):
    return L.mlvfs_amd_last_error().decode()


def test_batch_encoder_refuses_bad_arguments_before_device_work(amd):
    L = amd
    fake, out = C.c_void_p(0x10000), C.c_void_p(0x20000)                  # never dereferenced: every call below is refused first
    n = np.zeros(4, np.uint32)
    st = np.zeros(4, np.int32)
    cl = np.zeros(4, np.int32)
    w, h = 64, 48
    call = lambda *a: L.mlvfs_amd_lj92_encode_batch_dev(*a)
    ok = [fake, w * h * 2, 2, w, h, 14, out, 8192, lib.ptr(n), lib.ptr(st), lib.ptr(cl), None]
    for at in (0, 6, 8, 9):
        bad = list(ok)
        bad[at] = None
        assert call(*bad) == lib.ERR_ARG and "null" in _err(L), at
    assert call(*(ok[:2] + [-1] + ok[3:])) == lib.ERR_ARG and "negative" in _err(L)
    for bits in (0, -3, 17):
        assert call(*(ok[:5] + [bits] + ok[6:])) == lib.ERR_ARG and "bit depth" in _err(L), bits
    for ww, hh in ((0, 48), (64, 0), (-1, 48), (65536, 2), (16384, 16384)):
        assert call(*(ok[:3] + [ww, hh] + ok[5:])) == lib.ERR_ARG and "not supported" in _err(L), (ww, hh)
    for stride in (w * h * 2 - 2, w * h * 2 + 1):
        assert call(*([fake, stride] + ok[2:])) == lib.ERR_ARG and "stride" in _err(L), stride
    for cap in (0, 64, 8190):
        assert call(*(ok[:7] + [cap] + ok[8:])) == lib.ERR_ARG and "out_stride" in _err(L), cap
    assert call(*(ok[:6] + [C.c_void_p(0x20002)] + ok[7:])) == lib.ERR_ARG and "out_stride" in _err(L)
    assert call(*(ok[:2] + [0] + ok[3:])) == lib.OK                          # no frames: nothing to do, nothing touched
    assert not n.any() and not st.any() and not cl.any()


@pytest.fixture()
def clip(tmp_path):
    w, h = 256, 130
    pl = [synth.pack_bits(synth.normal_frame(w, h, frame=k)).tobytes() for k in range(3)]
    names = mlvfile.write_clip(str(tmp_path / "C.MLV"), pl, w, h)
    r = mlvfile.MlvReader(names[0])
    yield r, w, h
    r.close()


def test_mount_dng_lossless_refuses_bad_arguments_before_device_work(amd, clip):
    L = amd
    r, w, h = clip
    o = lib.MountOpts(chroma_smooth=5, fix_stripes=1, rand_mode=1)
    m = L.mlvfs_amd_mount_open(r.h, C.byref(o), b"/C.MLV")
    size = 65536 + w * h * 2
    out = np.zeros((3, size), np.uint8)
    sizes = np.full(3, 77, np.uintp)
    flags = np.full(3, 77, np.int32)
    call = L.mlvfs_amd_mount_dng_lossless
    try:
        assert call(None, 0, 1, lib.ptr(out), size, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert call(m, 0, 1, None, size, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert call(m, 0, 1, lib.ptr(out), size, None, lib.ptr(flags), 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert call(m, 0, 1, lib.ptr(out), size, lib.ptr(sizes), None, 2, 1, None) == lib.ERR_ARG and "null" in _err(L)
        assert call(m, 0, -1, lib.ptr(out), size, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG and "negative" in _err(L)
        for first, count in ((-1, 1), (2, 2), (3, 1), (0, 4)):
            assert call(m, first, count, lib.ptr(out), size, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG, (first, count)
            assert "outside the clip" in _err(L)
        assert call(m, 0, 2, lib.ptr(out), size - 1, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.ERR_ARG and "out_stride" in _err(L)
        assert call(m, 1, 0, lib.ptr(out), size, lib.ptr(sizes), lib.ptr(flags), 2, 1, None) == lib.OK      # nothing to serve
        assert not out.any() and (sizes == 77).all() and (flags == 77).all()
    finally:
        L.mlvfs_amd_mount_close(m)


def test_python_surface_exists():
    from mlvfs_amd import lj92
    from mlvfs_amd.mount import Mount
    assert callable(lj92.encode_batch) and callable(Mount.dng_lossless)


def _round_trip(oracle, reference, img):
    v = jpeg_view(img)
    s = oracle.lj92_encode(v, v.shape[1], v.shape[0], 16)
    assert s is not None
    st, back = reference.lj92_decode(s) if max_class(s) < 16 else (0, v)       # the reference's decoder runs off its array at class 16
    assert st == 0 and np.array_equal(back, v)
    return max_class(s)


def test_no_frame_of_the_gpu_tests_clips_reaches_class_16(oracle, reference):
    """The frames of the clips tests/test_gpu_lossless_dng.py serves, as recorded and -- the dual-ISO ones -- as converted (levels x 4),
    in the 2w x h/2 view at 16 bits: every stream decodes back through the reference's decoder and stays below class 16, so the
    GPU tests' flags == 0 assertions can hold for the reference's encoder alone."""
    worst = 0
    for f in clip_frames("plain", 8) + clip_frames("dual", 5):
        worst = max(worst, _round_trip(oracle, reference, f))
    for k, f in enumerate(clip_frames("dual", 5)):
        r, conv, _ = oracle.hdr_preview(f, synth.BLACK, synth.WHITE)
        assert r == 1
        worst = max(worst, _round_trip(oracle, reference, conv))
    for mode in (0, 1):
        r, conv, _ = oracle.cr2hdr20(clip_frames("dual", 1)[0], synth.BLACK, synth.WHITE, mode, 1, 1, 0, reset=True)
        assert r == 1
        worst = max(worst, _round_trip(oracle, reference, conv))
    for f in big_frames()[:2]:
        worst = max(worst, _round_trip(oracle, reference, f))
    assert worst < 16, worst
    # and the one frame that must fall back does reach it
    frames = fallback_frames()
    classes = [max_class(oracle.lj92_encode(jpeg_view(f), 2 * f.shape[1], f.shape[0] // 2, 16)) for f in frames]
    assert classes[2] == 16 and all(c < 16 for i, c in enumerate(classes) if i != 2), classes


def test_the_long_stream_frame_is_longer_than_its_pixels_below_class_16(oracle, reference):
    """The CPU side of test_mount_serves_a_frame_whose_stream_is_longer_than_its_pixels_uncompressed: frame 2 of long_stream_frames()
    encodes (oracle and reference agree, the reference's decoder gives the view back) to a stream longer than the frame's pixels with
    every class below 16, and longer than the room the mount gives a stream on the device -- so the refusal it takes is LJE_NOFIT
    from k_lje_scan_ff.  At this geometry the pixels' size is a multiple of 256, the device stride equals the host's cap, and no length
    lies between the two: `res.length > cap` (csrc/mount.cpp) cannot be the refusal here."""
    frames = long_stream_frames()
    cap, stride = mount_stream_room(W, H)
    assert cap == stride == W * H * 2
    for k, f in enumerate(frames):
        assert f.shape == (H, W) and int(f.max()) < 16384
        v = jpeg_view(f)
        s = oracle.lj92_encode(v, 2 * W, H // 2, 16)
        assert s is not None and max_class(s) < 16, k
        if k != 2:
            assert len(s) <= cap, k
            continue
        assert (v == v[0]).all()                                        # every row the same staircase
        longest = max(l for l in range(1, 17) if s[19 + l])           # DHT: codes per length; the longest is class 0's, all ones
        assert longest >= LONG_K >= 9
        assert len(s) > 65 + (W * H * longest // 8) * 2 - 4 * W         # 0xFF bytes, each stuffed, behind the first row
        assert len(s) > stride >= cap                                   # NOFIT on the device
        assert len(s) <= 2 * W * (H // 2) * 3 + 200 and reference.lj92_encode_tile(v, 2 * W, H // 2, 16) == s
        st, back = reference.lj92_decode(s)
        assert st == 0 and np.array_equal(back, v)


def test_stream_geometry_sizes(oracle):
    """2w x h/2 against w x h on one frame of each kind, printed (DESIGN.md records the full-size figures).  14-bit values in
    16-bit words: either stream is smaller than the pixels."""
    for f in (clip_frames("plain", 1)[0], clip_frames("dual", 1)[0]):
        h, w = f.shape
        paired = len(oracle.lj92_encode(jpeg_view(f), 2 * w, h // 2, 16))
        rows = len(oracle.lj92_encode(f, w, h, 16))
        print(f"{w}x{h}: 2w x h/2 {paired / (w * h * 2):.3f}, w x h {rows / (w * h * 2):.3f} of the uncompressed size")
        assert paired < w * h * 2 and rows < w * h * 2
