"""mlvfs_amd_mlv_transcode on the GPU (csrc/mlvwriter.cpp, csrc/k_mlvpack.hip): the two kernels against numpy and the checker's
untiling / unpacking, and whole clips rewritten with LJ92 or plain payloads.

Two yardsticks for a rewritten clip: the reference's own encoder gives every stream byte for byte (Reference.lj92_encode_tile of the
quadrant-tiled frame, one component of W x H at the clip's bit depth), and the reference's own reader + process_frame text
(oracle/_ref/ref_host_ref) serves the output exactly as it serves the source.  Every input this file sends to the encoder -- the two
of test_frames_the_encoder_cannot_take aside -- is checked here on the CPU to be one the reference encodes (class_of <= 15).

The 16-bit failure cases: the tiled pattern 0, 0 over 65535, 65535 has no 17-bit difference under lj92.c:754-761 -- its largest is
65535, class 16 --; in a frame of ordinary content it puts all 17 classes in use, which the encoder refuses as the reference would
write behind its tables.  A true 17-bit difference (0, 65535 over 65535, 0: predictor 65535 + (65535 >> 1) against a pixel of 0)
and class 16 alone (a first pixel of 0 in a quiet frame: encoded by the reference, refused by the transcoder's rule) are cases of
their own; bad16_frames works out on the CPU which of the three refusals each frame must meet."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions
from test_gpu_ref_host import H, W, make_clip, need_hosts, run_host, vpath
from test_lj92 import quadrants
from test_mlv_transcode import NAME, check_container, raw_transcode

pytestmark = pytest.mark.gpu
PAD = 0xA5


def classes_of(tiled, bits):
    """The difference classes SSSS the reference's encoder meets in this image (lj92.c:746-764)."""
    t = np.asarray(tiled).astype(np.int64)
    px = np.empty_like(t)
    px[0, 0] = 1 << (bits - 1)
    px[0, 1:] = t[0, :-1]
    px[1:, 0] = t[:-1, 0]
    px[1:, 1:] = t[:-1, 1:] + ((t[1:, :-1] - t[:-1, :-1]) >> 1)
    return {int(d).bit_length() for d in np.unique(np.abs(t - px))}


def class_of(tiled, bits):
    return max(classes_of(tiled, bits))


def reference_stream(reference, frame, bits):
    tiled = quadrants(frame)
    assert class_of(tiled, bits) <= 15                                   # an input the reference encodes inside the JPEG standard
    h, w = frame.shape
    return reference.lj92_encode_tile(tiled, w, h, bits)


def device_buffer(torch, frames, stride, offset=0):
    """The frames `stride` bytes apart from byte `offset` on in a device buffer whose every other byte is PAD."""
    n, size = len(frames), frames[0].nbytes
    host = np.full(offset + n * stride + 64, PAD, np.uint8)
    for k, f in enumerate(frames):
        host[offset + k * stride: offset + k * stride + size] = np.ascontiguousarray(f).view(np.uint8).reshape(-1)
    return torch.from_numpy(host).cuda()


def split(buf, n, stride, size, offset=0):
    """-> (the n payloads of `size` bytes, every byte that belongs to none of them)"""
    host = buf.cpu().numpy()
    rest = np.ones(host.size, bool)
    parts = []
    for k in range(n):
        a = offset + k * stride
        parts.append(host[a:a + size].copy())
        rest[a:a + size] = False
    return parts, host[rest]


TILE_CASES = [(w, h, n, 0) for w, h in ((2, 2), (4, 2), (6, 4), (8, 2), (16, 4), (24, 6), (70, 6), (72, 4), (416, 264)) for n in (1, 3)]
TILE_CASES += [(3584, 1320, 1, 0), (16, 4, 3, 2), (24, 6, 1, 8)]         # one full-size frame; buffers off the fast form's alignment


@pytest.mark.parametrize("w,h,n,offset", TILE_CASES, ids=lambda v: str(v))
def test_quadrant_tiling(gpu, oracle, w, h, n, offset):
    import torch
    rng = np.random.default_rng(w * 131 + h + n)
    frames = [rng.integers(0, 65536, (h, w)).astype(np.uint16) for _ in range(n)]
    size, stride = w * h * 2, w * h * 2 + 512
    src = device_buffer(torch, frames, stride, offset)
    dst = torch.full((offset + n * stride + 64,), PAD, dtype=torch.uint8, device="cuda")
    lib.check(gpu.mlvfs_amd_lj92_tile_dev(C.c_void_p(src.data_ptr() + offset), stride, C.c_void_p(dst.data_ptr() + offset), stride, w, h, n, None), "tile")
    torch.cuda.synchronize()
    got, rest = split(dst, n, stride, size, offset)
    assert (rest == PAD).all()                                          # nothing outside the frames is touched
    for k, f in enumerate(frames):
        tiled = got[k].view(np.uint16).reshape(h, w)
        assert np.array_equal(tiled, quadrants(f)), k
        if w * h <= 416 * 264 or k == 0:
            assert np.array_equal(oracle.lj92_untile(tiled, w, h), f), k
    assert np.array_equal(src.cpu().numpy()[offset:offset + size].view(np.uint16).reshape(h, w), frames[0])


def test_quadrant_tiling_refuses_what_has_no_defined_result(gpu):
    import torch
    a = torch.zeros(1 << 16, dtype=torch.int16, device="cuda")
    b = torch.full((1 << 16,), 7, dtype=torch.int16, device="cuda")
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for w, h in ((3, 2), (2, 3), (5, 5), (417, 264), (416, 263), (0, 2), (2, -2)):
        assert gpu.mlvfs_amd_lj92_tile_dev(pa, 0, pb, 0, w, h, 1, None) == lib.ERR_ARG, (w, h)
    assert gpu.mlvfs_amd_lj92_tile_dev(pa, 0, pa, 0, 16, 4, 1, None) == lib.ERR_ARG          # not in place
    assert gpu.mlvfs_amd_lj92_tile_dev(None, 0, pb, 0, 16, 4, 1, None) == lib.ERR_ARG
    assert gpu.mlvfs_amd_lj92_tile_dev(pa, 64, pb, 256, 16, 4, 2, None) == lib.ERR_ARG        # frames that overlap
    assert gpu.mlvfs_amd_lj92_tile_dev(pa, 0, pb, 0, 16, 4, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((b == 7).all())


PACK_CASES = [(w, h, bpp, n, 0) for bpp in (14, 12, 10) for w, h in ((8, 2), (16, 4), (416, 264)) for n in (1, 3)]
PACK_CASES += [(3584, 1320, 14, 1, 0), (6, 2, 14, 1, 0), (6, 2, 14, 3, 0), (16, 4, 14, 3, 2), (416, 264, 12, 1, 2)]
PACK_CASES += [(10, 6, bpp, n, 0) for bpp in (1, 7, 8, 9, 11, 13, 15, 16) for n in (1, 3)]


@pytest.mark.parametrize("w,h,bpp,n,offset", PACK_CASES, ids=lambda v: str(v))
def test_bit_packing(gpu, oracle, w, h, bpp, n, offset):
    """Every frame holds values above bpp bits: the kernel masks them, a stray bit would land in the neighbouring pixel."""
    import torch
    rng = np.random.default_rng(w * 17 + h * 3 + bpp + n)
    frames = [rng.integers(0, 65536, (h, w)).astype(np.uint16) for _ in range(n)]
    frames[0][0, 0] = frames[0][-1, -1] = 0xFFFF
    mask = (1 << bpp) - 1
    words = (w * h * bpp + 15) // 16
    stride, pstride = w * h * 2 + 512, words * 2 + 64
    src = device_buffer(torch, frames, stride)
    dst = torch.full((offset + n * pstride + 64,), PAD, dtype=torch.uint8, device="cuda")
    geom = lib.Geom(w, h, bpp, 0, 0, 0, 0)
    lib.check(gpu.mlvfs_amd_pack_dev(C.byref(geom), C.c_void_p(src.data_ptr()), stride, C.c_void_p(dst.data_ptr() + offset), pstride, n, None), "pack")
    torch.cuda.synchronize()
    got, rest = split(dst, n, pstride, words * 2, offset)
    assert (rest == PAD).all()                                          # exactly ceil(w * h * bpp / 16) words per frame
    for k, f in enumerate(frames):
        want = synth.pack_bits(f & mask, bpp)[:words]
        assert np.array_equal(got[k].view("<u2"), want), k
        if (w * h * bpp) % 16:
            assert int(got[k].view("<u2")[-1]) & ((1 << (16 - (w * h * bpp) % 16)) - 1) == 0          # the unused low bits
        if w * h <= 416 * 264:
            back = oracle.unpack(np.concatenate([got[k].view("<u2"), np.zeros(8, "<u2")]), w, h, bpp)
            assert np.array_equal(back.reshape(h, w), f & mask), k


def test_bit_packing_refusals(gpu):
    import torch
    a = torch.zeros(4096, dtype=torch.int16, device="cuda")
    b = torch.full((4096,), 7, dtype=torch.int16, device="cuda")
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for w, h, bpp in ((16, 4, 0), (16, 4, 17), (0, 4, 14), (16, -1, 14)):
        assert gpu.mlvfs_amd_pack_dev(C.byref(lib.Geom(w, h, bpp, 0, 0, 0, 0)), pa, 0, pb, 0, 1, None) == lib.ERR_ARG, (w, h, bpp)
    g = lib.Geom(16, 4, 14, 0, 0, 0, 0)
    assert gpu.mlvfs_amd_pack_dev(None, pa, 0, pb, 0, 1, None) == lib.ERR_ARG
    assert gpu.mlvfs_amd_pack_dev(C.byref(g), pa, 128, pb, 64, 2, None) == lib.ERR_ARG        # packed frames that overlap
    torch.cuda.synchronize()
    assert bool((b == 7).all())


def test_python_wrappers(gpu, oracle):
    """mlvfs_amd.lj92.tile_frames / pack_frames: host arrays (uploaded), device tensors with a padded frame stride, a caller's `out`,
    and the `out` they refuse."""
    import torch
    from mlvfs_amd import lj92
    w, h, bpp = 24, 6, 12
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 65536, (h, w)).astype(np.uint16) for _ in range(3)]
    words = (w * h * bpp + 15) // 16
    want_tiled = np.stack([quadrants(f) for f in frames])
    want_packed = np.stack([synth.pack_bits(f & 0xFFF, bpp)[:words] for f in frames])
    tiled = lj92.tile_frames(frames)                                      # host arrays
    assert tiled.shape == (3, h, w) and np.array_equal(tiled.cpu().numpy().view(np.uint16), want_tiled)
    packed = lj92.pack_frames(frames, bpp)
    assert packed.shape == (3, words) and np.array_equal(packed.cpu().numpy().view(np.uint16), want_packed)
    # device frames two frame sizes apart, into every other row of the caller's buffers
    wide = torch.zeros((3, 2, h, w), dtype=torch.int16, device="cuda")
    wide[:, 0] = torch.from_numpy(np.stack(frames).view(np.int16)).cuda()
    out_t = torch.full((3, 2, h, w), 7, dtype=torch.int16, device="cuda")
    out_p = torch.full((3, 2, words), 7, dtype=torch.int16, device="cuda")
    assert lj92.tile_frames(wide[:, 0], out=out_t[:, 1]).data_ptr() == out_t[:, 1].data_ptr()
    lj92.pack_frames(wide[:, 0], bpp, out=out_p[:, 1])
    torch.cuda.synchronize()
    assert np.array_equal(out_t[:, 1].cpu().numpy().view(np.uint16), want_tiled) and bool((out_t[:, 0] == 7).all())
    assert np.array_equal(out_p[:, 1].cpu().numpy().view(np.uint16), want_packed) and bool((out_p[:, 0] == 7).all())
    for k in range(3):
        assert np.array_equal(oracle.lj92_untile(want_tiled[k], w, h), frames[k])
    for bad in (torch.zeros((3, h, w + 2), dtype=torch.int16, device="cuda"), torch.zeros((3, h, w), dtype=torch.int32, device="cuda"),
                torch.zeros((3, h, w), dtype=torch.int16), torch.zeros((3, h, 2 * w), dtype=torch.int16, device="cuda")[:, :, ::2],
                np.zeros((3, h, w), np.uint16)):
        with pytest.raises(ValueError):
            lj92.tile_frames(wide[:, 0], out=bad)
    for bad in (torch.zeros((3, words + 1), dtype=torch.int16, device="cuda"), torch.zeros((3, 2 * words), dtype=torch.int16, device="cuda")[:, ::2]):
        with pytest.raises(ValueError):
            lj92.pack_frames(wide[:, 0], bpp, out=bad)
    with pytest.raises(ValueError):
        lj92.tile_frames(torch.zeros((3, h, 2 * w), dtype=torch.int16, device="cuda")[:, :, ::2])     # frames that are not contiguous


# ---- whole clips -------------------------------------------------------------------------------------------------------
_streams = {}


def clip_streams(reference, frames, bits=14, key="416x264"):
    if key not in _streams:
        _streams[key] = [reference_stream(reference, f, bits) for f in frames]
    return _streams[key]


def transcode(src_dir, out_dir, lj92, batch=0, name=NAME):
    out_dir.mkdir()
    with mlvfile.MlvReader(str(src_dir / name)) as r:
        return r.transcode(str(out_dir / name), lj92=lj92, batch=batch, io_threads=3)


def lj92_payload_check(frames, streams):
    h, w = frames[0].shape

    def payload_of(k, p):
        assert p[:4] == struct.pack("<I", w * h * 2), k
        assert p[4:] == streams[k], (k, len(p) - 4, len(streams[k]))     # the reference encoder's stream and nothing behind it
    return payload_of


def plain_payload_check(frames, bpp=14):
    h, w = frames[0].shape
    nbytes = (w * h * bpp + 7) // 8

    def payload_of(k, p):
        assert len(p) == (nbytes + 1) // 2 * 2 and p[:nbytes] == synth.pack_bits(frames[k], bpp).tobytes()[:nbytes], k
    return payload_of


@pytest.mark.parametrize("kind,batch", [("plain", 2), ("plain", 8), ("lzma", 3), ("lj92", 8)])
def test_lj92_output_is_the_reference_encoders(gpu, reference, tmp_path, kind, batch):
    d, frames = make_clip(tmp_path, kind, reference=reference)
    stats = transcode(d, tmp_path / "out", True, batch)
    seen = check_container(str(d / NAME), str(tmp_path / "out" / NAME), 2, 0x101, lj92_payload_check(frames, clip_streams(reference, frames)))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)
    assert sorted(os.listdir(tmp_path / "out")) == [NAME[:-2] + "00", NAME]


def test_plain_output_of_an_lj92_clip(gpu, reference, tmp_path):
    d, frames = make_clip(tmp_path, "lj92")
    stats = transcode(d, tmp_path / "out", False, 2)
    seen = check_container(str(d / NAME), str(tmp_path / "out" / NAME), 2, 1, plain_payload_check(frames))
    assert seen[0] == len(frames) and stats == dict(frames=seen[0], bytes_in=seen[1], bytes_out=seen[2], files=2)


def test_the_reference_text_serves_the_lj92_output_as_it_serves_the_source(gpu, tmp_path):
    need_hosts()
    d, _ = make_clip(tmp_path, "plain")
    transcode(d, tmp_path / "out", True, 8)
    order = [vpath(2), vpath(0), vpath(4), vpath(1), vpath(3), "/" + NAME + "/_PREVIEW.gif"]
    opts = dict(cs=5, badpix=1, stripes=1)
    want, _ = run_host("ref", d, tmp_path / "src", opts, order)
    got, _ = run_host("ref", tmp_path / "out", tmp_path / "dst", opts, order)
    assert got == want


def test_the_mount_serves_the_lj92_output_as_it_serves_the_source(gpu, tmp_path):
    d, frames = make_clip(tmp_path, "plain")
    transcode(d, tmp_path / "out", True, 8)
    files = []
    for where in (d, tmp_path / "out"):
        with mlvfile.MlvReader(str(where / NAME)) as r, Mount(r, MlvfsOptions(chroma_smooth=2), basename="/" + NAME) as m:
            files.append(m.dng(0, len(frames), batch=4))
    assert files[0].shape == (len(frames), 65536 + W * H * 2) == files[1].shape and np.array_equal(files[0], files[1])


def other_clip(tmp_path, frames, bpp):
    d = tmp_path / "card"
    d.mkdir()
    h, w = frames[0].shape
    pl = [np.ascontiguousarray(synth.pack_bits(f, bpp), "<u2").tobytes() for f in frames]
    mlvfile.write_clip(str(d / NAME), pl, w, h, bpp=bpp, chunks=2, frame_space=16, shuffle=True)
    return d


ROUND_TRIPS = {
    "14": lambda w, h, k: (synth.normal_frame(w, h, seed=6, frame=k), 14),
    "12": lambda w, h, k: (synth.normal_frame(w, h, seed=6, frame=k) >> 2, 12),
    "10": lambda w, h, k: (synth.normal_frame(w, h, seed=6, frame=k) >> 4, 10),
    "dual_iso": lambda w, h, k: (synth.dual_iso_frame(w, h, frame=k), 14),
    "adversarial": lambda w, h, k: (synth.adversarial_frame(w, h, frame=k), 14),
}


@pytest.mark.parametrize("what", sorted(ROUND_TRIPS))
def test_round_trip_plain_lj92_plain(gpu, reference, tmp_path, what):
    """136x72: a width the 8-pixel form of the tiling takes; three frames in two chunks, batches of two."""
    w, h = 136, 72
    made = [ROUND_TRIPS[what](w, h, k) for k in range(3)]
    frames, bpp = [np.ascontiguousarray(f, np.uint16) for f, _ in made], made[0][1]
    d = other_clip(tmp_path, frames, bpp)
    transcode(d, tmp_path / "lj", True, 2)
    streams = [reference_stream(reference, f, bpp) for f in frames]
    check_container(str(d / NAME), str(tmp_path / "lj" / NAME), 2, 0x101, lj92_payload_check(frames, streams))
    transcode(tmp_path / "lj", tmp_path / "back", False, 2)
    check_container(str(d / NAME), str(tmp_path / "back" / NAME), 2, 1, plain_payload_check(frames, bpp))


def test_full_size_frames(gpu, reference, tmp_path):
    need_hosts()
    d, frames = make_clip(tmp_path, "plain", n=2, w=3584, h=1320)
    transcode(d, tmp_path / "out", True)
    check_container(str(d / NAME), str(tmp_path / "out" / NAME), 2, 0x101,
                    lj92_payload_check(frames, clip_streams(reference, frames, key="3584x1320")))
    want, _ = run_host("ref", d, tmp_path / "src", {}, [vpath(0), vpath(1)])
    got, _ = run_host("ref", tmp_path / "out", tmp_path / "dst", {}, [vpath(0), vpath(1)])
    assert got == want


def bad16_frames(oracle, what, w=64, h=48):
    """Three 16-bit frames; the middle one is made so that the call must fail -> (frames, the words its error must hold)."""
    shift = 4 if what == "first_pixel_0" else 0                          # a quiet frame: few classes in use
    frames = [np.ascontiguousarray(synth.normal_frame(w, h, seed=2, frame=k) >> shift, np.uint16) for k in range(3)]
    tiled = quadrants(frames[1])
    if what == "diff17":
        tiled[:2, :2] = [[0, 65535], [65535, 0]]                          # predictor 65535 + (65535 >> 1), pixel 0
    elif what == "rows_0_65535":
        tiled[:2, :2] = [[0, 0], [65535, 65535]]
    else:
        tiled[0, 0] = 0                                                   # against the first predictor 32768: -32768
    used = classes_of(tiled, 16)
    # what lj92.c does with it: a 17-bit difference is counted behind hist[]; 17 classes in use write an 18th code behind the
    # tables; class 16 alone is encoded, with 16 value bits the JPEG standard does not have
    why = "17 bits" if max(used) == 17 else "17 difference classes" if len(used) == 17 else "class 16"
    assert max(used) == (17 if what == "diff17" else 16)
    assert why == {"diff17": "17 bits", "first_pixel_0": "class 16"}.get(what, why)
    assert (oracle.lj92_encode(tiled, w, h, 16) is None) == (why != "class 16")
    frames[1] = oracle.lj92_untile(tiled, w, h)
    assert np.array_equal(quadrants(frames[1]), tiled)
    assert class_of(quadrants(frames[0]), 16) <= 15 and class_of(quadrants(frames[2]), 16) <= 15
    return frames, why


@pytest.mark.parametrize("what", ["diff17", "rows_0_65535", "first_pixel_0"])
def test_frames_the_encoder_cannot_take(gpu, oracle, tmp_path, what):
    frames, why = bad16_frames(oracle, what)
    d = other_clip(tmp_path, frames, 16)
    out = tmp_path / "out"
    out.mkdir()
    with mlvfile.MlvReader(str(d / NAME)) as r:
        rc, stats, err = raw_transcode(r.h, str(out / NAME), lib.MLV_LJ92, batch=2)
        assert rc == lib.ERR_ARG and "frame 1 " in err and why in err and stats == [0, 0, 0, 0], err
        assert os.listdir(out) == []
        # the same clip as plain payloads: nothing to refuse
        assert r.transcode(str(out / NAME), lj92=False)["frames"] == 3
    check_container(str(d / NAME), str(out / NAME), 2, 1, plain_payload_check(frames, 16))
