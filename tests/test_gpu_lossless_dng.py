"""Losslessly compressed .dng files on the GPU: the batched LJ92 encoder on frames in device memory (csrc/k_lj92enc.hip,
mlvfs_amd_lj92_encode_batch_dev) against the reference's own encoder, byte for byte, and mlvfs_amd_mount_dng_lossless (csrc/mount.cpp)
against the uncompressed files of mlvfs_amd_mount_dng: the header but for two tags, the payload = the reference's encoding of the
uncompressed file's pixels, which its decoder gives back.  No frame of these clips may fall back (flags == 0 for every one; the
CPU-side proof is tests/test_lossless_dng.py); the one frame that must fall back is asserted to do so."""
import numpy as np
import pytest

from mlvfs_amd import lj92, mlvfile
from mlvfs_amd.mount import Mount

from lossless_cases import (BIG_H, BIG_W, H, W, assert_lossless_header, big_frames, fallback_frames, jpeg_view, long_stream_frames, max_class,
                            mount_stream_room)
from mount_harness import NAME, dual_clip, fresh, mount_opts, open_mount, payloads
from test_gpu_ref_host import make_clip
from test_lj92_encode import CASES as SMALL_CASES, material

pytestmark = pytest.mark.gpu

GEOMETRIES = sorted({(w, h) for w, h, _ in SMALL_CASES}) + [(1736, 976), (3584, 1320)]
KINDS = ["smooth", "flat", "noise", "sparse"]


def _device_batch(frames, pad):
    """frames at a device stride larger than a frame: an (n, h, w) view into a padded buffer"""
    import torch
    n = len(frames)
    h, w = frames[0].shape
    per = w * h + pad
    buf = torch.full((n * per,), 0x5A5A, dtype=torch.int16, device="cuda")
    for k, f in enumerate(frames):
        buf[k * per:k * per + w * h] = torch.from_numpy(np.ascontiguousarray(f).view(np.int16).reshape(-1)).cuda()
    return torch.as_strided(buf, (n, h, w), (per, w, 1))


def _expect(oracle, reference, img, bits):
    """the reference's stream, or None where it cannot encode the frame inside its arrays (told by the oracle's restatement, which
    is what keeps such a frame away from the reference's encoder).  The reference also writes past the w * h * 3 + 200 bytes it
    allocates (lj92.c:1120) when a stream is longer -- class 0 with a 16-bit all-ones code, every byte stuffed, is 4 bytes per
    pixel -- so for such a frame the yardstick is the oracle's restatement."""
    h, w = img.shape
    restated = oracle.lj92_encode(img, w, h, bits)
    if restated is None or len(restated) > w * h * 3 + 200:
        return restated
    want = reference.lj92_encode_tile(img, w, h, bits)
    assert want == restated
    return want


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_batch_encoder_equals_the_reference_encoder(gpu, oracle, reference, w, h):
    for n in (1, 3, 8):
        frames = [material(w, h, KINDS[(k + n) % 4], 10 * n + k) for k in range(n)]        # distinct tables inside one batch
        streams, classes, status = lj92.encode_batch(_device_batch(frames, pad={1: 8, 3: 49, 8: 88}[n]), bits=14)   # 16-byte aligned frames and not
        for k, f in enumerate(frames):
            want = _expect(oracle, reference, f, 14)
            assert want is not None and status[k] == 0 and streams[k] == want, (w, h, n, k, status[k], len(streams[k] or b""), len(want or b""))
            assert classes[k] == max_class(want)


@pytest.mark.parametrize("bits", [8, 9, 10, 12, 14, 15, 16])
def test_batch_encoder_bit_depths(gpu, oracle, reference, bits):
    """values of `bits` bits at that SOF3 precision; at 16 bits noise over the whole range has 17-bit differences, which is the next
    test's subject: there the material keeps to 15 bits"""
    vb = min(bits, 15)
    frames = [material(130, 40, KINDS[k % 4], 3 + k, vb) for k in range(5)]
    streams, classes, status = lj92.encode_batch(_device_batch(frames, pad=8), bits=bits)
    for k, f in enumerate(frames):
        want = _expect(oracle, reference, f, bits)
        if want is None:                                    # all 17 classes in use: refused like lj92_encode refuses it
            assert status[k] == lj92.STATUS_TABLE and streams[k] is None, (bits, k)
        else:
            assert status[k] == 0 and streams[k] == want, (bits, k)


def test_batch_encoder_reports_what_the_reference_cannot_encode_and_leaves_the_rest(gpu, oracle, reference):
    w, h = 64, 48
    frames = [material(w, h, KINDS[k % 4], 40 + k) for k in range(6)]
    bad = np.zeros((h, w), np.uint16)                       # 17-bit differences in rows below the first (test_lj92_encode.py)
    bad[:, ::2] = 65535
    bad[1::2] = 65535 - bad[1::2]
    frames[1] = bad
    frames[4] = frames[4].copy()
    frames[4][0, 0] = 0                                     # first difference 0 - 32768: class 16
    streams, classes, status = lj92.encode_batch(_device_batch(frames, pad=40), bits=16)
    assert status[1] == lj92.STATUS_DIFF17 and classes[1] == 17 and streams[1] is None
    assert oracle.lj92_encode(bad, w, h, 16) is None
    assert status[4] == 0 and classes[4] == 16
    assert streams[4] == oracle.lj92_encode(frames[4], w, h, 16)       # the oracle's restatement: valid pixels the mount declines
    for k in (0, 2, 3, 5):
        assert status[k] == 0 and classes[k] < 16 and streams[k] == reference.lj92_encode_tile(frames[k], w, h, 16), k
    # a stream that does not fit its room says so and the others stand
    noise = [material(w, h, "noise", 7), material(w, h, "flat", 8)]
    streams, classes, status = lj92.encode_batch(_device_batch(noise, pad=0), bits=14, out_stride=1024)
    assert status == [lj92.STATUS_NOFIT, 0] and streams[0] is None and streams[1] == reference.lj92_encode_tile(noise[1], w, h, 14)


def test_batch_encoder_takes_host_arrays(gpu, reference):
    frames = [material(96, 40, "smooth", 9), material(96, 40, "sparse", 2)]
    streams, _, status = lj92.encode_batch(frames, bits=14)
    assert status == [0, 0] and streams == [reference.lj92_encode_tile(f, 96, 40, 14) for f in frames]


# ------------------------------------------------------------------ the mount
def _check_files(reference, plain, files, flags, w, h, label=""):
    """every lossless file against the uncompressed one of the same frame; returns the compressed bytes"""
    total = 0
    for k, (p, f) in enumerate(zip(plain, files)):
        assert flags[k] == 0, f"{label} frame {k} fell back"
        px = p[65536:].view(np.uint16).reshape(h, w)
        v = jpeg_view(px)
        want = reference.lj92_encode_tile(v, v.shape[1], v.shape[0], 16)
        assert len(f) == 65536 + len(want), (label, k, len(f), len(want))            # sizes[k]
        assert f[65536:] == want, f"{label} frame {k}: the payload differs from the reference's encoding"
        assert_lossless_header(f[:65536], p[:65536].tobytes(), len(want))
        st, back = reference.lj92_decode(f[65536:])
        assert st == 0 and np.array_equal(back, v), (label, k)
        total += len(f)
    return total


MOUNT_CASES = [
    ("plain", dict(cs=5, badpix=1, stripes=1)),
    ("lzma", dict(cs=5, badpix=1, stripes=1, pnoise=1, deflicker=3000)),
    ("lj92", dict(cs=3, badpix=2, stripes=1, pnoise=1, deflicker=2800)),
    ("plain", dict()),
    ("dual:plain", dict(dual_iso=1, pnoise=1)),
    ("dual:lzma", dict(dual_iso=1, stripes=1, badpix=1)),
    ("dual:lj92", dict(dual_iso=2, hdr_interp=1)),
    ("dual:plain", dict(dual_iso=2, hdr_interp=0, pnoise=1, deflicker=3000)),
]


@pytest.mark.parametrize("kind,opts", MOUNT_CASES, ids=[k + ":" + ",".join(f"{a}={b}" for a, b in o.items()) for k, o in MOUNT_CASES])
def test_mount_lossless_against_uncompressed(gpu, reference, tmp_path, kind, opts):
    d = dual_clip(tmp_path, kind[5:], reference) if kind.startswith("dual:") else make_clip(tmp_path, kind, reference=reference)[0]
    path = str(d / NAME)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        plain = list(m.dng(2, 3, batch=2)) + list(m.dng(0, 2, batch=2))
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        res = np.full(3, -1, np.int32)
        a, fa = m.dng_lossless(2, 3, batch=2, results=res)
        b, fb = m.dng_lossless(0, 2, batch=2)
    assert list(res) == [1 if opts.get("dual_iso") else 0] * 3
    _check_files(reference, plain, a + b, fa + fb, W, H, kind)


def test_mount_lossless_and_plain_calls_interleave_in_serve_order(gpu, tmp_path):
    d, _ = make_clip(tmp_path, "plain", n=8)
    path = str(d / NAME)
    opts = dict(cs=5, badpix=1, stripes=1)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        want = m.dng(0, 8, batch=4)
    fresh(gpu)
    r, m = open_mount(path, opts)
    with r, m:
        files, flags = m.dng_lossless(0, 4, batch=4)
        got = m.dng(4, 4, batch=4)
    assert flags == [0] * 4 and all(len(f) < 65536 + W * H * 2 for f in files)
    assert np.array_equal(got, want[4:])


def test_mount_serves_a_class_16_frame_uncompressed(gpu, reference, tmp_path):
    d = tmp_path / "card"
    d.mkdir()
    frames = fallback_frames(n=5, at=2)
    pl = payloads(frames, "plain")[0]
    mlvfile.write_clip(str(d / NAME), pl, W, H, chunks=2, frame_space=32, shuffle=True)
    path = str(d / NAME)
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        plain = m.dng(0, 5, batch=3)
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        files, flags = m.dng_lossless(0, 5, batch=3)
    assert flags[2] & 1, "the frame whose first pixel is 0 must be served uncompressed"
    assert files[2] == plain[2].tobytes()
    assert np.array_equal(plain[2][65536:].view(np.uint16).reshape(H, W), frames[2])
    rest = [k for k in range(5) if k != 2]
    _check_files(reference, [plain[k] for k in rest], [files[k] for k in rest], [flags[k] for k in rest], W, H, "neighbours")


def test_mount_serves_a_frame_whose_stream_is_longer_than_its_pixels_uncompressed(gpu, oracle, reference, tmp_path):
    """Frame 2's stream is all 0xFF bytes, each stuffed: longer than the frame's pixels with every class below 16
    (tests/test_lossless_dng.py proves it on the CPU).  The refusal it takes is LJE_NOFIT on the device: the oracle's length is beyond
    the stride the mount gives a stream there.  That stride equals the host's cap at this geometry (W * H * 2 is a multiple of 256), so
    no length can pass k_lje_scan_ff and then fail `res.length > cap`; there is no second frame for that refusal."""
    d = tmp_path / "card"
    d.mkdir()
    frames = long_stream_frames(n=5, at=2)
    v = jpeg_view(frames[2])
    cap, stride = mount_stream_room(W, H)
    long = oracle.lj92_encode(v, v.shape[1], v.shape[0], 16)
    assert max_class(long) < 16 and len(long) > stride == cap
    pl = payloads(frames, "plain")[0]
    mlvfile.write_clip(str(d / NAME), pl, W, H, chunks=2, frame_space=32, shuffle=True)
    path = str(d / NAME)
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        plain = m.dng(0, 5, batch=3)
    fresh(gpu)
    r, m = open_mount(path, {})
    with r, m:
        files, flags = m.dng_lossless(0, 5, batch=3)
    assert flags[2] & 1, "a stream longer than the pixels must be served uncompressed"
    assert files[2] == plain[2].tobytes()
    assert np.array_equal(plain[2][65536:].view(np.uint16).reshape(H, W), frames[2])
    rest = [k for k in range(5) if k != 2]
    _check_files(reference, [plain[k] for k in rest], [files[k] for k in rest], [flags[k] for k in rest], W, H, "neighbours")


def test_mount_lossless_full_size_batch(gpu, reference, tmp_path):
    frames = big_frames()
    pl = payloads(frames, "plain")[0]
    path = str(tmp_path / "B.MLV")
    mlvfile.write_clip(path, pl, BIG_W, BIG_H)
    opts = dict(cs=5, stripes=1)
    fresh(gpu)
    with mlvfile.MlvReader(path) as r, Mount(r, mount_opts(opts)[0], basename="/B.MLV") as m:
        plain = m.dng(0, 8, batch=8)
    fresh(gpu)
    with mlvfile.MlvReader(path) as r, Mount(r, mount_opts(opts)[0], basename="/B.MLV") as m:
        files, flags = m.dng_lossless(0, 8, batch=8)
    total = _check_files(reference, list(plain), files, flags, BIG_W, BIG_H, "3584x1320")
    print(f"8 frames of {BIG_W}x{BIG_H}: {total / 8:.0f} bytes per lossless file, {plain.shape[1]} uncompressed "
          f"({total / 8 / plain.shape[1]:.3f})")
