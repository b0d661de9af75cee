"""The batched stages that existed only per frame (pattern noise, deflicker, dual-ISO preview) and the mount that chains every stage
of process_frame (mlvfs/main.c:908-1005) over batches of a clip's frames and hands out whole .dng files (csrc/mount.cpp)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mlvfs_amd import lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

from mount_harness import H, NAME, W, dual_clip, fresh, open_mount
from test_gpu_ref_host import OPTION_SETS, make_clip, need_hosts, run_host, vpath

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE


def _dev_frames(frames, pad=512):
    """frames -> one device buffer, frame k at k * stride bytes (stride = frame + pad); returns (tensor, stride)"""
    import torch
    h, w = frames[0].shape
    stride = w * h * 2 + pad
    buf = np.zeros(len(frames) * stride, np.uint8)
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + w * h * 2] = np.ascontiguousarray(f, np.uint16).view(np.uint8).reshape(-1)
    return torch.from_numpy(buf).cuda(), stride


def _host_frames(d, stride, n, w, h):
    b = d.cpu().numpy()
    return [b[k * stride:k * stride + w * h * 2].view(np.uint16).reshape(h, w).copy() for k in range(n)]


def _golden():
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["full_size"]


# ------------------------------------------------------------------ pattern noise
@pytest.mark.parametrize("w,h", [(256, 130), (416, 264), (96, 1200), (1920, 1080)])
def test_batched_pattern_noise_equals_the_oracle(gpu, oracle, w, h):
    for n in ((1, 3) if w == 1920 else (1, 3, 8)):
        frames = [synth.normal_frame(w, h, seed=11 + k, frame=k) for k in range(n)]
        d, stride = _dev_frames(frames)
        geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
        lib.check(gpu.mlvfs_amd_fix_pattern_noise_dev(C.byref(geom), C.c_void_p(d.data_ptr()), stride, n, None), "fix_pattern_noise_dev")
        got = _host_frames(d, stride, n, w, h)
        tail = d.cpu().numpy()
        for k in range(n):
            want = oracle.fix_pattern_noise(frames[k], WHITE)
            assert np.array_equal(got[k], want), f"{w}x{h} frame {k}/{n}: {(got[k] != want).sum()} px differ"
            assert (tail[k * stride + w * h * 2:(k + 1) * stride] == 0).all(), "wrote into the padding"


def _pn_frame_bytes(w, h):
    """pattern_noise_batch_frame_bytes (csrc/k_pnoise.hip): the scratch one frame of a sub-batch takes"""
    up = lambda b: (b + 255) // 256 * 256
    n = w * h
    return up(n * 2) * 2 + up(n * 4) + up((2 * max(w, h) + 8) * 4) + 256


@pytest.mark.parametrize("fit", [1, 3, 7])
def test_batched_pattern_noise_in_sub_batches_equals_the_oracle(gpu, oracle, fit):
    """A batch larger than the scratch: 8 frames where `fit` fit go as even sub-batches (8 x 1, 3 + 3 + 2, 4 + 4)."""
    w, h, n = 416, 264, 8
    frames = [synth.normal_frame(w, h, seed=31 + k, frame=k) for k in range(n)]
    d, stride = _dev_frames(frames)
    geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
    gpu.mlvfs_amd_test_pn_scratch_cap(fit * _pn_frame_bytes(w, h))
    try:
        lib.check(gpu.mlvfs_amd_fix_pattern_noise_dev(C.byref(geom), C.c_void_p(d.data_ptr()), stride, n, None), "fix_pattern_noise_dev")
    finally:
        gpu.mlvfs_amd_test_pn_scratch_cap(0)
    for k, g in enumerate(_host_frames(d, stride, n, w, h)):
        want = oracle.fix_pattern_noise(frames[k], WHITE)
        assert np.array_equal(g, want), f"fit {fit}, frame {k}: {(g != want).sum()} px differ"


def test_batched_pattern_noise_full_size_hashes(gpu):
    """3 and 8 copies of the 3584x1320 frame (8 do not fit the default scratch: two sub-batches of 4), 2 of the 1920x1080 one."""
    from conftest import fnv1a
    meta = _golden()
    for (w, h, n, key) in ((3584, 1320, 3, "B_3584x1320_pattern_noise"), (3584, 1320, 8, "B_3584x1320_pattern_noise"),
                           (1920, 1080, 2, "A_1920x1080_pattern_noise")):
        f = synth.normal_frame(w, h, seed=1)
        d, stride = _dev_frames([f] * n)
        geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
        lib.check(gpu.mlvfs_amd_fix_pattern_noise_dev(C.byref(geom), C.c_void_p(d.data_ptr()), stride, n, None), "fix_pattern_noise_dev")
        for k, g in enumerate(_host_frames(d, stride, n, w, h)):
            assert fnv1a(g) == meta[key], (key, k)


# ------------------------------------------------------------------ deflicker
def _deflicker_counts(f, bpp):
    """main.c:897-899 on the host: the 32-bit counts of every second pixel from pixel 1, and the medians with the reference's
    16-bit counters (histogram.c:57,63-76) and without the fold"""
    flat = f.reshape(-1)
    size = (flat.size * 2 - 1) // 2
    white = (1 << bpp) + 1
    c = np.bincount(np.minimum(flat[1:][:size][::2], white), minlength=white + 1).astype(np.int64)
    mid = (size // 2) // 2
    a16, a32 = np.cumsum(c & 0xFFFF) > mid, np.cumsum(c) > mid
    return c, (int(np.argmax(a16)) if a16.any() else 0), (int(np.argmax(a32)) if a32.any() else 0)


def _wrapping_frames():
    """3584x1320 frames whose 16-bit counters wrap: a flat grey band (the fold moves the median) and a clipped sky (it does not)"""
    a = synth.normal_frame(3584, 1320, seed=5, frame=0)
    a[:400, :] = 3000
    b = synth.normal_frame(3584, 1320, seed=6, frame=1)
    b[:300, :] = WHITE
    return [a, b]


@pytest.mark.parametrize("bpp", [14, 12, 10])
def test_batched_deflicker_equals_the_per_frame_path_and_the_reference_rule(gpu, reference, bpp):
    sizes = [(416, 264)] * 3 + ([(3584, 1320)] * 2 if bpp == 14 else [])
    for (w, h) in sorted(set(sizes)):
        n = sizes.count((w, h))
        shift = 14 - bpp
        black = BLACK >> shift
        frames = [(synth.normal_frame(w, h, seed=5 + k, frame=k) >> shift).astype(np.uint16) for k in range(n)]
        if w == 3584:
            frames = _wrapping_frames()
            counts = [_deflicker_counts(f, bpp) for f in frames]
            assert all(c.max() > 65535 for c, _, _ in counts), "the 16-bit counters must wrap in these frames"
            assert counts[0][1] != counts[0][2], "the fold must move the median of the grey-band frame"
        d, stride = _dev_frames(frames)
        geom = lib.Geom(w, h, bpp, black, WHITE >> shift, 0, 0)
        size_bytes = w * h * 2
        for target in (3072 >> shift, 5000 >> shift):
            eb = np.zeros(2 * n, np.int32)
            lib.check(gpu.mlvfs_amd_deflicker_batch_dev(C.byref(geom), C.c_void_p(d.data_ptr()), stride, n, size_bytes, target, lib.ptr(eb), None))
            for k in range(n):
                one = np.zeros(2, np.int32)
                lib.check(gpu.mlvfs_amd_deflicker_dev(C.byref(geom), C.c_void_p(d.data_ptr() + k * stride), size_bytes, target, lib.ptr(one), None))
                assert tuple(eb[2 * k:2 * k + 2]) == tuple(one), (bpp, w, k, target)
                flat = np.ascontiguousarray(frames[k].reshape(-1))
                median = int(reference.L.ref_hist_median_of(np.ascontiguousarray(flat[1:]), (size_bytes - 1) // 2, 1, (1 << bpp) + 1))
                with np.errstate(divide="ignore"):
                    corr = np.log2(np.float64(target - black) / np.float64(median - black)) * 10000
                assert (int(eb[2 * k]), int(eb[2 * k + 1])) == (int(np.trunc(corr)), 10000), (bpp, w, k, target, median)
                if w == 3584:
                    assert median == counts[k][1], (k, median, counts[k])


# ------------------------------------------------------------------ dual-ISO preview
def test_batched_preview_equals_hdr_convert_data_frame_by_frame(gpu, oracle):
    """pixels and results per frame; the batched call reports no levels (the x4 levels reach the DNG headers the mount tests
    compare byte for byte)"""
    w, h = 416, 264
    frames = [synth.normal_frame(w, h, seed=7) if k in (1, 4) else synth.dual_iso_frame(w, h, seed=3 + k, frame=k) for k in range(6)]
    d, stride = _dev_frames(frames)
    geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
    res = np.full(len(frames), -7, np.int32)
    lib.check(gpu.mlvfs_amd_hdr_preview_batch_dev(C.byref(geom), C.c_void_p(d.data_ptr()), stride, len(frames), w * h * 2, lib.ptr(res), None))
    got = _host_frames(d, stride, len(frames), w, h)
    for k, f in enumerate(frames):
        r, want, lv = oracle.hdr_preview(f, BLACK, WHITE)
        assert int(res[k]) == r == (0 if k in (1, 4) else 1), k
        assert np.array_equal(got[k], want), f"frame {k}: {(got[k] != want).sum()} px differ"


# ------------------------------------------------------------------ the mount against the reference's process_frame text
ORDER = [2, 3, 4, 0, 1]


def serve(gpu, d, opts):
    """frames 2..4, then 0..1, in batches of 2, through one fresh mount; [(data, header)] in the order 2, 3, 4, 0, 1"""
    fresh(gpu)
    r, m = open_mount(str(d / NAME), opts)
    with r, m:
        files = np.concatenate([m.dng(2, 3, batch=2), m.dng(0, 2, batch=2)])
    return [(f[65536:].tobytes(), f[:65536].tobytes()) for f in files]


def compare(host, want, got):
    assert len(want) == len(got)
    for (wd, wh), (gd, gh), k in zip(want, got, ORDER):
        assert len(gd) == len(wd), (host, k)
        if gd != wd:
            a, b = np.frombuffer(gd, np.uint8), np.frombuffer(wd, np.uint8)
            raise AssertionError(f"frame {k}: the pixels differ from {host}'s in {(a != b).sum()} bytes")
        assert gh == wh, f"frame {k}: the header differs from {host}'s in {(np.frombuffer(gh, np.uint8) != np.frombuffer(wh, np.uint8)).sum()} bytes"


CASES = [(k, None, o) for k, o in OPTION_SETS] + [
    ("plain", None, dict(cs=5, badpix=1, stripes=1, pnoise=1)),
    ("lzma", None, dict(cs=3, pnoise=1, deflicker=2800, stripes=1)),
    ("lj92", None, dict(cs=5, badpix=2, stripes=1, pnoise=1, deflicker=3000)),
    ("plain", None, dict(cs=5, fps1000=23976)),
    ("dual:plain", (), dict(pnoise=1, dual_iso=1)),
    ("dual:lzma", (), dict(pnoise=1, dual_iso=1, stripes=1)),
    ("dual:lj92", (), dict(pnoise=1, dual_iso=1, badpix=1)),
    ("dual:plain", (), dict(pnoise=1, deflicker=3000, dual_iso=2, hdr_interp=0)),
    ("dual:lzma", (), dict(pnoise=1, deflicker=3000, dual_iso=2, hdr_interp=1)),
    ("dual:lj92", (), dict(pnoise=1, deflicker=3000, dual_iso=2, hdr_interp=0)),
    ("dual:lj92", (), dict(pnoise=1, deflicker=3000, dual_iso=2, hdr_interp=1)),
    ("dual:plain", (3,), dict(dual_iso=2, hdr_interp=1, badpix=1, stripes=1)),
    ("dual:lzma", (0,), dict(dual_iso=2, hdr_interp=0, badpix=1, stripes=1, cs=2)),
    ("dual:plain", (4,), dict(dual_iso=1, badpix=1, stripes=1, deflicker=2500)),
]


@pytest.mark.parametrize("kind,normal_at,opts", CASES, ids=[k + ":" + ",".join(f"{a}={b}" for a, b in o.items()) for k, _, o in CASES])
def test_mount_serves_the_reference_dng_files(gpu, reference, tmp_path, kind, normal_at, opts):
    need_hosts()
    if kind.startswith("dual:"):
        d = dual_clip(tmp_path, kind[5:], reference, normal_at)
    else:
        d, _ = make_clip(tmp_path, kind, reference=reference)
    want, _ = run_host("ref", d, tmp_path / "ref", opts, [vpath(k) for k in ORDER])
    got = serve(gpu, d, opts)
    compare("the reference", want, got)


def test_mount_preview_with_chroma_smoothing_equals_the_library_dropin_sequence(gpu, reference, tmp_path):
    """dual_iso = 1 with chroma smoothing reads past the reference's raw2ev table (main.c:154-179): no defined result; the mount gives
    what the library's own drop-in symbols give under the reference's process_frame text."""
    need_hosts()
    opts = dict(dual_iso=1, cs=5, stripes=1)
    d = dual_clip(tmp_path, "plain", normal_at=(1,))
    want, _ = run_host("amd", d, tmp_path / "amd", opts, [vpath(k) for k in ORDER])
    compare("the drop-in sequence", want, serve(gpu, d, opts))


def test_mount_results_and_sizes(gpu, tmp_path):
    d, _ = make_clip(tmp_path, "dual_iso")
    gpu.mlvfs_amd_dualiso_reset()
    with mlvfile.MlvReader(str(d / "M07-1234.MLV")) as r, Mount(r, MlvfsOptions(dual_iso=2, hdr_interpolation_method=1)) as m:
        res = np.full(5, -1, np.int32)
        files = m.dng(0, 5, batch=3, results=res)
        assert files.shape == (5, 65536 + W * H * 2) and m.dng_size() == files.shape[1]
        assert list(res) == [1] * 5
        assert m.dng(4, 0).shape[0] == 0
