"""GPU parity of the full dual-ISO conversion (cr2hdr 20-bit, mlvfs/hdr.c:230-1957),
mean23 interpolation, against the oracle (which tests/test_oracle_vs_ref.py pins
byte-exact against the reference's own code).

Stated tolerance: the pattern, white levels and exposure fit are integer /
host-libm work and must be identical; the only device transcendental is the cos() of the per-frame mixing curve,
for which 1 LSB on at most 0.01 % of the pixels is allowed.  MEASURED: every frame comes out bit-identical, and that is
what the tests below require (the tolerance stays documentation); the global decisions (pattern, bright rows, white
levels, exposure fit a / b, ISO difference, darkened white) are compared one by one as well.
"""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import abi, lib, synth

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE


def convert(gpu, f, interp=1, fullres=1, alias=1, cs=0, bad=0, reset=True):
    h, w = f.shape
    if reset:
        gpu.mlvfs_amd_dualiso_reset()
    fh = abi.make_frame_headers(w, h, black=BLACK, white=WHITE)
    out = f.copy()
    r = gpu.cr2hdr20_convert_data(C.byref(fh), lib.ptr(out), interp, fullres, alias, cs, bad)
    return r, out, (fh.rawi_hdr.raw_info.black_level, fh.rawi_hdr.raw_info.white_level)


def check_close(got, want):
    """(name kept from when this was a tolerance: the conversion is bit-identical and has to stay so)"""
    assert np.array_equal(got, want), f"{(got != want).sum()} px differ, max |diff| = {np.abs(got.astype(np.int64) - want.astype(np.int64)).max()}"


def scalars(gpu):
    sc = np.zeros(8, np.float64)
    gpu.mlvfs_amd_dualiso_last_scalars(lib.ptr(sc))
    return sc


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("kind", ["rggb", "gbrg"])
def test_cr2hdr20_global_decisions_equal_the_oracle(gpu, oracle, interp, kind):
    """H3 / H4: pattern, bright rows, white levels, the robust exposure fit and what follows from it -- each on its own, so that
    two errors that cancel in the pixels cannot hide."""
    f = synth.dual_iso_frame(416, 266)[1:265].copy() if kind == "gbrg" else synth.dual_iso_frame(416, 264)
    r0, want, lv0, sc0 = oracle.cr2hdr20(f, BLACK, WHITE, interp, 1, 1, 0, want_scalars=True)
    r1, got, lv1 = convert(gpu, f, interp)
    assert r0 == r1 == 1 and lv0 == lv1
    sc1 = scalars(gpu)
    names = ("rggb", "is_bright", "white", "white_bright", "a", "b", "corr_ev", "white_darkened")
    for n, x, y in zip(names, sc1, sc0):
        assert x == y, (n, x, y)                      # doubles included: same libm, same operation order
    assert sc1[0] == (kind == "rggb") and sc1[4] > 0 and sc1[6] > 0.26
    check_close(got, want)


@pytest.mark.parametrize("fullres,alias", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("w,h", [(64, 48), (136, 72), (416, 264)])
def test_cr2hdr20_mean23(gpu, oracle, w, h, fullres, alias):
    f = synth.dual_iso_frame(w, h)
    r0, want, lv0 = oracle.cr2hdr20(f, BLACK, WHITE, 1, fullres, alias, 0)
    r1, got, lv1 = convert(gpu, f, 1, fullres, alias)
    assert r0 == r1 == 1 and lv0 == lv1 == (BLACK * 4, WHITE * 4)
    check_close(got, want)
    assert (got != f).mean() > 0.9


def test_cr2hdr20_gbrg_and_not_dual_iso(gpu, oracle):
    f = synth.dual_iso_frame(136, 74)[1:73].copy()          # frame that starts on a GB row
    r0, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 1, 1, 1, 0)
    r1, got, _ = convert(gpu, f)
    assert r0 == r1 == 1
    check_close(got, want)
    assert np.array_equal(got[0], f[0])                     # the skipped first row is untouched (hdr.c:1783-1790)
    n = synth.normal_frame(136, 72)
    r, got, lv = convert(gpu, n)
    assert r == 0 and np.array_equal(got, n) and lv == (BLACK, WHITE)


def test_cr2hdr20_amaze_refuses_widths_the_reference_cannot_handle(gpu):
    """w % 4 != 0 leaves part of the reference's green plane unwritten (SSE2 store loop, amaze_demosaic_RT.c:1459):
    no defined result to match, so the frame is reported and left alone."""
    f = synth.dual_iso_frame(66, 48)
    r, got, lv = convert(gpu, f, interp=0)
    assert r == 0 and np.array_equal(got, f) and lv == (BLACK, WHITE)
    assert b"multiple of 4" in gpu.mlvfs_amd_last_error()


def amaze_gpu(gpu, raw):
    import torch
    h, w = raw.shape
    d_raw = torch.from_numpy(raw).cuda()
    out = [torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    rc = gpu.mlvfs_amd_amaze_demosaic_dev(C.c_void_p(d_raw.data_ptr()), w, h, *[C.c_void_p(o.data_ptr()) for o in out], None)
    assert rc == 0, gpu.mlvfs_amd_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("w,h", [(64, 48), (136, 72), (160, 160), (300, 200), (128, 130), (416, 264), (1024, 700)])
def test_amaze_planes_bit_identical(gpu, oracle, w, h):
    """k_amaze.hip against the oracle's restatement of the SSE2 reference: all three float planes, bit for bit.
    Run twice, smaller plane after a larger one, so that stale tile planes of an earlier call would show."""
    for (ww, hh, seed) in ((w, h, 1), (max(w - 28, 36), max(h - 9, 36), 2)):
        raw = synth.amaze_plane(ww, hh, seed)
        for got, want in zip(amaze_gpu(gpu, raw), oracle.amaze_demosaic(raw)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fullres,alias,cs", [(1, 1, 0), (0, 1, 0), (1, 0, 0), (1, 1, 5)])
@pytest.mark.parametrize("w,h", [(64, 48), (136, 72), (416, 264), (640, 400)])
def test_cr2hdr20_amaze_edge(gpu, oracle, w, h, fullres, alias, cs):
    """BASELINE.json config 4 (--amaze-edge), hdr.c:954-1229."""
    f = synth.dual_iso_frame(w, h)
    r0, want, lv0 = oracle.cr2hdr20(f, BLACK, WHITE, 0, fullres, alias, cs)
    r1, got, lv1 = convert(gpu, f, 0, fullres, alias, cs)
    assert r0 == r1 == 1 and lv0 == lv1
    check_close(got, want)


def test_cr2hdr20_amaze_gbrg(gpu, oracle):
    f = synth.dual_iso_frame(136, 74)[1:73].copy()
    r0, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 0, 1, 1, 0)
    r1, got, _ = convert(gpu, f, 0)
    assert r0 == r1 == 1
    check_close(got, want)


def test_cr2hdr20_amaze_full_size(gpu, oracle):
    """BASELINE.json config 4 at 3584x1320."""
    f = synth.dual_iso_frame(3584, 1320)
    r0, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 0, 1, 1, 0)
    r1, got, _ = convert(gpu, f, 0)
    assert r0 == r1 == 1
    check_close(got, want)
    assert np.array_equal(got, want)          # in practice bit-identical; check_close states the tolerance


@pytest.mark.parametrize("fullres", [1, 0])
@pytest.mark.parametrize("cs", [2, 3, 5, 4])
@pytest.mark.parametrize("w,h", [(64, 48), (416, 264)])
def test_cr2hdr20_chroma_smooth(gpu, oracle, w, h, cs, fullres):
    """hdr_chroma_smooth on the 20-bit half-res / full-res planes (hdr.c:1488-1522, 1612-1619); method 4 is the
    reference's "unsupported" branch, which converts without smoothing."""
    f = synth.dual_iso_frame(w, h)
    r0, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 1, fullres, 1, cs)
    r1, got, _ = convert(gpu, f, 1, fullres, 1, cs)
    assert r0 == r1 == 1
    check_close(got, want)


def test_cr2hdr20_sticky_tables(gpu, oracle):
    """The reference keeps the 20-bit tables of the first white level seen per black level
    (hdr.c:1240,1575,1672); a second frame with a different white level reuses them."""
    a, b = synth.dual_iso_frame(136, 72, seed=3), np.minimum(synth.dual_iso_frame(136, 72, seed=4), 12000).astype(np.uint16)
    oracle.L.orc_dualiso_reset()
    gpu.mlvfs_amd_dualiso_reset()
    for f in (a, b):
        _, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 1, 1, 1, 0, reset=False)
        _, got, _ = convert(gpu, f, reset=False)
        check_close(got, want)


def test_cr2hdr20_full_size(gpu, oracle):
    """BASELINE.json config 4 geometry (3584x1320), mean23 interpolation."""
    f = synth.dual_iso_frame(3584, 1320)
    r0, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 1, 1, 1, 0)
    r1, got, _ = convert(gpu, f)
    assert r0 == r1 == 1
    check_close(got, want)


def test_cr2hdr20_device_api(gpu, oracle):
    import torch
    w, h = 416, 264
    f = synth.dual_iso_frame(w, h)
    _, want, _ = oracle.cr2hdr20(f, BLACK, WHITE, 1, 1, 1, 0)
    gpu.mlvfs_amd_dualiso_reset()
    t = torch.from_numpy(f.view(np.int16)).cuda()
    geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
    assert gpu.mlvfs_amd_cr2hdr20_dev(C.byref(geom), C.c_void_p(t.data_ptr()), 1, 1, 1, 0, None) == 1
    torch.cuda.synchronize()
    check_close(t.cpu().numpy().view(np.uint16), want)


# ---------------------------------------------------------------------------------------------- batches
def batch_convert(gpu, frames, interp, fullres=1, alias=1, cs=0, reset=True, pad_rows=3):
    """mlvfs_amd_cr2hdr20_batch_dev on frames of one geometry laid out `stride` bytes apart (with a gap, to catch stride errors)."""
    import torch
    h, w = frames[0].shape
    if reset:
        gpu.mlvfs_amd_dualiso_reset()
    stride = (h + pad_rows) * w * 2
    host = np.full((len(frames), h + pad_rows, w), 0x5A5A, np.uint16)
    for k, f in enumerate(frames):
        host[k, :h] = f
    t = torch.from_numpy(host.view(np.int16)).cuda()
    res = np.full(len(frames), -7, np.int32)
    geom = lib.Geom(w, h, 14, BLACK, WHITE, 0, 0)
    rc = gpu.mlvfs_amd_cr2hdr20_batch_dev(C.byref(geom), C.c_void_p(t.data_ptr()), stride, len(frames), interp, fullres, alias, cs, lib.ptr(res), None)
    assert rc == 0, gpu.mlvfs_amd_last_error()
    torch.cuda.synchronize()
    out = t.cpu().numpy().view(np.uint16)
    assert (out[:, h:] == 0x5A5A).all(), "the batch wrote between the frames"
    return res, [out[k, :h] for k in range(len(frames))]


@pytest.mark.parametrize("interp,cs", [(0, 0), (1, 0), (0, 5), (1, 3)])
def test_cr2hdr20_batch_equals_the_oracle_frame_by_frame(gpu, oracle, interp, cs):
    """One submission for a mixed batch: dual-ISO frames of different content and white levels, one that is not dual ISO, one
    whose pattern starts on a GB row -- results, pixels and the order-dependent table caches (the first frame that converts fixes
    the tables' white level, hdr.c:1240) as if the frames had been converted one after the other."""
    w, h = 416, 264
    frames = [synth.dual_iso_frame(w, h, seed=3), synth.normal_frame(w, h), synth.dual_iso_frame(w, h, seed=5, frame=2),
              np.minimum(synth.dual_iso_frame(w, h, seed=4), 12000).astype(np.uint16),
              synth.dual_iso_frame(w, h + 2, seed=6)[1:h + 1].copy(), synth.dual_iso_frame(w, h, seed=3)]
    oracle.L.orc_dualiso_reset()
    want = [oracle.cr2hdr20(f, BLACK, WHITE, interp, 1, 1, cs, reset=False) for f in frames]
    res, got = batch_convert(gpu, frames, interp, 1, 1, cs)
    assert list(res) == [r for r, _, _ in want] == [1, 0, 1, 1, 1, 1]
    for k, (r, img, _) in enumerate(want):
        assert np.array_equal(got[k], img), f"frame {k}: {(got[k] != img).sum()} px differ"
    assert np.array_equal(got[1], frames[1]) and np.array_equal(got[0], got[5])
    # the same frames one by one through the single-frame entry give the same bytes (a batch of one is the same code)
    gpu.mlvfs_amd_dualiso_reset()
    for k, f in enumerate(frames):
        r1, one, _ = convert(gpu, f, interp, 1, 1, cs, reset=False)
        assert r1 == res[k] and np.array_equal(one, got[k]), k


def test_cr2hdr20_batch_in_parts_equals_the_oracle(gpu, oracle, monkeypatch):
    """A batch that goes out in PARTS (csrc/dualiso.cpp: batches of 8 and more of large frames; here forced with MLVFS_AMD_DI_PART=2
    on nine small ones: parts of 2, 2, 3 and 2 frames -- the last part is smaller than an even share): AMaZE of one part on the
    caller's stream beside interpolation and blend of the part before on a second one.  Frame by frame the oracle's bytes."""
    monkeypatch.setenv("MLVFS_AMD_DI_PART", "2")
    w, h = 416, 264
    frames = [synth.dual_iso_frame(w, h, seed=3), synth.dual_iso_frame(w, h, seed=5, frame=2), synth.normal_frame(w, h),
              np.minimum(synth.dual_iso_frame(w, h, seed=4), 12000).astype(np.uint16), synth.dual_iso_frame(w, h, seed=7),
              synth.dual_iso_frame(w, h + 2, seed=6)[1:h + 1].copy(), synth.dual_iso_frame(w, h, seed=8, frame=1),
              synth.dual_iso_frame(w, h, seed=9), synth.dual_iso_frame(w, h, seed=3)]
    oracle.L.orc_dualiso_reset()
    want = [oracle.cr2hdr20(f, BLACK, WHITE, 0, 1, 1, 0, reset=False) for f in frames]
    res, got = batch_convert(gpu, frames, 0, 1, 1, 0)
    assert list(res) == [r for r, _, _ in want]
    for k, (r, img, _) in enumerate(want):
        assert np.array_equal(got[k], img), f"frame {k}: {(got[k] != img).sum()} px differ"


def test_cr2hdr20_batch_decisions_equal_the_oracle(gpu, oracle):
    """The device-side decisions, scalar by scalar, for the last frame of a batch (mlvfs_amd_dualiso_last_scalars) on frames whose
    white levels, fits and patterns differ."""
    w, h = 416, 264
    for frames in ([synth.dual_iso_frame(w, h, seed=9)], [synth.normal_frame(w, h), synth.dual_iso_frame(w, h + 2, seed=2)[1:h + 1].copy()],
                   [synth.dual_iso_frame(w, h, seed=1), np.minimum(synth.dual_iso_frame(w, h, seed=8), 11000).astype(np.uint16)]):
        oracle.L.orc_dualiso_reset()
        sc0 = None
        for f in frames:
            r0, _, _, sc = oracle.cr2hdr20(f, BLACK, WHITE, 1, 1, 1, 0, want_scalars=True, reset=False)
            if r0 == 1:
                sc0 = sc
        res, _ = batch_convert(gpu, frames, 1)
        sc1 = scalars(gpu)
        for n, x, y in zip(("rggb", "is_bright", "white", "white_bright", "a", "b", "corr_ev", "white_darkened"), sc1, sc0):
            assert x == y, (n, x, y)


def test_cr2hdr20_batch_full_size(gpu):
    """BASELINE.json config 4 at 3584x1320, --amaze-edge: a batch of three against the hashes of the reference's output."""
    import json
    import os
    from conftest import fnv1a
    full = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["full_size"]
    f = synth.dual_iso_frame(3584, 1320)
    res, got = batch_convert(gpu, [f, f, f], 0, 1, 1, 0, pad_rows=0)
    assert list(res) == [1, 1, 1]
    for g in got:
        assert fnv1a(g) == full["dualiso_3584x1320_i0_f1_a1_cs0"]


@pytest.mark.parametrize("interp,cs,key", [(1, 0, "dualiso_3584x1320_i1_f1_a1_cs0"), (0, 5, "dualiso_3584x1320_i0_f1_a1_cs5")])
def test_cr2hdr20_batch_full_size_other_switches(gpu, interp, cs, key):
    """3584x1320 with the reference's default interpolator (mean23) and with --amaze-edge + cs5x5 (the planes then travel as raw
    values through the 20-bit chroma smoothing, not as EV): a batch of two against the hashes of the reference's output."""
    import json
    import os
    from conftest import fnv1a
    full = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["full_size"]
    f = synth.dual_iso_frame(3584, 1320)
    res, got = batch_convert(gpu, [f, f], interp, 1, 1, cs, pad_rows=0)
    assert list(res) == [1, 1]
    for g in got:
        assert fnv1a(g) == full[key]


def test_cr2hdr20_batch_decisions_on_random_material(gpu):
    """tools/dualiso_decision_sweep.py: mixed batches of random material -- ISO ratios 1..16, scenes from deep shadow to mostly
    clipped, noise, black levels 512..2049, any of the four bright-row phases, GBRG-like starts, normal / flat / noise frames that
    are no dual ISO -- through the batch entry point against the checker, results and pixels frame by frame.  (The first run of
    this sweep found what the fixed frames could not: the bright / dark walk takes ONE row phase's count as its total,
    hdr.c:553-555.)  A fixed seed here; the tool takes any."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "dualiso_decision_sweep.py"), "11", "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches" in r.stderr, r.stderr[-3000:]
