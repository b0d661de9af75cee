"""Every task shape of the streaming kernels against the oracle: k_frame_p5 (cs5x5) and k_frame_s (cs2x2 / cs3x3) over the geometry
list of tests/stream_shapes.py, which reaches every class of the cut of a frame into tasks (tests/test_stream_shapes.py) -- last columns
of 1, 13 .. 16, 29 .. 31 and 62 items, every fold with both input layouts, every number of parts in the last folded task, last segments
of one row, two rows and a full task, one to several folded tasks and columns --, with tasks of 30 and of 60 rows, on every footage
kind, and the headline geometry 3584x1320 in the long launches the benchmark measures.

Everything is bit-exact against the `oracle` fixture.  After every launch the plan that launch took is read back from the library
(mlvfs_amd_test_last_frame_plan): a launch that dropped to another kernel than the case is there for fails, although every kernel
gives the oracle's bytes.  And what k_frame_p5 leaves to the list-mode k_frame is counted (mlvfs_amd_test_stream_listed): k_frame does
those tiles again, so on footage k_frame_p5 can settle it must have listed next to nothing (check_listed)."""
import numpy as np
import pytest

import stream_shapes as S
from mlvfs_amd import synth
from stream_shapes import P_NONE, P_P5, P_S, P_TILES
from test_gpu_stream import BLACK, make_stream, oracle_clip

pytestmark = pytest.mark.gpu

POISON = 0x5A5A
geom_ids = lambda g: f"{g[0]}x{g[1]}"


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


def where(diff, w, h, seg_rows):
    """Where the pixels of a frame that differ lie: columns, segments and, in a folded column, parts of the cut"""
    ys, xs = np.nonzero(diff)
    if not len(ys):
        return "no pixel differs"
    cols, segs, fold, _ = S.stream_plan(w, h, seg_rows) if seg_rows else (0, 0, 1, 0)
    msg = f"{len(ys)} px differ, x {xs.min()}..{xs.max()}, y {ys.min()}..{ys.max()}"
    if seg_rows:
        at = sorted({(int(x) // (8 * S.col_items()), int(y) // (2 * seg_rows)) for x, y in zip(xs[:100000], ys[:100000])})
        msg += f"; (column, segment) of {cols} x {segs}, fold {fold}: {at[:24]}"
    return msg


def check_frames(got, want, w, h, seg_rows, what):
    """numpy frames against the oracle's"""
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), f"{what} frame {k}: {where(got[k] != want[k], w, h, seg_rows)}"


def check_on_device(torch, out, want, w, h, seg_rows, what):
    """Every frame of a launch whose input repeats len(want) distinct frames, compared on the device"""
    exp = torch.from_numpy(np.stack(want).view(np.int16)).to(out.device)
    n = len(want)
    bad = torch.zeros(out.shape[0], dtype=torch.bool, device=out.device)
    for k in range(n):
        bad[k::n] = (out[k::n] != exp[k]).flatten(1).any(1)
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        diff = (out[i] != exp[i % n]).cpu().numpy()
        raise AssertionError(f"{what}: {int(bad.sum())} of {out.shape[0]} frames differ, the first is frame {i}: {where(diff, w, h, seg_rows)}")


def check_listed(listed, w, h, nf, judged, what):
    """What k_frame_p5 left to the list-mode k_frame: k_frame does every listed tile again, so the bytes alone cannot tell a k_frame_p5
    that is right from one that lists everything.  Where `judged` -- the benchmark's footage kind, and no pixel map dense enough to
    send whole regions to the list (the synthetic frames carry 128 defects whatever their size: on the small geometries more than
    the 64 records a wave holds in most regions, on 3584x1320 a record or two per region) -- a long launch stays below the share at
    which the library's own policy would take its stream away from k_frame_p5 (stream_shapes.CALM_PERCENT).  The other footage
    kinds are uncertain, dark or full of pixel-map records on purpose: reported only."""
    tiles = S.launch_tiles(w, h, nf)
    print(f"{w}x{h} {what}: {listed} of {tiles} tiles listed ({100.0 * listed / tiles:.2f} %)")
    if judged:
        assert listed * 100 <= tiles * S.CALM_PERCENT, f"{what}: k_frame_p5 listed {listed} of {tiles} tiles"


def repeat(torch, base, nf):
    """nf frames: the rows of `base` over and over"""
    return base[torch.arange(nf, device=base.device) % base.shape[0]].contiguous()


# ------------------------------------------------------------------ the sweep: short launches (k_frame_p5 in 30-row tasks, k_frame_s in 60-row tasks)
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("w,h", S.GEOMETRIES, ids=[geom_ids(g) for g in S.GEOMETRIES])
def test_sweep_k_frame_p5(torch_cuda, oracle, w, h, kind, monkeypatch):
    """cs5x5 on three frames of every geometry and footage kind, with a pixel map of either detection mode and stripes, and with
    neither: forced through k_frame_p5 (tasks of 30 rows: a forced short launch), then the same input through k_frame_p + list and
    through k_frame alone.  Each launch took the kernel it is there for, cut as the hook cuts the frame."""
    from mlvfs_amd.stream import to_numpy_u16
    frames = S.footage(kind, w, h, 3)
    for bad, stripes in ((1, 1), (0, 0), (2, 0)):
        want, pixels, _ = oracle_clip(oracle, frames, w, h, 5, bad, stripes)
        s = make_stream(w, h)
        packed = s.upload_packed([synth.pack_bits(f) for f in frames])
        s.analyse_first_frame(packed, cs=5, bad_pix=bad, stripes=bool(stripes), rand_mode=1)
        if bad:
            assert np.array_equal(s.get_pixel_map(), pixels)
        out = s.alloc_out(3)
        for p, p5, first in (("2", "2", P_P5), ("2", "0", P_TILES), ("0", "1", P_NONE)):
            monkeypatch.setenv("MLVFS_AMD_KF_P", p)
            monkeypatch.setenv("MLVFS_AMD_KF_P5", p5)
            what = f"{kind} bad {bad} stripes {stripes} first kernel {first}"
            out.fill_(POISON)
            before = S.listed_tiles()
            s.process(packed, out, cs=5, fix_pixels=bool(bad), stripes=bool(stripes))
            S.assert_took(first, w, h, 30, what)
            check_frames(to_numpy_u16(out), want, w, h, 30, what)
            if first == P_P5:                        # (three frames, a few dozen tiles: reported, not judged)
                print(f"{w}x{h} {what}: {S.listed_tiles() - before} of {S.launch_tiles(w, h, 3)} tiles listed")
        s.close()


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("w,h", S.GEOMETRIES, ids=[geom_ids(g) for g in S.GEOMETRIES])
def test_sweep_k_frame_s(torch_cuda, oracle, w, h, kind, monkeypatch):
    """cs2x2 and cs3x3 with and without stripes on three frames of every geometry and footage kind: forced through k_frame_s (tasks of 60
    rows, always), then through k_frame alone."""
    from mlvfs_amd.stream import to_numpy_u16
    frames = S.footage(kind, w, h, 3)
    for cs in (2, 3):
        for stripes in (1, 0):
            want, _, _ = oracle_clip(oracle, frames, w, h, cs, 0, stripes)
            s = make_stream(w, h)
            packed = s.upload_packed([synth.pack_bits(f) for f in frames])
            s.analyse_first_frame(packed, cs=cs, bad_pix=0, stripes=bool(stripes), rand_mode=1)
            out = s.alloc_out(3)
            for mode, first in (("2", P_S), ("0", P_NONE)):
                monkeypatch.setenv("MLVFS_AMD_KF_S", mode)
                what = f"{kind} cs {cs} stripes {stripes} first kernel {first}"
                out.fill_(POISON)
                s.process(packed, out, cs=cs, fix_pixels=False, stripes=bool(stripes))
                S.assert_took(first, w, h, 60, what)
                check_frames(to_numpy_u16(out), want, w, h, 60, what)
            s.close()


# ------------------------------------------------------------------ k_frame_p5 in 60-row tasks: long launches of small frames
def cu_count(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("kind", ["normal", "adversarial"])
@pytest.mark.parametrize("w,h", S.LONG_GEOMETRIES, ids=[geom_ids(g) for g in S.LONG_GEOMETRIES])
def test_k_frame_p5_60_row_tasks(torch_cuda, oracle, w, h, kind, monkeypatch):
    """k_frame_p5 gets tasks of 60 rows only where a launch is long enough to give every wave 3.5 of them (csrc/frame_plan.cpp:
    p5_seg_rows; a forced short launch always gets 30): thousands of these small frames -- as many as the plan asks for on this device,
    8 distinct ones repeated.  A 60-row task's region of 64 cell rows spans five or six tile rows of the pixel-map record lists and
    holds more records (adversarial footage: over 64 in most regions, which then go to the list whole; the benchmark's footage: a
    few).  With pixel map and stripes, and with neither; the output poisoned before each launch; EVERY frame compared.  On the
    benchmark's footage kind without a pixel map k_frame_p5 must have settled the frames itself (check_listed)."""
    torch = torch_cuda
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    frames = S.footage(kind, w, h, 8)
    for bad, stripes in ((1, 1), (0, 0)):
        want, pixels, _ = oracle_clip(oracle, frames, w, h, 5, bad, stripes)
        nf = S.frames_for_60_rows(w, h, cu_count(torch), bool(bad) and len(pixels) > 0, stripes)
        assert (nf * w * h * 15) // 4 < 6 << 30, "packed and 16-bit frames of one launch: keep under 6 GB"
        s = make_stream(w, h)
        base = s.upload_packed([synth.pack_bits(f) for f in frames])
        s.analyse_first_frame(base, cs=5, bad_pix=bad, stripes=bool(stripes), rand_mode=1)
        packed = repeat(torch, base, nf)
        out = s.alloc_out(nf)
        out.fill_(POISON)
        before = S.listed_tiles()
        s.process(packed, out, cs=5, fix_pixels=bool(bad), stripes=bool(stripes))
        what = f"{kind} bad {bad} stripes {stripes}, {nf} frames"
        S.assert_took(P_P5, w, h, 60, what)
        check_on_device(torch, out, want, w, h, 60, what)
        check_listed(S.listed_tiles() - before, w, h, nf, kind == "normal" and not bad, what)
        s.close()
        del packed, out


# ------------------------------------------------------------------ the headline geometry
HW, HH = S.HEADLINE


@pytest.mark.parametrize("kind", S.KINDS)
def test_headline_k_frame_p5_long_launch(torch_cuda, oracle, kind, monkeypatch):
    """3584x1320 as the benchmark launches it: 8 columns x 11 segments of 60 rows, the last column folded in four, three parts in its last
    task -- as many frames as the plan needs for 60-row tasks on this device (about 165 on 256 CUs), four distinct ones per footage kind
    repeated (the oracle's cs5x5 costs about a second per frame of this size).  Forced through k_frame_p5 with pixel map and stripes,
    and with neither; every frame compared on the device, and on the benchmark's footage kind next to nothing left to the list."""
    torch = torch_cuda
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    w, h = HW, HH
    frames = S.footage(kind, w, h, 4)
    for bad, stripes in ((1, 1), (0, 0)):
        want, pixels, _ = oracle_clip(oracle, frames, w, h, 5, bad, stripes)
        nf = S.frames_for_60_rows(w, h, cu_count(torch), bool(bad) and len(pixels) > 0, stripes)
        assert (nf * w * h * 15) // 4 < 6 << 30
        s = make_stream(w, h)
        base = s.upload_packed([synth.pack14(f).astype("<u2") for f in frames])
        s.analyse_first_frame(base, cs=5, bad_pix=bad, stripes=bool(stripes), rand_mode=1)
        packed = repeat(torch, base, nf)
        out = s.alloc_out(nf)
        out.fill_(POISON)
        before = S.listed_tiles()
        s.process(packed, out, cs=5, fix_pixels=bool(bad), stripes=bool(stripes))
        what = f"{kind} bad {bad} stripes {stripes}, {nf} frames"
        p = S.assert_took(P_P5, w, h, 60, what)
        assert (p["cols"], p["segs"], p["fold"]) == (8, 11, 4)
        check_on_device(torch, out, want, w, h, 60, what)
        check_listed(S.listed_tiles() - before, w, h, nf, kind == "normal", what)
        s.close()
        del packed, out


@pytest.mark.parametrize("kind", S.KINDS)
def test_headline_k_frame_s(torch_cuda, oracle, kind, monkeypatch):
    """3584x1320 forced through k_frame_s, cs2x2 and cs3x3 with stripes, on every footage kind: eight frames (four distinct ones twice)
    are enough, its tasks are always 60 rows."""
    torch = torch_cuda
    monkeypatch.setenv("MLVFS_AMD_KF_S", "2")
    w, h = HW, HH
    frames = S.footage(kind, w, h, 4)
    for cs in (2, 3):
        want, _, _ = oracle_clip(oracle, frames, w, h, cs, 0, 1)
        s = make_stream(w, h)
        base = s.upload_packed([synth.pack14(f).astype("<u2") for f in frames])
        s.analyse_first_frame(base, cs=cs, bad_pix=0, stripes=True, rand_mode=1)
        packed = repeat(torch, base, 8)
        out = s.alloc_out(8)
        out.fill_(POISON)
        s.process(packed, out, cs=cs, fix_pixels=False, stripes=True)
        p = S.assert_took(P_S, w, h, 60, f"{kind} cs {cs}")
        assert (p["cols"], p["segs"], p["fold"]) == (8, 11, 4)
        check_on_device(torch, out, want, w, h, 60, f"{kind} cs {cs}")
        s.close()


# ------------------------------------------------------------------ focus-pixel maps through k_frame_p5
@pytest.mark.parametrize("seg_rows", S.SEG_ROWS)
@pytest.mark.parametrize("grid", ["dense", "thin"])
def test_focus_pixel_map_through_k_frame_p5(torch_cuda, oracle, grid, seg_rows, monkeypatch):
    """Focus-pixel maps (set_pixel_map(kind=1)) reached k_frame_p only: the tests that have one launch two or three frames.  Forced
    through k_frame_p5 in tasks of 30 rows (three frames) and of 60 (as many frames as the plan asks for): the grid of
    test_dense_focus_pixel_map, more than 64 records in every task's region, so every region goes to the list whole; and a thinner grid
    with at most 64 records in some regions -- a record per lane, patched in the step that loads its row -- and more in others
    (counted from the task cut: tests/test_stream_shapes.py: test_focus_map_regions)."""
    torch = torch_cuda
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    w, h = S.FOCUS_GEOMETRY
    pts = S.grid_map(w, h, *(S.DENSE_GRID if grid == "dense" else S.THIN_GRID))
    per_region = S.records_per_region(pts, w, h, seg_rows)
    assert max(per_region) > 64 and (min(per_region) > 64) == (grid == "dense"), per_region
    frames = [synth.normal_frame(w, h, frame=k) for k in range(3)]
    want = [oracle.chroma_smooth(oracle.apply_focus_pixels(f, BLACK, pts, (0, 0), 0), BLACK, 5) for f in frames]
    nf = 3 if seg_rows == 30 else S.frames_for_60_rows(w, h, cu_count(torch), True, 0)
    s = make_stream(w, h)
    s.set_pixel_map(pts, kind=1)
    packed = repeat(torch, s.upload_packed([synth.pack_bits(f) for f in frames]), nf)
    out = s.alloc_out(nf)
    out.fill_(POISON)
    before = S.listed_tiles()
    s.process(packed, out, cs=5, fix_pixels=True, stripes=False)
    S.assert_took(P_P5, w, h, seg_rows, f"{grid} grid")
    check_on_device(torch, out, want, w, h, seg_rows, f"{grid} grid, {nf} frames")
    listed, tiles = S.listed_tiles() - before, S.launch_tiles(w, h, nf)
    print(f"{grid} grid, tasks of {seg_rows} rows: {listed} of {tiles} tiles listed")
    if grid == "dense":                              # every region whole, so every tile at least once
        assert listed >= tiles
    s.close()
