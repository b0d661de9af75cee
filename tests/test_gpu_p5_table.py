"""k_frame_p5's loader reads a pixel's EV from the whole of raw2ev in LDS, indexed by pixel - black + 1 (csrc/k_frame_p.hip): the cases of
tests/p5_table_cases.py put pixels on every edge of that table -- below black, at black, one above, 16383 -- at black levels on both
of its ends, switch the loader between its two forms from step to step, and give a workgroup of sixteen waves fewer tasks than waves.

Every launch is forced through k_frame_p5 (MLVFS_AMD_KF_P=2, MLVFS_AMD_KF_P5=2), proved from the plan it took, and compared bit for bit
with the oracle.  The list-mode k_frame does every tile again that k_frame_p5 lists, and would hide a wrong loader behind right
bytes: without a pixel map the launches may list at most stream_shapes.CALM_PERCENT of their tiles (a sparse outlier cannot move a
median of 25).

Listing depends on the packed medians alone, not on how the loader forms them.  Measured on one MI355X with the loader that rebuilt
log2 from the mantissa table and with the full table, the same counts from both: without a pixel map 0 of 60 (504x122) and 0 of 51
(112x484) tiles at black 0, 1, 2048, 8191 and 16384, all 60 and 48 of 51 at black 16383 (reported, not judged: no pixel lies above
black there and the references are INT_MIN differences); the dark-rows case 3 of 60; with the pixel map, whose detection takes
most sprinkled pixels for defects, most regions go to the list whole (48 of 51 at 112x484 black 16384)."""
import numpy as np
import pytest

import level_cases as LC
import p5_table_cases as PC
import stream_shapes as S
from mlvfs_amd import synth
from stream_shapes import P_P5

pytestmark = pytest.mark.gpu

POISON = 0x5A5A


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    monkeypatch.delenv("MLVFS_AMD_KF_S", raising=False)


def check(got, want, what):
    for k in range(len(want)):
        if not np.array_equal(got[k], want[k]):
            ys, xs = np.nonzero(got[k] != want[k])
            y, x = int(ys[0]), int(xs[0])
            raise AssertionError(f"{what} frame {k}: {len(ys)} px differ, x {xs.min()}..{xs.max()}, y {ys.min()}..{ys.max()}; "
                                 f"at ({x}, {y}) {got[k][y, x]} for {want[k][y, x]}")


def run(oracle, frames, w, h, black, white, pmap, stripes, what, launches=1):
    """One clip through k_frame_p5, `launches` times on the same stream; the tiles it listed per launch"""
    from mlvfs_amd.stream import ClipStream, to_numpy_u16
    pixels = oracle.detect_bad_pixels(frames[0], black, 1) if pmap else None
    coeffs = LC.REALISTIC if stripes else None
    want = LC.oracle_pass(oracle, frames, black, white, 5, pixels, coeffs)
    s = ClipStream(w, h, 14, black, white, device=0)
    if pmap:
        s.set_pixel_map(pixels)
    if stripes:
        s.set_stripes(1, coeffs)
    src = s.upload_packed([synth.pack_bits(f) for f in frames])
    out = s.alloc_out(len(frames))
    listed = []
    for n in range(launches):
        out.fill_(POISON)
        before = S.listed_tiles()
        s.process(src, out, cs=5, fix_pixels=pmap, stripes=stripes)
        p = S.assert_took(P_P5, w, h, 30, what)
        check(to_numpy_u16(out), want, f"{what} launch {n}")
        listed.append(S.listed_tiles() - before)
    s.close()
    return listed, p


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_table_edges(torch_cuda, oracle, case):
    """The benchmark's footage kind with a hundredth of its pixels on the table's edges, at every black level of the cases: with pixel
    map (detection mode 1: the sprinkled pixels fill it, most regions go to the list whole -- reported) and stripes, and with neither
    (judged: next to nothing listed).  At black 16384 every pixel lies below black, nothing is smoothed and the kernel still unpacks
    and applies stripes; at 16383 no pixel lies above black either, a reference of INT_MIN differences can saturate whole medians:
    reported."""
    (w, h), black = case
    frames = PC.footage(w, h, black)
    white = PC.white_of(black)
    for pmap, stripes in ((True, True), (False, False)):
        what = f"{w}x{h} black {black} white {white} map {int(pmap)} stripes {int(stripes)}"
        (listed,), _ = run(oracle, frames, w, h, black, white, pmap, stripes, what)
        tiles = S.launch_tiles(w, h, len(frames))
        print(f"{what}: {listed} of {tiles} tiles listed")
        if not pmap and black in PC.JUDGED_BLACKS:
            assert listed * 100 <= tiles * S.CALM_PERCENT, f"{what}: k_frame_p5 listed {listed} of {tiles} tiles"


def test_dark_rows_among_bright_ones(torch_cuda, oracle):
    """Bands of four pixel rows at or below black between bright ones: the loader's form changes from step to step, and in the dark
    bands every lane of a wave reads the table's entry 0 or 1 at once.  No window of 5 x 5 cells holds more than 10 dark cells and
    every task's reference comes from bright rows (tests/test_p5_table_cases.py), so k_frame_p5 settles the frames itself."""
    (w, h), black = PC.DARK_ROWS_GEOMETRY, PC.DARK_ROWS_BLACK
    frames = PC.dark_rows_footage()
    tiles = S.launch_tiles(w, h, len(frames))
    for stripes in (False, True):
        (listed,), _ = run(oracle, frames, w, h, black, synth.WHITE, False, stripes, f"dark rows, stripes {int(stripes)}")
        print(f"dark rows, stripes {int(stripes)}: {listed} of {tiles} tiles listed")
        assert listed * 100 <= tiles * S.CALM_PERCENT, f"dark rows: k_frame_p5 listed {listed} of {tiles} tiles"


def test_fewer_tasks_than_waves(torch_cuda, oracle):
    """One frame of 112x484 is a handful of tasks for the sixteen waves of a workgroup: the idle waves leave at once, and the last
    wave out resets the tickets for the next launch on the stream -- the same launch again, which must find them at zero"""
    w, h = PC.FEW_TASKS_GEOMETRY
    frames = [synth.normal_frame(w, h, frame=0)]
    listed, p = run(oracle, frames, w, h, synth.BLACK, synth.WHITE, False, False, "one frame, twice", launches=2)
    assert 0 < p["tasks"] < 16, p
    tiles = S.launch_tiles(w, h, 1)
    assert all(n * 100 <= tiles * S.CALM_PERCENT for n in listed), f"k_frame_p5 listed {listed} of {tiles} tiles"
