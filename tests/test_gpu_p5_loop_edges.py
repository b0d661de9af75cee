"""The edges of k_frame_p5's step loop against the oracle.  The kernel runs a task of n rows as four warm-up steps, a main loop of pairs
of steps with output stage and prefetch, and one or two last steps without prefetch (csrc/k_frame_p.hip); the sizes of
tests/p5_loop_cases.py give tasks of 1 .. 5 rows (the warm-up alone, an empty, a one-pair and a two-pair main loop, one and two last
steps), last tasks of 1 and 2 rows behind full ones, in one narrow column, a column folded in four, a full column next to a folded one,
and in both unpack alignments (tests/test_p5_loop_edges.py checks that on the CPU).

Every launch is forced through k_frame_p5 and proved from the plan it took; two frames per launch, the output poisoned before each
launch with one spare frame behind the last, which must come back untouched; each launch twice on the same stream (the second finds
the tickets the first one left); outputs bit for bit the oracle's.  The list-mode k_frame does every tile again that k_frame_p5 lists:
without a pixel map a launch may list at most stream_shapes.CALM_PERCENT of its tiles -- with these few tiles, nearly always none."""
import numpy as np
import pytest

import level_cases as LC
import p5_loop_cases as LP
import stream_shapes as S
from mlvfs_amd import synth
from stream_shapes import P_P5
from test_gpu_stream import BLACK, WHITE, make_stream

pytestmark = pytest.mark.gpu

POISON = 0x5A5A
NFRAMES = 2


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")


def check(got, want, w, h, what):
    for k in range(len(want)):
        if not np.array_equal(got[k], want[k]):
            ys, xs = np.nonzero(got[k] != want[k])
            y, x = int(ys[0]), int(xs[0])
            rows = sorted({int(v) // 2 for v in ys})
            raise AssertionError(f"{what} frame {k}: {len(ys)} px differ, x {xs.min()}..{xs.max()}, cell rows {rows[:40]} of tasks of "
                                 f"{LP.task_rows(h)} rows; at ({x}, {y}) {got[k][y, x]:#x} for {want[k][y, x]:#x}")


def run_case(oracle, kind, w, h):
    """The clip's pixel map (the oracle's detection on the first frame; on the smallest frames it finds nothing) and stripe gains are
    set from outside: only the steady-state pass runs here, and starts with k_frame_p5"""
    from mlvfs_amd.stream import to_numpy_u16
    frames = S.footage(kind, w, h, NFRAMES)
    for pmap, stripes in ((True, True), (False, False)):
        pixels = oracle.detect_bad_pixels(frames[0], BLACK, 0) if pmap else None
        coeffs = LC.REALISTIC if stripes else None
        want = LC.oracle_pass(oracle, frames, BLACK, WHITE, 5, pixels, coeffs)
        s = make_stream(w, h)
        if pmap:
            s.set_pixel_map(pixels)
        if stripes:
            s.set_stripes(1, coeffs)
        packed = s.upload_packed([synth.pack_bits(f) for f in frames])
        out = s.alloc_out(NFRAMES + 1)               # (the kernels write packed.shape[0] frames: the last one is spare)
        for launch in range(2):
            what = f"{w}x{h} {kind} map {int(pmap)} ({0 if pixels is None else len(pixels)} px) stripes {int(stripes)} launch {launch}"
            out.fill_(POISON)
            before = S.listed_tiles()
            s.process(packed, out, cs=5, fix_pixels=pmap, stripes=stripes)
            S.assert_took(P_P5, w, h, LP.SEG_ROWS, what)
            got = to_numpy_u16(out)
            assert (got[NFRAMES] == POISON).all(), f"{what}: {int((got[NFRAMES] != POISON).sum())} px of the spare frame written"
            check(got, want, w, h, what)
            listed, tiles = S.listed_tiles() - before, S.launch_tiles(w, h, NFRAMES)
            print(f"{what}: {listed} of {tiles} tiles listed")
            if not pmap and kind == "normal":
                assert listed * 100 <= tiles * S.CALM_PERCENT, f"{what}: k_frame_p5 listed {listed} of {tiles} tiles"
        s.close()


@pytest.mark.parametrize("case", LP.CASES, ids=LP.case_id)
def test_loop_edges(torch_cuda, oracle, case):
    """The benchmark's footage kind at every size of the cases, with pixel map and stripes and with neither"""
    run_case(oracle, "normal", *case)


def test_loop_edges_low_light(torch_cuda, oracle):
    """Underexposed footage: the loader takes its second form in some steps and not in others on both sides of the boundary between
    the main loop and the last steps (what it lists is reported, not judged: dark references saturate medians)"""
    run_case(oracle, "low_light", *LP.LOW_LIGHT_CASE)
