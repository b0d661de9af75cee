"""The sizes of tests/p5_loop_cases.py are the edges they are there for -- checked against the library's own cut of a frame into tasks
(mlvfs_amd_test_stream_plan) and the plan of a forced short launch, without a GPU: the heights give tasks of every length at which
another part of k_frame_p5's step loop runs, the widths the column shapes, and the launches are so small that the bound on listed
tiles of tests/test_gpu_p5_loop_edges.py means "none" nearly everywhere."""
import numpy as np
import pytest

import p5_loop_cases as LP
import stream_shapes as S
from mlvfs_amd import synth


def test_heights_reach_every_part_of_the_loop():
    """Tasks of 1 .. 5 rows: the warm-up alone with one and with two last steps, then a main loop of one and of two pairs; the taller
    frames end in a task of 1 and of 2 rows behind full ones"""
    assert [LP.task_rows(h) for h in LP.HEIGHTS] == [[1], [2], [3], [4], [5], [30, 1], [30, 2], [30, 30, 1]]
    assert [LP.loop_parts(n) for n in (1, 2, 3, 4, 5)] == [(4, 0, 1), (4, 0, 2), (4, 1, 1), (4, 1, 2), (4, 2, 1)]
    assert LP.loop_parts(30) == (4, 14, 2) and LP.loop_parts(60) == (4, 29, 2)
    # every combination of (main loop runs or not, one or two last steps) occurs among the tasks of the cases
    seen = {(LP.loop_parts(n)[1] > 0, LP.loop_parts(n)[2]) for h in LP.HEIGHTS for n in LP.task_rows(h)}
    assert seen == {(False, 1), (False, 2), (True, 1), (True, 2)}


@pytest.mark.parametrize("case", LP.CASES, ids=LP.case_id)
def test_the_cut_of_a_case(amd, case):
    w, h = case
    cols, segs, fold, tasks = S.stream_plan(w, h, LP.SEG_ROWS)
    s = S.shape(w, h, LP.SEG_ROWS)
    assert segs == len(LP.task_rows(h)) and s["last_rows"] == LP.task_rows(h)[-1]
    assert s["vec"] == {16: 1, 112: 1, 504: 2, 520: 2}[w]            # (w % 16 == 8: odd pixel rows start two bytes into a dword)
    assert cols == (1 if w <= 112 else 2)
    # one segment folds nothing; with two and more the narrow last column folds in four, and its groups end at different rows
    assert s["last_items"] == {16: 2, 112: 14, 504: 1, 520: 3}[w]
    assert fold == (4 if segs >= 2 else 1)
    if fold > 1:
        assert s["folded"] == 1 and s["last_parts"] == segs           # one folded task: 2 or 3 of its 4 groups have rows
        assert tasks == (cols - 1) * segs + 1
    else:
        assert tasks == cols * segs


@pytest.mark.parametrize("case", LP.CASES + [LP.LOW_LIGHT_CASE], ids=LP.case_id)
def test_a_forced_launch_of_two_frames_goes_to_k_frame_p5(amd, case, monkeypatch):
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    w, h = case
    for pmap, stripes in ((True, True), (False, False)):
        p = S.frame_plan(w, h, 5, 2, 256, pmap, stripes)
        assert p is not None and p["first"] == S.P_P5 and p["seg_rows"] == LP.SEG_ROWS and p["list_after"], p
        cols, segs, fold, tasks = S.stream_plan(w, h, LP.SEG_ROWS)
        assert (p["cols"], p["segs"], p["fold"], p["tasks"]) == (cols, segs, fold, 2 * tasks)


def test_tile_counts_and_what_may_be_listed():
    """Two frames per launch: up to 19 tiles nothing may be listed; the largest cases may list a tile or two"""
    allowed = {c: LP.allowed_listed(*c, 2) for c in LP.CASES}
    assert S.launch_tiles(16, 2, 2) == 2 and S.launch_tiles(520, 122, 2) == 50
    assert all(n == 0 for (w, h), n in allowed.items() if S.launch_tiles(w, h, 2) < 20)
    assert max(allowed.values()) == 2 and allowed[(504, 122)] == 2 and allowed[(112, 122)] == 0


def test_footage_of_the_cases():
    """The benchmark's footage kind keeps every pixel above black on the smallest frames (the loader's common form in every step) and
    has its dead pixels on the taller ones; the low-light case switches the loader between its two forms on both sides of the boundary
    between the main loop and the last steps"""
    for w, h in LP.CASES:
        f = S.footage("normal", w, h, 2)
        assert all(x.shape == (h, w) and x.dtype == np.uint16 and int(x.max()) <= 16383 for x in f)
        assert not np.array_equal(f[0], f[1])
    w, h = LP.LOW_LIGHT_CASE
    assert LP.task_rows(h) == [30, 1]
    # cell rows with a pixel at or below black, per frame: the loader's form changes inside the main loop of the first task, and some
    # frame has dark and bright rows among the task's last steps (rows 28 .. 30) and the main loop's last ones
    dark = [(x <= synth.BLACK).reshape(h // 2, 2, w).any(axis=(1, 2)) for x in S.footage("low_light", w, h, 2)]
    assert all(d[:4].all() and 0 < d[4:26].sum() < 22 for d in dark), [d.astype(int) for d in dark]
    assert any(d[26:28].any() and not d[26:28].all() and d[28:].any() and not d[28:].all() for d in dark), [d.astype(int) for d in dark]
