"""The cases of tests/p5_pair_cases.py are the edges they are there for -- checked against the library's own cut of a frame into tasks
(mlvfs_amd_test_stream_plan) and against the frames themselves, without a GPU.  Whoever changes the task length, the fold rule or the
footage learns here which class of k_frame_p5's pair step lost its case."""
import numpy as np
import pytest

import p5_pair_cases as PP
import stream_shapes as S
from mlvfs_amd import synth


@pytest.mark.parametrize("seg_rows", S.SEG_ROWS)
def test_parity_geometries_reach_every_last_segment(amd, seg_rows):
    """Last segments of 1, 2, 3 and 4 rows behind full tasks, odd and even tasks and a folded last column, at both task lengths"""
    cases = [c for c in PP.CASES if c[:2] in PP.PARITY_GEOMETRIES]
    lost = PP.missing(cases, seg_rows)
    assert not lost, f"no geometry of p5_pair_cases.PARITY_GEOMETRIES gives, with tasks of {seg_rows} rows: {lost}"
    assert [S.shape(w, h, seg_rows)["last_rows"] for w, h in PP.PARITY_GEOMETRIES] == [1, 2, 3, 4]
    assert all(S.shape(w, h, seg_rows)["segs"] >= 2 for w, h in PP.PARITY_GEOMETRIES)


def test_the_whole_list_covers_the_classes(amd):
    assert not PP.missing(PP.CASES, 30)
    assert set(PP.PARITY_GEOMETRIES[:2]) <= set(S.GEOMETRIES)
    for c in ("odd task", "even task", "task of <= 4 rows", "folded last column"):
        assert any(c in PP.classes(*case) for case in PP.CASES), c


def test_the_short_and_the_low_geometry(amd):
    """One segment of three rows (fewer than the four rows of the warm-up: no pair step has an output stage); a frame of six rows of
    which only rows 2 and 3 are smoothed (chroma_smooth.c:25: 4 <= y < h - 5)"""
    w, h = PP.SHORT_GEOMETRY
    s = S.shape(w, h, 30)
    assert (s["segs"], s["last_rows"], s["fold"], s["cols"]) == (1, 3, 1, 8)
    w, h = PP.LOW_GEOMETRY
    s = S.shape(w, h, 30)
    assert (s["segs"], s["last_rows"], s["vec"]) == (1, 6, 2)
    assert [j for j in range(h // 2) if 4 <= 2 * j < h - 5] == [2, 3]


@pytest.mark.parametrize("case", PP.CASES, ids=PP.case_id)
def test_a_forced_short_launch_goes_to_k_frame_p5(amd, case, monkeypatch):
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")
    w, h, _ = case
    p = S.frame_plan(w, h, 5, 3, 256, False, 0)
    assert p is not None and p["first"] == S.P_P5 and p["seg_rows"] == 30 and p["list_after"], p


def test_seam_geometry_is_one_task_of_pairs(amd):
    w, h = PP.SEAM_GEOMETRY
    assert S.stream_plan(w, h, 30) == (1, 1, 1, 1) and h // 2 == 30
    assert PP.ROW_A % 2 == 0 and PP.ROW_B % 2 == 1 and PP.ROW_A // 2 != PP.ROW_B // 2


def test_seam_frames_differ_in_one_row_of_a_pair():
    """dark: the only row with a pixel at or below black is ROW_A in frame 0 and ROW_B in frame 1 (its partner has none); uncertain:
    the only row whose median colour difference lies a stop and more from the rest is that row; pixel map: one cell in each row"""
    w, h = PP.SEAM_GEOMETRY
    for kind in PP.SEAM_KINDS:
        frames = PP.seam_frames(kind)
        assert len(frames) == 2 and all(f.shape == (h, w) and f.dtype == np.uint16 for f in frames)
        for f, row in zip(frames, (PP.ROW_A, PP.ROW_B)):
            assert PP.rows_with(f, "dark") == ([row] if kind == "dark" else [])
            assert PP.rows_with(f, "uncertain") == ([row] if kind == "uncertain" else [])
            assert int(f.min()) >= synth.BLACK and int(f.max()) <= 16383
    pm = PP.seam_pixel_map("pixel_map")
    assert sorted(int(y) // 2 for _, y in pm) == [PP.ROW_A, PP.ROW_B]
    assert PP.seam_pixel_map("dark") is None and PP.seam_pixel_map("uncertain") is None
    assert set(PP.PARENT_LISTED) == set(PP.SEAM_KINDS)
