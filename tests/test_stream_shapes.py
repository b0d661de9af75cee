"""The geometry list of the streaming kernels' task-shape tests (tests/stream_shapes.py) reaches every shape class -- checked against
the library's own cut of a frame into tasks (mlvfs_amd_test_stream_plan), without a GPU.  Whoever changes the column width, the task
length or the fold rule learns here which classes lost their geometry; the picked sizes would otherwise quietly stop being edges."""
import pytest

import stream_shapes as S


@pytest.mark.parametrize("seg_rows", S.SEG_ROWS)
def test_geometry_list_reaches_every_class(amd, seg_rows):
    lost = S.missing(S.GEOMETRIES, seg_rows)
    assert not lost, f"no geometry of stream_shapes.GEOMETRIES gives, with tasks of {seg_rows} rows: {lost}"
    assert all(w * h <= 800_000 for w, h in S.GEOMETRIES if (w, h) != S.HEADLINE)


def test_long_launch_subset_reaches_every_class_at_60_rows(amd):
    assert set(S.LONG_GEOMETRIES) <= set(S.GEOMETRIES) and S.HEADLINE not in S.LONG_GEOMETRIES
    lost = S.missing(S.LONG_GEOMETRIES, 60)
    assert not lost, f"no geometry of stream_shapes.LONG_GEOMETRIES gives, with tasks of 60 rows: {lost}"


def test_every_listed_geometry_has_two_segments_and_more(amd):
    """(a geometry of one segment counts for no class: nothing folds, there is no last segment)"""
    for w, h in S.GEOMETRIES:
        for seg_rows in S.SEG_ROWS:
            assert S.shape(w, h, seg_rows)["segs"] >= 2 and S.classes(w, h, seg_rows), (w, h, seg_rows)


def test_classes_are_those_of_the_cut(amd):
    """The classifier on shapes whose cut is known (csrc/frame_plan.cpp: 62 items per column; a last column of <= 14 items folds in
    four, of <= 30 in two)"""
    assert S.col_items() == 62
    assert S.shape(3584, 1320, 60) == dict(cols=8, segs=11, fold=4, tasks=80, vec=1, last_items=14, last_rows=60, folded=3, last_parts=3)
    assert S.classes(3584, 1320, 60) == {"last column of 13-14 items", "fold 4, VEC 1", "fold 4, 3 part(s) in the last folded task",
                                         "last segment of a full task", ">= 3 folded task(s) per column", ">= 3 column(s)"}
    assert S.classes(504, 122, 30) == {"last column of 1 items", "fold 4, VEC 2", "fold 4, 3 part(s) in the last folded task",
                                       "last segment of 1 row", "1 folded task(s) per column", "2 column(s)"}
    assert S.classes(744, 244, 60) == {"last column of 31 items", "fold 1, VEC 2", "last segment of 2 rows", "2 column(s)"}
    assert S.classes(3584, 66, 60) == set()                          # one segment


def test_focus_map_regions(amd):
    """The two grids of test_gpu_stream_shapes.py: the dense one has more records than a wave has lanes in every task's region (the
    whole region goes to the list), the thin one in some regions and not in others -- at both task lengths"""
    w, h = S.FOCUS_GEOMETRY
    for seg_rows in S.SEG_ROWS:
        dense = S.records_per_region(S.grid_map(w, h, *S.DENSE_GRID), w, h, seg_rows)
        thin = S.records_per_region(S.grid_map(w, h, *S.THIN_GRID), w, h, seg_rows)
        assert len(dense) == len(thin) == len(S.task_regions(w, h, seg_rows)) >= 3
        assert min(dense) > 64, dense
        assert 0 < min(thin) <= 64 < max(thin), thin
