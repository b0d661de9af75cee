"""The cases of tests/p5_table_cases.py are what they are there for -- checked with the oracle and the library's host-side plan, without
a GPU: every edge value of k_frame_p5's EV table often enough, no band of rows that is all below, all at or all above black unless the
case is about such bands, and frames that chroma smoothing changes -- a loader that smoothed nothing must not pass on them."""
import numpy as np
import pytest

import level_cases as LC
import p5_table_cases as PC
import stream_shapes as S

SMOOTHED = [c for c in PC.CASES if c[1] < 16383]


def test_levels_reach_both_ends_of_the_table():
    assert PC.BLACKS == (0, 1, 2048, 8191, 16383, 16384)
    for black in PC.BLACKS:
        assert PC.white_of(black) > black + 64, "the packed stripes form"        # (else the streaming kernels decline)
    # entry 0 (below black) is read wherever black >= 1, the last entry (16383 above black) at black 0
    assert PC.edge_values(0) == [0, 1, 16383] and PC.edge_values(1) == [0, 1, 2, 16383]
    assert PC.edge_values(2048) == [0, 2047, 2048, 2049, 16383]
    assert PC.edge_values(16384) == [0, 16383]
    assert PC.JUDGED_BLACKS == (0, 1, 2048, 8191, 16384)


def test_geometries_are_the_cuts_they_are_there_for(amd):
    s = S.shape(504, 122, 30)
    assert (s["cols"], s["last_items"], s["fold"], s["vec"]) == (2, 1, 4, 2)
    s = S.shape(112, 484, 30)
    assert (s["cols"], s["last_items"], s["fold"], s["vec"]) == (1, 14, 4, 1)
    assert S.shape(112, 484, 60)["tasks"] == 2 and s["tasks"] < 16, "fewer tasks than a workgroup has waves"


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_edge_values_and_bands(case):
    (w, h), black = case
    for f in PC.footage(w, h, black):
        assert f.shape == (h, w) and f.dtype == np.uint16 and int(f.max()) <= 16383
        for v in PC.edge_values(black):
            assert int((f == v).sum()) >= 100, (v, int((f == v).sum()))
        if black < 16383:
            for i, classes in enumerate(PC.band_classes(f, black)):
                assert len(classes) >= 2, f"band {i} is all {classes}"
    if black == 16384:
        assert all(int(f.max()) < black for f in PC.footage(w, h, black))


@pytest.mark.parametrize("case", SMOOTHED, ids=PC.case_id)
def test_smoothing_changes_the_frames(oracle, case):
    (w, h), black = case
    for f in PC.footage(w, h, black):
        changed, cells = PC.interior_cells_changed(f, oracle.chroma_smooth(f, black, 5))
        assert changed * 2 >= cells, f"{changed} of {cells} interior cells"


def test_dark_rows_case(amd, oracle):
    (w, h), black = PC.DARK_ROWS_GEOMETRY, PC.DARK_ROWS_BLACK
    want = {"at": {"at"}, "below": {"below"}, "mixed": {"at", "below"}}
    bands = PC.dark_bands()
    assert {kind for _, kind in bands} == set(PC.DARK_BAND_KINDS) and len(bands) >= 6
    dark = {y for y0, _ in bands for y in range(y0, y0 + PC.BAND)}
    assert all(y0 % 2 == 0 for y0, _ in bands), "whole cell rows: whole steps of the loader"
    # at most two dark cell rows in any five: the median of a window is a bright cell's
    assert PC.DARK_PERIOD - PC.BAND >= 2 * 3 and PC.BAND == 4
    # the reference of every task (tasks of 30 rows: a forced short launch) comes from bright rows
    assert S.stream_plan(w, h, 30)[1] == 3
    assert not (PC.reference_rows(h, 30) & dark), sorted(PC.reference_rows(h, 30) & dark)
    for f in PC.dark_rows_footage():
        assert f.shape == (h, w) and int(f.max()) <= 16383
        for y0, kind in bands:
            assert PC.row_classes(f, black, y0, y0 + PC.BAND) == want[kind], (y0, kind)      # this case says so
        for y in range(0, h, 2):                                             # the other steps: the loader's common path
            if y not in dark:
                assert PC.row_classes(f, black, y, y + 2) == {"above"}, y
        bright = np.array([y not in dark for y in range(h)])
        assert (f[bright] == black + 1).sum() >= 100 and (f[bright] == 16383).sum() >= 100
        changed, cells = PC.interior_cells_changed(f, oracle.chroma_smooth(f, black, 5), bright_rows_only=True)
        assert changed * 2 >= cells, f"{changed} of {cells} interior cells of the bright rows"
