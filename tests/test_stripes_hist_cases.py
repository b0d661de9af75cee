"""The frames of tests/stripes_hist_cases.py are what they are there for -- checked on the oracle's histogram alone, without a GPU: samples
on both sides of both ends of the LDS window and in the clamped bins, calls exactly on a bin edge, calls decided by each threshold
of add_pixel at every level pair, frames without an accepted call, and the long geometry's four properties.  Whoever moves a
constant of csrc/k_stripes.hip or a generator learns here which case has become vacuous.  The oracle itself is pinned to the
reference's stripes.c on every case and level pair."""
import numpy as np
import pytest

import stripes_hist_cases as SC
from mlvfs_amd import lib

W, H = 266, SC.SMALL_H


def rand_stream(amd, n_calls: int) -> np.ndarray:
    rnd = np.zeros(2 * n_calls + 2, np.uint16)
    amd.mlvfs_amd_rand_stream(lib.ptr(rnd), 2 * n_calls, 0, 1)
    return rnd


def near_edge(amd, f, black, white):
    """(calls with equal dither values, calls within 1e-6 of a bin edge: the ones the device hands to the host)"""
    n_calls = int(SC.calls_of(f, black, white)[2].sum())
    _, r1, r2, pos = SC.positions_of(f, black, white, rand_stream(amd, n_calls))
    return int((r1 == r2).sum()), int((np.abs(pos - np.rint(pos)) < 1e-6).sum())


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_ratio_frame_fills_the_window_edges_and_the_clamped_bins(oracle, level):
    f = SC.ratio_frame(W, H, *level)
    assert f.shape == (H, W) and f.dtype == np.uint16
    _, _, hist, num = oracle.stripes_compute(f, *level, want_hist=True)
    assert int(num.sum()) == int(SC.calls_of(f, *level)[2].sum()) == 24 * SC.groups_per_row(W) * H       # every call accepted
    edges = hist[2:, list(SC.WINDOW_EDGE_BINS)]
    assert edges.min() >= 10, edges
    assert hist[2:, 0].min() >= 100 and hist[2:, 65535].min() >= 100
    assert (hist[2:, 1:5] > 0).all() and (hist[2:, 65531:65535] > 0).all()
    assert not hist[:2].any() and not num[:2].any()


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_flat_frame_has_calls_exactly_on_a_bin_edge(amd, oracle, level):
    f = SC.flat_frame(W, H, *level)
    assert len(np.unique(f)) == 1
    _, _, hist, num = oracle.stripes_compute(f, *level, want_hist=True)
    assert int(num.sum()) == 24 * SC.groups_per_row(W) * H
    equal, near = near_edge(amd, f, *level)
    assert equal >= 50 and equal <= near < SC.RECHECK_CAP


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_every_small_case_stays_below_the_recheck_cap(amd, level):
    for name in SC.SMALL_CASES:
        for w in SC.WIDTHS:
            assert near_edge(amd, SC.small_case(name, w, *level), *level)[1] < SC.RECHECK_CAP, (name, w)


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_threshold_frame_has_calls_decided_by_each_threshold(oracle, level):
    black, white = level
    f = SC.threshold_frame(W, H, black, white, seed=W)
    decided = SC.deciding_values(f, black, white)
    assert all(n >= 100 for n in decided.values()), decided
    v = f.astype(np.int64) - black
    assert ((v < 0).sum() if black else (v == 0).sum()) >= 100                    # below black; at it where black is 0
    assert ((v > 32) & (v < SC.limit_of(white))).sum() >= 100                      # ordinary content
    # the restatement of MIN / MAX counts what the oracle accepts
    _, _, _, num = oracle.stripes_compute(f, black, white, want_hist=True)
    assert int(num.sum()) == int(SC.calls_of(f, black, white)[2].sum()) > 1000
    # white / 1.5 is an integer at every pair but 1 / 10000 (6666.67): the comparison is made in double either way
    assert (white / 1.5 == SC.limit_of(white)) == (white % 3 == 0)


def test_levels_have_whole_and_fractional_limits_and_16_bit_pairs():
    assert [w % 3 == 0 for _, w in SC.LEVELS] == [True, True, False, True, True, True]
    assert (16383 / 1.5, 65535 / 1.5) == (10922.0, 43690.0)
    assert sum(w > 16383 for _, w in SC.LEVELS) == 2 and sum(b > 16383 - 32 for b, _ in SC.LEVELS) == 1
    assert len(set(SC.LEVELS)) == 6 and SC.LEVELS[0] == (2048, 15000)


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_nothing_frames_accept_nothing_or_one_call(oracle, level):
    for name in SC.NOTHING:
        for w in SC.WIDTHS:
            f = SC.nothing_frame(name, w, H, *level)
            needed, co, hist, num = oracle.stripes_compute(f, *level, want_hist=True)
            assert int(num.sum()) == int(hist.sum()) == SC.expected_calls(name, w), (name, w)
            # no histogram is solved (num < frame_size / 128): the coefficients stay as they came in, 0 here, which counts as "needed"
            assert needed == 1 and list(co) == [65536, 65536, 0, 0, 0, 0, 0, 0], (name, w)
            if name == "one_call" and w > 10:
                assert num[2] == 1


def test_widths_are_the_group_counts_they_are_there_for():
    assert [SC.groups_per_row(w) for w in SC.WIDTHS] == [0, 1, 1, 2, 31, 32]
    assert 8 * (SC.groups_per_row(19) - 1) + 9 == 19 - 2                            # the second group's pb2: the row's last pixel but one
    assert 266 % 8 != 0 and 256 % 8 == 0


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_long_geometry(cus):
    w, h = SC.long_geometry(cus)
    p = SC.long_properties(w, h, cus)
    assert w == 2070 and SC.groups_per_row(w) == 258 and 258 % 8 != 0
    assert p["nblk"] > 2048 and p["nblk"] % 1024 != 0
    assert -(-p["nblk"] // 4) > 2 * cus and -(-p["nblk"] // 4) % cus != 0
    assert p["nblk"] % 4 != 0 and p["n_groups"] % 256 != 0
    if h > 1:
        q = SC.long_properties(w, h - 1, cus)
        assert not (q["three_passes_last_ragged"] and q["third_round_for_some"] and q["ragged_quad"] and q["ragged_block"])
    # no workgroup comes near the 65 536 calls of a 16-bit LDS counter (the launcher's guard stays out of it)
    assert -(-p["quads"] // cus) * 4 * 256 * 4 < 65536
    assert all(r0 >= 0 and r1 <= h - 12 for r0, r1 in SC.LONG_BANDS.values())


def test_long_frame_has_its_bands(amd, oracle):
    w, h = SC.long_geometry(256)
    f = SC.long_frame(w, h)
    a, b, ok = SC.calls_of(f, 2048, 15000)
    r0, r1 = SC.LONG_BANDS["dark"]
    assert r1 - r0 >= 4 and not ok[r0:r1].any() and ok[r0 - 1].any() and ok[r1].any()
    per_block = np.add.reduceat(ok.reshape(-1, 24).sum(1), np.arange(0, ok.shape[0] * ok.shape[1], SC.GROUPS_PER_BLOCK))
    assert (per_block == 0).sum() >= 2                                             # whole blocks without a call
    assert per_block[SC.SCAN_PASS - 1] > 0 and per_block[SC.SCAN_PASS] > 0 and per_block[2 * SC.SCAN_PASS] > 0
    r0, r1 = SC.LONG_BANDS["flat"]
    assert r1 - r0 >= 4 and len(np.unique(f[r0:r1])) == 1 and ok[r0:r1].all()
    assert np.array_equal(f[h - 12:h - 4], SC.ratio_frame(w, 8, 2048, 15000))
    equal, near = near_edge(amd, f, 2048, 15000)
    assert 100 <= near < SC.RECHECK_CAP
    _, _, hist, num = oracle.stripes_compute(f, 2048, 15000, want_hist=True)
    assert int(num.sum()) == int(ok.sum())
    assert hist[2:, list(SC.WINDOW_EDGE_BINS)].min() >= 1 and hist[2:, 0].min() >= 100 and hist[2:, 65535].min() >= 100


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
def test_oracle_equals_reference_on_every_case(oracle, reference, level):
    for name in SC.SMALL_CASES:
        for w in SC.WIDTHS:
            f = SC.small_case(name, w, *level)
            needed, co = oracle.stripes_compute(f, *level)
            ref_needed, ref_co = reference.stripes_compute(f, *level)
            assert needed == ref_needed and list(co) == list(ref_co), (name, w)
            # a solved histogram replaces what came in, a skipped one keeps it
            needed, co = oracle.stripes_compute(f, *level, coeffs=[70000] * 8)
            ref_needed, ref_co = reference.stripes_compute(f, *level, coeffs=[70000] * 8)
            assert needed == ref_needed and list(co) == list(ref_co), (name, w)
