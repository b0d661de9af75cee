"""The cases of tests/demosaic_cases.py are not vacuous (no GPU): with the intermediates of mlvfs_amd/demosaic.py, every interpolated
(site, channel) entry of the definition's table has sums below zero, below zero off a multiple of 16 (where a truncating shift would
differ from the floor), above 16 * 65535 and in range; at every border row, border column and corner the output bytes depend on the
reflection (the edge pixel repeated, and the mirror that repeats it, are the two wrong forms); both clamps of step 1, t = 0, t = 4095
and more than 1000 distinct t are hit; parameter sets of both matrix paths take part.  And the definition itself: a frame that is flat
per CFA colour renders to the half-size definition's pixel everywhere."""
import numpy as np
import pytest

from mlvfs_amd import demosaic, render

import demosaic_cases as dm
import render_cases as rc


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


@pytest.fixture(scope="module")
def all_cases():
    """[(frame, parameters)] of every size the GPU test runs"""
    return [fp for w, h in dm.SIZES for batch, _, _, _ in dm.dev_cases(w, h) for fp in batch]


def test_every_entry_of_the_table_meets_every_kind_of_sum(all_cases):
    kinds = ("negative", "negative off a multiple of 16", "above 16 * 65535", "in range")
    seen = {}
    for f, p in all_cases:
        st = demosaic.stages(f, p)
        h, w = f.shape
        y, x = np.mgrid[0:h, 0:w]
        for i in range(3):
            s, which = st["s"][i], st["which"][i]
            for yo in (0, 1):
                for xo in (0, 1):
                    if demosaic.SUM_OF[yo][xo][i] < 0:
                        continue
                    v = s[((y & 1) == yo) & ((x & 1) == xo)]
                    assert (which[yo::2, xo::2] == demosaic.SUM_OF[yo][xo][i]).all()
                    got = seen.setdefault((yo, xo, i), [0, 0, 0, 0])
                    got[0] += int((v < 0).sum())
                    got[1] += int(((v < 0) & (v % 16 != 0)).sum())
                    got[2] += int((v > 16 * 65535).sum())
                    got[3] += int(((v >= 0) & (v <= 16 * 65535)).sum())
    assert len(seen) == 8, sorted(seen)
    for entry, got in sorted(seen.items()):
        print(entry, dict(zip(kinds, got)))
        assert all(got), (entry, dict(zip(kinds, got)))


def test_the_sums_fit_32_bits_and_both_clamps_of_step_2_are_hit_in_every_channel(all_cases):
    lo, hi = [0] * 3, [0] * 3
    for f, p in all_cases:
        st = demosaic.stages(f, p)
        assert int(np.abs(st["sums"]).max()) < 1 << 22
        for i in range(3):
            m = (st["s"][i] + 8) >> 4
            lo[i] += int((m < 0).sum())
            hi[i] += int((m > 65535).sum())
    assert all(lo) and all(hi), (lo, hi)


BORDER_SIZES = [(4, 4), (5, 4), (4, 5), (7, 5), (6, 6), (16, 4), (32, 5), (30, 10), (16, dm.RUN + 1)]


@pytest.mark.parametrize("wrong", ["clamp", "mirror"])
def test_the_reflection_shows_at_every_border_pixel_class(lut, wrong):
    """rows 0, 1, H - 2, H - 1, columns 0, 1, W - 2, W - 1 and the four corners: pixels whose bytes another border rule changes"""
    for w, h in BORDER_SIZES:
        hit = np.zeros((h, w), bool)
        for batch, _, _, _ in dm.dev_cases(w, h):
            for f, p in batch:
                hit |= (demosaic.render(f, p, lut) != demosaic.render(f, p, lut, border=wrong)).any(axis=2)
        assert not hit[2:h - 2, 2:w - 2].any(), "the border rule reached the interior"
        classes = {"row 0": hit[0], "row 1": hit[1], "row H-2": hit[h - 2], "row H-1": hit[h - 1], "column 0": hit[:, 0], "column 1": hit[:, 1],
                   "column W-2": hit[:, w - 2], "column W-1": hit[:, w - 1], "corners": None}
        for name, v in classes.items():
            if v is None:
                assert hit[0, 0] and hit[0, w - 1] and hit[h - 1, 0] and hit[h - 1, w - 1], (w, h, wrong, "a corner does not depend on the rule")
            else:
                assert v.any(), (w, h, wrong, name)


def test_step_1_step_3_and_the_matrix_paths(all_cases):
    below = capped = 0
    ts = set()
    paths = set()
    for f, p in all_cases:
        st = demosaic.stages(f, p)
        below += int(st["below"].sum())
        capped += int((st["b"] == 65535).sum())
        ts.update(np.unique(st["t"]).tolist())
        paths.add(demosaic.matrix_fits_32(p))
    assert below and capped and 0 in ts and 4095 in ts and len(ts) > 1000, (below, capped, len(ts))
    assert paths == {True, False}
    for w, h in dm.SIZES:                                   # a batch of three holds a frame of each path
        for batch, _, _, _ in dm.dev_cases(w, h):
            if len(batch) == 3:
                assert {demosaic.matrix_fits_32(p) for _, p in batch} == {True, False}, (w, h)
    assert not demosaic.matrix_fits_32(dm.wide_param_set(0)[1]) and demosaic.matrix_fits_32(rc.param_set(0)[1])
    # the condition by hand: rows of 32767 and of 32768 in all
    assert demosaic.matrix_fits_32([0] * 4 + [32767, 0, 0, 0, -32767, 0, 10000, -10000, 12767])
    assert not demosaic.matrix_fits_32([0] * 4 + [32767, 0, 0, 0, -32768, 0, 0, 0, 0])
    assert not demosaic.matrix_fits_32([0] * 4 + [-(1 << 31)] * 9)


@pytest.mark.parametrize("w,h", [(4, 4), (5, 7), (8, 16)])
def test_a_frame_flat_per_colour_renders_to_the_half_size_pixel(lut, w, h):
    for k in range(8):
        (black, white), p = dm.param_set(k)
        g = np.random.default_rng(k)
        r_, g_, b_ = (int(v) for v in g.integers(max(black - 20, 0), min(white + 20, 65535) + 1, 3))
        f = dm.flat_frame(w, h, r_, g_, b_)
        want = render.render(f[:2, :2], p, lut)[0, 0]
        got = demosaic.render(f, p, lut)
        assert (got == want).all(), (w, h, k)


def test_the_reflection_rule_and_the_geometry():
    assert [demosaic.reflect(i, 5) for i in range(-2, 7)] == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert [demosaic.reflect(i, 4) for i in (-2, -1, 4, 5)] == [2, 1, 2, 1]
    assert demosaic.geom(4, 4) == (4, 4) and demosaic.geom(3584, 1320) == (3584, 1320) and demosaic.geom(8191, 4095) == (8191, 4095)
    for w, h in ((3, 4), (4, 3), (0, 0), (1 << 13, 1 << 12)):
        with pytest.raises(ValueError):
            demosaic.geom(w, h)
    # one pixel by hand: an R site in a frame flat but for itself
    p = [0, 4096, 4096, 4096] + [65536, 0, 0, 0, 65536, 0, 0, 0, 65536]
    f = np.full((6, 6), 1000, np.uint16)
    f[2, 2] = 1160
    st = demosaic.stages(f, p)
    assert st["b"][2, 2] == 1160 and st["sums"][0][2, 2] == 8 * 1160 + 16 * 1000 - 8 * 1000 and st["n"][1][2, 2] == 1080
    assert st["sums"][3][2, 2] == 12 * 1160 + 16 * 1000 - 12 * 1000 and st["n"][2][2, 2] == 1120 and st["n"][0][2, 2] == 1160
