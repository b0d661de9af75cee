"""Rendered full-size frames demosaiced by AMaZE, on the CPU: the definition of mlvfs_amd/amaze_render.py with the checker's AMaZE on the
cases of tests/amaze_render_cases.py.  The cases reach what they are there for -- finite planes, both clamps of step 3, values that
differ from the linear filter's -- and tell the definition from five wrong ones; step 3 on crafted values; the geometry."""
import numpy as np
import pytest

from mlvfs_amd import amaze_render, demosaic, lib, look, render

import amaze_render_cases as ac
import demosaic_cases as dm


@pytest.fixture(scope="module")
def staged(oracle):
    """the definition's intermediates of every case, computed once: [(label, frame, parameters, set, stages)]"""
    out = []
    for i, (w, h, f, p, label) in enumerate(ac.cases()):
        out.append((label, f, p, i % ac.NSETS, amaze_render.stages(f, p, oracle.amaze_demosaic)))
    return out


def test_the_case_set(staged):
    assert len(staged) == 30 and len({s[0] for s in staged}) == 30
    assert [demosaic.matrix_fits_32(dm.param_set(k)[1]) for k in range(ac.NSETS)] == [True, False, True]
    assert not demosaic.matrix_fits_32(ac.wide_set()[1]) and ac.wide_set()[1] != dm.param_set(1)[1]
    assert not any(w % 16 == 0 for w, _ in ac.SIZES) and ac.FAST_SIZE[0] % 16 == 0      # the fast forms need the extra size


def test_the_rows_size_has_one_complete_tile():
    w, h, nfx, nfy = ac.rows_size()
    assert (nfx, nfy) == (1, 1), "k_amaze_rows runs, on exactly one tile"
    assert amaze_render.geom(w, h) == (w, h)
    import ctypes as C
    L = lib.load()
    for ww, hh in ((w - 4, h), (w, h - 1)):                       # no smaller neighbour has one
        a, b = C.c_int(-1), C.c_int(-1)
        L.mlvfs_amd_amaze_rows_extent(ww, hh, C.byref(a), C.byref(b))
        assert a.value * b.value == 0, (ww, hh)


def test_every_amaze_value_is_finite(staged):
    for label, _, _, _, st in staged:
        assert np.isfinite(st["planes"]).all(), label


def test_a_sites_own_channel_rounds_back_to_b(staged):
    for label, _, _, _, st in staged:
        own = np.take_along_axis(st["n"], st["site"][None], 0)[0]
        assert np.array_equal(own, st["b"]), (label, int((own != st["b"]).sum()))
        assert np.array_equal(st["raw"].astype(np.int64), st["b"]), label       # float32(b) is exact


def test_both_clamps_of_step_3_are_reached(staged):
    below = [label for label, _, _, _, st in staged if (st["planes"] < 0).any()]
    above = [(label, k) for label, _, _, k, st in staged if (st["planes"] > 65535).any()]
    assert len(below) == 30, "values below 0 in every case"
    assert len(above) == 24, [a[0] for a in above]
    assert any(k == 1 for _, k in above), "cases of param_set(1) among them"
    for label, _, _, _, st in staged:
        assert st["n"].min() >= 0 and st["n"].max() <= 65535, label


def test_n_differs_from_the_linear_filters_at_about_half_of_the_values(staged):
    """a site's own channel is the same in both, a third of the values; most interpolated ones differ on these frames"""
    differ = total = 0
    for label, f, p, _, st in staged:
        lin = demosaic.stages(f, p)["n"]
        d = int((lin != st["n"]).sum())
        assert 0.35 * lin.size < d <= 2 * lin.size // 3, (label, d / lin.size)
        differ += d
        total += lin.size
    assert 0.4 < differ / total < 0.6, differ / total


@pytest.mark.parametrize("kind", ac.VARIANTS)
def test_the_cases_tell_a_wrong_definition_apart(oracle, staged, kind):
    """in n, in t and in the 16-bit index, on every case where the wrong form can show at all (the clamp only where AMaZE overshoots
    upwards: below zero both forms give 0 after step 3's own clamp ... which the unclamped form lacks, so it shows everywhere)"""
    shown = 0
    for label, f, p, _, st in staged:
        n = ac.variant_n(kind, f, p, oracle.amaze_demosaic)
        t, t16 = ac.matrix(p, n)
        if not np.array_equal(n, st["n"]):
            assert not np.array_equal(t16, st["t16"]), (kind, label)
            shown += 1 if not np.array_equal(t, st["t"]) else 0
    assert shown >= 24, (kind, shown)


def test_step_3_on_crafted_values():
    v = np.array([c[0] for c in ac.CRAFTED], np.float32)
    want = [c[1] for c in ac.CRAFTED]
    got = amaze_render.sample16(v)
    assert got.dtype == np.int64 and list(got) == want, [(float(a), int(b), c) for a, b, c in zip(v, got, want) if b != c]
    assert np.isnan(np.clip(np.float32("nan"), 0, 65535)), "np.clip alone hands NaN on: the definition must not rest on it"
    planes, n = ac.crafted_planes(48, 37)
    assert np.array_equal(amaze_render.sample16(planes), n)
    for c in range(3):                                            # every crafted value in every channel
        assert len(np.unique(n[c])) == len(set(want)) and np.isnan(planes[c]).any()


def test_render_goes_through_the_three_tone_forms(oracle):
    """render() is develop() of the stages: the table, a look and a deep look see the same t and t16"""
    import deep_cases as dc
    import look_cases as lc
    w, h, f, p, _ = ac.cases()[4]
    st = amaze_render.stages(f, p, oracle.amaze_demosaic)
    rgb = amaze_render.render(f, p, oracle.amaze_demosaic)
    assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, render.tone(st["t"]))
    lk, lk16 = lc.look_of("random17"), dc.look_of("random3")
    got = amaze_render.render(f, p, oracle.amaze_demosaic, look=lk)
    assert np.array_equal(got, look.apply(st["t"], *lk).transpose(1, 2, 0)) and not np.array_equal(got, rgb)
    deep = amaze_render.render(f, p, oracle.amaze_demosaic, look16=lk16)
    assert deep.dtype == np.uint16 and np.array_equal(deep, look.apply16(st["t16"], *lk16).transpose(1, 2, 0))


def test_geometry():
    for w, h in ac.SIZES + [ac.FAST_SIZE, (ac.BIG_W, ac.BIG_H), (36, 1 << 19), (5792, 5792)]:
        assert amaze_render.geom(w, h) == (w, h)
    for w, h in [(34, 36), (36, 35), (38, 38), (37, 40), (32, 64), (0, 0), (-36, 36), (5796, 5796), (1 << 13, 1 << 12)]:
        with pytest.raises(ValueError):
            amaze_render.geom(w, h)
