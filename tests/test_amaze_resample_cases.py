"""Resampled rendered frames demosaiced by AMaZE, on the CPU: the definition of mlvfs_amd/amaze_resample.py with the checker's AMaZE on
the cases of tests/amaze_resample_cases.py.  The identity size is the AMaZE full-size rendering; the cases tell the definition from six
wrong ones; the plan of the fast form (mlvfs_amd_test_amz_resample_plan, host code) has the seams the cases are there for, and both
kernel forms are taken; the geometry."""
import numpy as np
import pytest

from mlvfs_amd import amaze_render, amaze_resample, lib, look, render, resample

import amaze_resample_cases as arc


@pytest.fixture(scope="module")
def staged(oracle):
    """the AMaZE stages of every case, computed once: [(label, w, h, frame, parameters, stages)]"""
    return [(label, w, h, f, p, amaze_render.stages(f, p, oracle.amaze_demosaic)) for w, h, f, p, label in arc.cases()]


def test_the_case_set(staged):
    assert len(staged) == 38 and len({s[0] for s in staged}) == 38
    assert {(w, h) for _, w, h, _, _, _ in staged} == set(arc.SOURCES)
    for w, h in arc.SOURCES:
        sizes = arc.out_sizes(w, h)
        assert sizes[0] == (w, h) and len(sizes) == len(set(sizes)) >= 8 and (1, 1) in sizes and (w, 1) in sizes and (1, h) in sizes
        for ow, oh in sizes:
            assert amaze_resample.geom(w, h, ow, oh) == (w, h)


def test_the_identity_size_is_the_full_size_rendering(oracle, staged):
    import deep_cases as dc
    import look_cases as lc
    lk, lk16 = lc.look_of("random17"), dc.look_of("random3")
    for label, w, h, f, p, st in staged:
        rs = amaze_resample.stages(f, p, oracle.amaze_demosaic, w, h, source=st["n"])
        assert np.array_equal(rs["m"], st["n"]) and np.array_equal(rs["t"], st["t"]) and np.array_equal(rs["t16"], st["t16"]), label
    label, w, h, f, p, st = staged[4]
    A = oracle.amaze_demosaic
    assert np.array_equal(amaze_resample.render(f, p, A, w, h), amaze_render.render(f, p, A))
    assert np.array_equal(amaze_resample.render(f, p, A, w, h, look=lk), amaze_render.render(f, p, A, look=lk))
    assert np.array_equal(amaze_resample.render(f, p, A, w, h, look16=lk16), amaze_render.render(f, p, A, look16=lk16))


def test_the_definition_composes_the_two(oracle, staged):
    """resample.stages on the AMaZE rendering's n: with and without the source handed in"""
    label, w, h, f, p, st = staged[7]
    ow, oh = arc.out_sizes(w, h)[3]
    a = amaze_resample.stages(f, p, oracle.amaze_demosaic, ow, oh)
    b = resample.stages(f, p, ow, oh, source=st["n"])
    assert all(np.array_equal(a[k], b[k]) for k in ("d", "hd", "m", "acc", "t", "t16"))
    assert a["m"].shape == (3, oh, ow) and a["hd"].shape == (3, h, ow)
    rgb = amaze_resample.render(f, p, oracle.amaze_demosaic, ow, oh, source=st["n"])
    assert rgb.shape == (oh, ow, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, render.tone(a["t"]))


@pytest.mark.parametrize("kind", arc.VARIANTS)
def test_the_cases_tell_a_wrong_definition_apart(staged, kind):
    """every case, by at least one value of m at its non-identity sizes taken together; and the 16-bit index follows"""
    total = 0
    for label, w, h, f, p, st in staged:
        shown = shown16 = 0
        for ow, oh in arc.out_sizes(w, h)[1:]:
            m = resample.stages(f, p, ow, oh, source=st["n"])["m"]
            wrong = arc.variant_m(kind, f, p, st, ow, oh)
            assert wrong.shape == m.shape
            shown += int((wrong != m).sum())
            shown16 += int((arc.matrix(p, wrong)[1] != arc.matrix(p, m)[1]).sum())
        assert shown >= 1 and shown16 >= 1, (kind, label, shown, shown16)
        total += shown
    print(kind, total)


def test_the_plan_has_the_seams_and_both_forms_are_taken(amd):
    """a source column shared by two strips, a source row shared by two bands, a source row shared by two output rows inside a band;
    the fast form's width rule is W % 8 == 0 with 2 ow >= W"""
    fast = generic = strip_seam = band_seam = row_change = 0
    for w, h in arc.SOURCES:
        for ow, oh in arc.out_sizes(w, h):
            pl = arc.plan(amd, w, h, ow, oh)
            assert pl["fast"] == int(arc.takes_fast(w, ow)), (w, h, ow, oh)
            assert (pl["strip"], pl["rows"]) == (512, 4)
            if not pl["fast"]:
                assert (pl["uo"], pl["nstrips"], pl["bo"], pl["nbands"]) == (0, 0, 0, 0)
                generic += 1
                continue
            fast += 1
            uo, bo = pl["uo"], pl["bo"]
            assert 1 <= uo <= ow and pl["nstrips"] == -(-ow // uo) and 1 <= bo <= oh and pl["nbands"] == -(-oh // bo)
            for k in range(pl["nstrips"]):                       # a strip's source columns, rounded to 8 both ways, fit the strip
                us0, us1 = k * uo, min((k + 1) * uo, ow)
                x0, x1 = us0 * w // ow // 8 * 8, -(-(-(-us1 * w // ow)) // 8) * 8
                assert x1 - x0 <= pl["strip"] and x1 <= w, (w, h, ow, oh, k)
                for u in range(us0, us1):                        # and a span is at most three pixels
                    assert (((u + 1) * w - 1) // ow) - (u * w // ow) <= 2
            strip_seam += any((k * uo * w) % ow for k in range(1, pl["nstrips"]))
            band_seam += any((k * bo * h) % oh for k in range(1, pl["nbands"]))
            row_change += any((v * h) % oh for v in range(1, oh) if v % bo)
    assert fast >= 20 and generic >= 20 and strip_seam >= 2 and band_seam >= 4 and row_change >= 8, (fast, generic, strip_seam, band_seam, row_change)
    assert arc.plan(amd, 528, 36, 528, 36)["nstrips"] == 2 and arc.plan(amd, 48, 70, 48, 70)["nbands"] == 3 and arc.plan(amd, 48, 600, 47, 599)["nbands"] >= 10
    assert arc.plan(amd, 40, 38, 40, 38)["fast"] == 1 and arc.plan(amd, 36, 36, 36, 36)["fast"] == 0 and arc.plan(amd, 48, 37, 23, 37)["fast"] == 0
    big = arc.plan(amd, arc.BIG_W, arc.BIG_H, *arc.BIG_SIZE, nframes=8)
    assert (big["fast"], big["uo"], big["nstrips"]) == (1, 256, 8) and big["nstrips"] * big["nbands"] <= 128


def test_geometry():
    for w, h in arc.SOURCES + [(arc.BIG_W, arc.BIG_H), (36, 65535), (65532, 500)]:
        assert amaze_resample.geom(w, h) == (w, h) and amaze_resample.geom(w, h, w, h) == (w, h) and amaze_resample.geom(w, h, 1, 1) == (w, h)
    for w, h in [(34, 36), (36, 35), (38, 38), (0, 0), (-36, 36), (5796, 5796), (36, 65536), (36, 1 << 19), (65536, 36), (8, 8)]:
        with pytest.raises(ValueError):
            amaze_resample.geom(w, h)
    for ow, oh in [(0, 1), (1, 0), (49, 37), (48, 38), (-1, 5), (1 << 20, 1)]:
        with pytest.raises(ValueError):
            amaze_resample.geom(48, 37, ow, oh)
    assert amaze_resample.fit(3584, 1320, 1920, 1080) == (1920, 707) == resample.fit(3584, 1320, 1920, 1080)
    assert amaze_resample.fit(1736, 976, 1280, 720) == (1280, 720)
    with pytest.raises(ValueError):
        amaze_resample.fit(34, 36, 10, 10)
