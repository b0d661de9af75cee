"""The cases of tests/resample_cases.py are not vacuous (no GPU): the weights of every pair of lengths used partition both ways; the
case set tells the definition of mlvfs_amd/resample.py from each wrong one by at least one output byte; spans straddle a strip seam,
a band seam and an output-row change inside a band of the plan that mlvfs_amd_test_resample_plan reports; a white frame reaches the
largest sum; the identity size is demosaic.render; a frame flat per CFA colour renders to the half-size pixel at every size; and
resample.fit is a brute-force search's answer and the library's."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import demosaic, lib, render, resample, scale

import demosaic_cases as dc
import resample_cases as rs

SMALL = [s for s in rs.SOURCES if s[0] * s[1] <= 4096]


@pytest.fixture(scope="module")
def lut():
    return render.srgb_lut12()


def plan(amd, w, h, ow, oh, nframes):
    out = np.zeros(8, np.int32)
    assert amd.mlvfs_amd_test_resample_plan(w, h, ow, oh, nframes, lib.ptr(out)) == 0, amd.mlvfs_amd_last_error()
    return dict(zip(("fast", "strip", "uo", "nstrips", "bo", "nbands", "band_rows", "rows"), out.tolist()))


def test_the_weights_partition_both_ways():
    pairs = {(w, ow) for w, h in rs.SOURCES if w <= 2048 for ow, _ in rs.out_sizes(w, h)} | {(h, oh) for w, h in rs.SOURCES for _, oh in rs.out_sizes(w, h)}
    pairs |= {(rs.BIG_W, 1920), (rs.BIG_W, 2560), (rs.BIG_H, 707), (rs.BIG_H, 943)}
    for n, n_out in sorted(pairs):
        wt = scale.weights(n, n_out)
        assert (wt.sum(axis=1) == n).all() and (wt.sum(axis=0) == n_out).all(), (n, n_out)
        lo, hi = scale.spans(n, n_out)
        if 2 * n_out >= n:
            assert (hi - lo).max() <= 2, (n, n_out)                          # at most three source pixels: what k_resample_x16 unrolls
        a = np.random.default_rng(n * 7 + n_out).integers(0, 65536, (2, n))
        assert np.array_equal(scale.average(a, n_out), (wt @ a.T).T // n + ((wt @ a.T).T % n + (n >> 1)) // n), (n, n_out)


@pytest.mark.parametrize("kind", rs.WRONG)
def test_the_cases_tell_the_definition_from_a_wrong_one(lut, kind):
    hits = 0
    for w, h in SMALL:
        for ow, oh, batch, _, _, _ in rs.dev_cases(w, h):
            for f, p in batch:
                hits += not np.array_equal(resample.render(f, p, ow, oh, lut), rs.wrong(kind, f, p, ow, oh, lut))
    assert hits > 0, kind


def test_the_plan_and_its_seams(amd):
    p = plan(amd, 528, 65, 527, 64, 1)
    assert p == dict(fast=1, strip=rs.STRIP, uo=495, nstrips=2, bo=32, nbands=2, band_rows=rs.BAND_ROWS, rows=rs.ROWS)
    assert plan(amd, 418, 267, 418, 267, 1)["fast"] == 0 and plan(amd, 32, 8, 15, 8, 1)["fast"] == 0 and plan(amd, 32, 8, 16, 1, 3)["fast"] == 1
    strip_seam = band_seam = row_change = many_bands = 0
    for w, h in rs.SOURCES:
        for ow, oh in rs.out_sizes(w, h):
            for n in (1, 3):
                p = plan(amd, w, h, ow, oh, n)
                assert p["fast"] == rs.takes_fast(w, ow)
                if not p["fast"]:
                    continue
                assert 1 <= p["uo"] <= ow and p["nstrips"] == -(-ow // p["uo"]) and 1 <= p["bo"] <= oh and p["nbands"] == -(-oh // p["bo"])
                # a strip's source columns fit the ring, and every one of its spans lies inside them
                for s in range(p["nstrips"]):
                    us0, us1 = s * p["uo"], min((s + 1) * p["uo"], ow)
                    x0, x1 = us0 * w // ow // 8 * 8, -(-(-(-us1 * w // ow)) // 8) * 8
                    assert x1 - x0 <= rs.STRIP and x1 <= w, (w, ow, s)
                    strip_seam += s > 0 and us0 * w % ow != 0                  # a source column shared by the spans at both sides
                for b in range(1, p["nbands"]):
                    band_seam += b * p["bo"] * h % oh != 0
                row_change += p["bo"] > 1 and any(v * h % oh for v in range(1, min(p["bo"], oh)))
                many_bands += p["nbands"] > 8
    assert strip_seam and band_seam and row_change and many_bands, (strip_seam, band_seam, row_change, many_bands)
    out = np.zeros(8, np.int32)
    for bad in ((3, 8, 1, 1, 1), (32, 8, 33, 8, 1), (32, 8, 32, 9, 1), (32, 8, 0, 1, 1), (65536, 4, 1, 1, 1), (8192, 4096, 1, 1, 1), (32, 8, 4, 4, 0)):
        assert amd.mlvfs_amd_test_resample_plan(*bad, lib.ptr(out)) == lib.ERR_ARG, bad
    assert amd.mlvfs_amd_test_resample_plan(32, 8, 4, 4, 1, None) == lib.ERR_ARG


@pytest.mark.parametrize("w,h", rs.WHITE, ids=lambda v: str(v))
def test_a_white_frame_reaches_the_largest_sum(w, h):
    for f, p, ow, oh, byte in rs.white_cases(w, h)[:4]:
        st = resample.stages(f, p, ow, oh)
        j = [k for k in range(3) if p[4 + k] == 1][0]                         # the probed channel
        assert (st["d"][j] == 65535).all() and (st["m"][j] == 65535).all()
        assert (resample.render(f, p, ow, oh, np.arange(4096) % 256) == byte).all()
    assert w * 65535 + (w >> 1) < 1 << 32 and (w < 65535 or w * 65535 == 65535 ** 2)


def test_the_identity_size_is_the_full_size_rendering(lut):
    for w, h in SMALL + [(96, 34)]:
        for f, p in dc.batch(w, h, 3, w):
            assert np.array_equal(resample.render(f, p, w, h, lut), demosaic.render(f, p, lut))


def test_a_flat_frame_renders_to_the_half_size_pixel(lut):
    for k, (w, h) in enumerate(SMALL):
        _, p = dc.param_set(k)
        f = dc.flat_frame(w, h, 900 + 50 * k, 3000, 1700)
        want = render.render(f[:2, :2], p, lut)[0, 0]
        for ow, oh in rs.out_sizes(w, h):
            assert (resample.render(f, p, ow, oh, lut) == want).all(), (w, h, ow, oh)


def test_this_is_not_the_scaled_route(lut):
    f, p = dc.batch(32, 8, 1, 2)[0]
    assert not np.array_equal(resample.render(f, p, 16, 4, lut), scale.render(f, p, 16, 4, lut))


def test_fit_equals_a_search_and_the_library(amd):
    assert resample.fit(3584, 1320, 1920, 1080) == (1920, 707)
    g = np.random.default_rng(18)
    a, b = C.c_int(0), C.c_int(0)
    for k in range(400):
        w, h = int(g.integers(4, 3000)), int(g.integers(4, 3000))
        bw, bh = int(g.integers(1, 4000)), int(g.integers(1, 4000))
        ow, oh = resample.fit(w, h, bw, bh)
        # the largest width that fits with its height rounded from the aspect, or the same the other way round
        if bw * h <= bh * w:
            cand = [(x, max(1, (2 * x * h + w) // (2 * w))) for x in range(1, w + 1) if x <= bw]
            best = max(cand)
        else:
            cand = [(max(1, (2 * y * w + h) // (2 * h)), y) for y in range(1, h + 1) if y <= bh]
            best = max(cand, key=lambda c: c[1])
        assert (ow, oh) == best and 1 <= ow <= w and 1 <= oh <= h and (ow <= bw or ow == 1) and (oh <= bh or oh == 1), (w, h, bw, bh)
        assert amd.mlvfs_amd_rgb_fit_full(w, h, bw, bh, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (ow, oh), (w, h, bw, bh)
    resample.geom(65535, 4, 65535, 4)
    for bad in ((3, 8), (8, 3), (65536, 4), (8192, 4096)):
        with pytest.raises(ValueError):
            resample.geom(*bad)
    for bad in ((0, 1), (33, 8), (32, 9)):
        with pytest.raises(ValueError):
            resample.geom(32, 8, *bad)
    with pytest.raises(ValueError):
        resample.fit(32, 8, 0, 5)
