"""Flat fields, the part that needs no GPU and no library: the cases of tests/flat_cases.py really reach every boundary of the
definition -- the gain cap, s = 1, both divisions exactly half way and just below, floor against truncation, both
clamps, products beyond 32 bits, channel sums beyond 32 bits, the constant-flat identity -- and the pre-corrected clips really differ
from their sources.  The library's host code: tests/test_flat_host.py; the GPU side: tests/test_gpu_flat.py."""
import numpy as np
import pytest

import dark_cases as dc
import flat_cases as fc


def planes():
    out = [(w, h, 14, dc.clip_black(14), fc.flat_plane(w, h)) for (w, h) in fc.HOST_GEOMETRIES + fc.GPU_GAIN_GEOMETRIES]
    out.append((640, 480, 16, 0, fc.overflow_plane()))
    return out


def test_the_oracle_is_the_definition_pixel_by_pixel():
    """gains() and apply() against the formulas written out with Python's own integers"""
    F, black_f = fc.flat_plane(5, 4), dc.clip_black(14)
    g = fc.gains(F, black_f)
    sums, counts = [0] * 4, [0] * 4
    for y in range(4):
        for x in range(5):
            sums[(y & 1) * 2 + (x & 1)] += max(int(F[y, x]) - black_f, 1)
            counts[(y & 1) * 2 + (x & 1)] += 1
    M = [(t + n // 2) // n for t, n in zip(sums, counts)]
    assert M == fc.channel_means(F, black_f)
    rng = np.random.default_rng(1)
    px = rng.integers(0, 1 << 14, (4, 5)).astype(np.uint16)
    out = fc.apply(px, g, 2048, 14)
    for y in range(4):
        for x in range(5):
            s = max(int(F[y, x]) - black_f, 1)
            assert int(g[y, x]) == min((M[(y & 1) * 2 + (x & 1)] * 16384 + s // 2) // s, 65535)
            v = 2048 + ((int(px[y, x]) - 2048) * int(g[y, x]) + 8192) // 16384             # Python's // floors
            assert int(out[y, x]) == min(max(v, 0), 16383)


def test_the_planes_reach_the_cap_s_of_1_and_both_roundings_of_both_divisions():
    seen = {}
    for w, h, bpp, black_f, F in planes():
        k = fc.rounding_classes(F, black_f)
        if w * h >= 16:
            assert k["cap"] > 0 and k["at_black"] > 0, (w, h, k)
            assert k["below_black"] > 0 or black_f == 0, (w, h, k)
        for name, v in k.items():
            seen[name] = seen.get(name, 0) + v
        if w * h >= 64:
            assert k["gain_below_half"] > 0 and k["mean_below_half"] > 0, (w, h, k)
            assert k["mean_half"] > 0 or fc.channel_sums(F, black_f)[1][0] % 2, (w, h, k)      # (an odd n_c has no exact half)
        g = fc.gains(F, black_f)
        assert g.dtype == np.uint16 and g.shape == (h, w)
        M = np.array(fc.channel_means(F, black_f))[fc.channels(h, w)]
        assert ((g == 65535) >= ((F <= black_f) & (M >= 4))).all()          # s = 1 meets the cap once M * 16384 > 65535
    assert all(seen[name] > 0 for name in ("cap", "at_black", "below_black", "gain_half", "gain_below_half", "mean_half", "mean_below_half",
                                           "sum_over_32_bits")), seen
    # where the roundings sit they decide the result: exactly half way goes up, the largest fraction below goes down
    for w, h, bpp, black_f, F in planes():
        s, c = fc.signal(F, black_f), fc.channels(h, w)
        M = np.array(fc.channel_means(F, black_f), np.int64)[c]
        r, g = (M * fc.ONE) % s, fc.gains(F, black_f).astype(np.int64)
        half, below = (2 * r == s) & (g < 65535), ((2 * r + 1 == s) | (2 * r + 2 == s)) & (g < 65535)
        assert (g[half] == (M * fc.ONE)[half] // s[half] + 1).all() and (g[below] == (M * fc.ONE)[below] // s[below]).all()


def test_the_overflow_plane_needs_64_bit_sums():
    F = fc.overflow_plane()
    sums, counts = fc.channel_sums(F, 0)
    assert F.shape == (480, 640) and counts == [76800] * 4 and max(sums) >= 1 << 32
    wrapped = [(t % (1 << 32) + n // 2) // n for t, n in zip(sums, counts)]
    assert wrapped != fc.channel_means(F, 0)                               # 32-bit sums give another plane


def test_a_constant_flat_is_the_identity():
    rng = np.random.default_rng(2)
    for w, h in ((2, 2), (3, 3), (1, 8), (30, 10)):
        for value, black_f in ((5000, 2048), (2048, 2048), (100, 2048), (65535, 0)):
            g = fc.gains(fc.constant_plane(w, h, value), black_f)
            assert (g == fc.ONE).all(), (w, h, value)
            for bpp in (10, 12, 14, 16):
                px = rng.integers(0, 1 << bpp, (h, w)).astype(np.uint16)
                assert np.array_equal(fc.apply(px, g, dc.clip_black(bpp), bpp), px)


@pytest.mark.parametrize("w,h,bpp,n,dark", fc.APPLY_CASES, ids=lambda v: str(v))
def test_every_apply_case_clamps_both_ways_and_floors(w, h, bpp, n, dark):
    c = fc.apply_case(w, h, bpp, n, dark)
    top, black, g = (1 << bpp) - 1, c["black"], c["gain"].astype(np.int64)
    assert c["F"].shape == (h, w) and len(c["frames"]) == n
    if w * h == 4:                                                          # one pixel per channel: M_c = s, every gain is 1.0
        assert (g == fc.ONE).all() and all(np.array_equal(wnt, dc.subtract(f, c["dark"], c["black_d"], bpp) if dark else f)
                                           for f, wnt in zip(c["frames"], c["want"]))
        return
    assert int(g[-1, -1]) == 65535
    for f, want in zip(c["frames"], c["want"]):
        src = dc.subtract(f, c["dark"], c["black_d"], bpp) if dark else f
        prod = (src.astype(np.int64) - black) * g
        v = black + (prod + 8192) // fc.ONE
        assert (v < 0).any() and (v > top).any() and ((v >= 0) & (v <= top)).any()
        assert int(want.min()) == 0 and int(want.max()) == top and int(f.max()) <= top
        assert (prod < 0).any()
        if w * h >= 16:
            assert not np.array_equal(fc.truncated(src, c["gain"], black, bpp), want)         # floor, not truncation
        if bpp == 16:
            assert int(prod.max()) >= 1 << 31                                # 32-bit products are not enough
        else:
            assert int(np.abs(prod).max()) + 8192 < 1 << 31
        if dark:
            assert not np.array_equal(want, fc.apply(f, c["gain"], black, bpp))               # the dark frame matters
    assert {b for _, _, b, _, _ in fc.APPLY_CASES} == {10, 12, 14, 16}


def test_a_ten_bit_case_clamps_at_zero_under_a_low_black_level():
    c = fc.apply_case(30, 10, 10, 1)
    assert c["black"] == 128
    v = c["black"] + ((c["frames"][0].astype(np.int64) - c["black"]) * c["gain"].astype(np.int64) + 8192) // fc.ONE
    assert int((v < 0).sum()) >= 3


def test_the_apply_rounding_sits_on_its_boundary_somewhere():
    """(px - black) * gain + 8192 a multiple of 16384, i.e. the quotient exactly half way, and one below it"""
    frames, F, _, _ = fc.clip_case("plain", n=2)
    g = fc.gains(F, fc.BLACK).astype(np.int64)
    t = (frames[0].astype(np.int64) - fc.BLACK) * g
    assert ((t % fc.ONE == 8192) & (g != fc.ONE)).any() and (t % fc.ONE == 8191).any()


@pytest.mark.parametrize("kind,dark", [("plain", False), ("plain", True), ("dual_iso", False)])
def test_every_clip_case_clamps_both_ways_and_the_corrected_clip_differs(oracle, kind, dark):
    frames, F, plane_d, pre = fc.clip_case(kind, dark=dark)
    g = fc.gains(F, fc.BLACK)
    assert int(g.max()) == 65535 and 1.3 < g[0, 0] / fc.ONE < 2.5 and abs(g[fc.H // 2, fc.W // 2] / fc.ONE - 1) < 0.35
    for f, p in zip(frames, pre):
        assert int(p.max()) == 16383 and int(p.min()) == 0 and p[0, 0] != 0
        for (y, x) in dc.TOP_AT:
            assert p[y, x] == 16383
        for (y, x) in dc.ZERO_AT:
            assert p[y, x] == 0
        assert (f != p).mean() > 0.5                                        # the correction changes most of the frame
    a, b = oracle.chroma_smooth(frames[0], fc.BLACK, 5), oracle.chroma_smooth(pre[0], fc.BLACK, 5)
    assert not np.array_equal(a, b)
    assert not np.array_equal(b, fc.apply(a, g, fc.BLACK, 14))              # nor is it a correction behind the stages
    if dark:
        assert not np.array_equal(pre[0], fc.apply(frames[0], g, fc.BLACK, 14))
        assert not np.array_equal(pre[0], dc.subtract(fc.apply(frames[0], g, fc.BLACK, 14), plane_d, fc.BLACK, 14))      # dark first


@pytest.mark.parametrize("w,h,bpp", fc.DEPTH_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dark", [False, True])
def test_every_depth_case_differs_and_takes_the_path_it_is_there_for(w, h, bpp, dark):
    frames, F, plane_d, black_d, pre = fc.depth_case(w, h, bpp, dark)
    top = (1 << bpp) - 1
    for f, p in zip(frames, pre):
        assert int(f.max()) <= top and int(p.max()) == top and int(p.min()) == 0 and (f != p).mean() > 0.5
    assert (w * h * bpp) % 16 == 0
    fused = bpp in (10, 12, 14) and (w * h) % 16 == 0                       # launch_cal_unpack's choice (csrc/k_cal.hip)
    assert fused == ((w, h, bpp) in [(dc.W, dc.H, 12), (dc.W, dc.H, 10)])
