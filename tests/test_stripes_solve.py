"""mlvfs_amd_stripes_solve (clip.cpp: stripes_solve, host code) against a plain restatement of stripes.c:218-245: which histograms are
solved, where the median bin lies for odd and even counts and at both ends of the histogram, and where the 0.998 / 1.002 decision
flips.  No GPU."""
import math

import numpy as np
import pytest

from mlvfs_amd import lib

ONE = 65536


def solve_restated(hist, num, frame_size, coeffs):
    """stripes.c:218-245 in Python ints and libm's pow.  hist: 8 dicts {bin: count}.  The running sum can first reach num / 2 only at
    bin 0 or at a bin that holds something, so only those are visited, in order."""
    co = [int(c) for c in coeffs]
    for j in range(8):
        if num[j] < frame_size // 128:
            continue
        t = 0
        for k in sorted(set(hist[j]) | {0}):
            t += hist[j].get(k, 0)
            if t >= num[j] // 2:
                co[j] = int(math.pow(2, (k - 32768) / 32768) * ONE)
                break
    co[0] = co[1] = ONE
    needed = 0
    for j in range(8):
        c = co[j] / ONE
        if c < 0.998 or c > 1.002:
            needed = 1
    return needed, co


def solve_lib(amd, hist, num, frame_size, coeffs):
    h = np.zeros((8, 65536), np.int32)
    for j in range(8):
        for k, n in hist[j].items():
            h[j, k] = n
    nn = np.array(num, np.int32)
    co = np.array(coeffs, np.int32)
    needed = amd.mlvfs_amd_stripes_solve(lib.ptr(h), lib.ptr(nn), frame_size, lib.ptr(co))
    return needed, [int(c) for c in co]


def check(amd, hist, num, frame_size, coeffs):
    want = solve_restated(hist, num, frame_size, coeffs)
    got = solve_lib(amd, hist, num, frame_size, coeffs)
    assert got == want, (hist, num, frame_size, coeffs)
    assert got[1][:2] == [ONE, ONE]
    return got


def same(h):
    return [dict(h) for _ in range(8)]


@pytest.mark.parametrize("start", [0, 70000])
@pytest.mark.parametrize("frame_size", [12800, 12927, 128, 255, 256])
def test_skip_threshold(amd, frame_size, start):
    """num one below, at and one above frame_size / 128 (integer division): below it the coefficient stays as it came in"""
    thr = frame_size // 128
    for n in (thr - 1, thr, thr + 1):
        if n < 0:
            continue
        needed, co = check(amd, same({33000: n} if n else {}), [n] * 8, frame_size, [start] * 8)
        solved = int(math.pow(2, ((33000 if n > 1 else 0) - 32768) / 32768) * ONE)     # num / 2 == 0 is reached at bin 0
        assert co[2:] == [start if n < thr else solved] * 6, (n, thr)
    # histograms on either side of the threshold in one call
    num = [thr + 1, thr - 1, thr, thr - 1, thr + 1, thr - 1, thr, thr + 7]
    needed, co = check(amd, [{32768 + 10 * j: n} for j, n in enumerate(num)], num, frame_size, [start] * 8)
    assert [c == start for c in co[2:]] == [n < thr for n in num[2:]]


@pytest.mark.parametrize("frame_size", [0, 1, 100, 127])
def test_small_frame_size_skips_nothing(amd, frame_size):
    """frame_size / 128 == 0: every histogram is solved, an empty one (num 0) at bin 0"""
    needed, co = check(amd, same({}), [0] * 8, frame_size, [70000] * 8)
    assert co[2:] == [ONE // 2] * 6 and needed == 1
    needed, co = check(amd, same({32768: 1}), [1] * 8, frame_size, [70000] * 8)          # 1 / 2 == 0: reached at bin 0 as well
    assert co[2:] == [ONE // 2] * 6
    needed, co = check(amd, same({32768: 2}), [2] * 8, frame_size, [70000] * 8)
    assert co[2:] == [ONE] * 6 and needed == 0


@pytest.mark.parametrize("n", [4, 5, 6, 7, 1000, 1001])
def test_odd_and_even_counts(amd, n):
    """t >= num / 2 with the integer quotient: one sample in each of two bins, the rest in a third"""
    hist = same({30000: 1, 33000: 1, 36000: n - 2})
    needed, co = check(amd, hist, [n] * 8, 128, [0] * 8)
    want_bin = 33000 if n // 2 == 2 else 36000
    assert co[2] == int(math.pow(2, (want_bin - 32768) / 32768) * ONE)
    half = same({32700: n // 2, 32800: n - n // 2})                                       # exactly num / 2 in the first bin: it is the median
    assert check(amd, half, [n] * 8, 128, [0] * 8)[1][2] == int(math.pow(2, -68 / 32768) * ONE)
    short = same({32700: n // 2 - 1, 32800: n - n // 2 + 1})
    assert check(amd, short, [n] * 8, 128, [0] * 8)[1][2] == int(math.pow(2, 32 / 32768) * ONE)


def test_medians_at_both_ends(amd):
    top = int(math.pow(2, 32767 / 32768) * ONE)
    for hist, want in (({0: 10}, ONE // 2), ({65535: 10}, top), ({0: 5, 65535: 5}, ONE // 2), ({0: 4, 65535: 6}, top),
                       ({0: 4, 1: 1, 65535: 5}, int(math.pow(2, -32767 / 32768) * ONE)),
                       ({0: 4, 65534: 1, 65535: 5}, int(math.pow(2, 32766 / 32768) * ONE))):
        needed, co = check(amd, same(hist), [10] * 8, 1280, [0] * 8)
        assert co[2:] == [want] * 6 and needed == 1, hist
    assert top == 131069 or top == 131070


def test_a_count_the_histogram_never_reaches_keeps_the_coefficient(amd):
    """num larger than twice the histogram's mass (not what the analysis produces): the loop ends without a median, as in the reference"""
    needed, co = check(amd, same({32768: 3}), [10] * 8, 1280, [70000] * 8)
    assert co[2:] == [70000] * 6 and needed == 1


def test_decision_flips_where_the_restatement_flips(amd):
    """single-bin histograms through bins 32768 +/- 110: 0.998 and 1.002 are crossed once each, at the restatement's bins"""
    flags = []
    for d in range(-110, 111):
        needed, co = check(amd, same({32768 + d: 10}), [10] * 8, 1280, [0] * 8)
        flags.append(needed)
        # one histogram alone decides, whichever it is
        for j in (2, 7):
            hist = same({32768: 10})
            hist[j] = {32768 + d: 10}
            assert check(amd, hist, [10] * 8, 1280, [0] * 8)[0] == needed
    assert flags[0] == flags[-1] == 1 and flags[110] == 0
    flips = [i - 110 for i in range(1, len(flags)) if flags[i] != flags[i - 1]]
    assert len(flips) == 2 and flips[0] < 0 < flips[1], flips
    # 0.998 * 65536 = 65404.9: bin -95 gives (int)65404.4 = 65404, below; bin -94 gives 65405.  1.002 * 65536 = 65667.1: bin 95 gives
    # (int)65667.8 = 65667, still inside; bin 96 gives 65669.
    assert flips == [-94, 96], flips
    # coefficients 0 and 1 never decide: they are set to one whatever their histograms say
    hist = same({32768: 10})
    hist[0] = hist[1] = {0: 10}
    assert check(amd, hist, [10] * 8, 1280, [0] * 8) == (0, [ONE] * 8)
