"""The cases of tests/scale_cases.py reach what they claim, on the CPU: the weights are a partition, the running-sum form of
mlvfs_amd/scale.py is the weight matrix applied, the identity size is the half-size rendering, a constant stays constant, the rounding
cases tell the definition's rounding from every other, the seams of k_scale_x16 lie inside spans, the widest spans fill the 32 bits,
the multiplication the kernel divides with is exact, and fit() finds what a brute-force search finds."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import lib, render, scale

import render_cases as rc
import scale_cases as sc

PAIRS = sorted({(n_src, n_out) for w, h in sc.SOURCES + sc.MOUNT_SIZES for ow, oh in sc.out_sizes(w, h) for n_src, n_out in ((w // 2, ow), (h // 2, oh))})


def plan(amd, w, h, ow, oh, nframes=1):
    out = np.zeros(8, np.int32)
    assert amd.mlvfs_amd_test_scale_plan(w, h, ow, oh, nframes, lib.ptr(out)) == 0, amd.mlvfs_amd_last_error()
    return dict(zip(("fast", "chunk", "strip_max", "uo", "nstrips", "bo", "nbands", "band_rows"), (int(v) for v in out)))


@pytest.mark.parametrize("n_src,n_out", [p for p in PAIRS if p[0] <= 4096], ids=lambda v: str(v))
def test_weights_partition_both_ways(n_src, n_out):
    w = scale.weights(n_src, n_out)
    assert (w.sum(axis=1) == n_src).all() and (w.sum(axis=0) == n_out).all() and w.max() <= n_out
    lo, hi = scale.spans(n_src, n_out)
    for u in range(n_out):
        nz = np.flatnonzero(w[u])
        assert nz[0] == lo[u] and nz[-1] == hi[u] and len(nz) == hi[u] - lo[u] + 1, u          # contiguous
    a = np.random.default_rng(n_src * 7 + n_out).integers(0, 65536, (3, n_src))
    assert np.array_equal(scale.average(a, n_out), (a @ w.T + (n_src >> 1)) // n_src)


@pytest.mark.parametrize("n_src,n_out", [p for p in PAIRS if p[0] > 4096], ids=lambda v: str(v))
def test_weights_of_the_long_sides_by_their_spans(n_src, n_out):
    """the same without the matrix: the closed form of each weight, summed over the spans"""
    lo, hi = scale.spans(n_src, n_out)
    u = np.arange(n_out, dtype=np.int64)
    first = np.minimum((lo + 1) * n_out, (u + 1) * n_src) - u * n_src
    last = np.where(hi > lo, (u + 1) * n_src - hi * n_out, 0)
    assert (first > 0).all() and (last >= 0).all() and (first + last + np.maximum(hi - lo - 1, 0) * n_out == n_src).all()
    assert (lo[1:] >= hi[:-1]).all() and (lo[1:] <= hi[:-1] + 1).all() and lo[0] == 0 and hi[-1] == n_src - 1
    a = np.random.default_rng(n_src + n_out).integers(0, 65536, n_src)
    got = scale.average(a, n_out)
    for k in {0, n_out // 2, n_out - 1}:
        wk = np.maximum(0, np.minimum((np.arange(n_src) + 1) * n_out, (k + 1) * n_src) - np.maximum(np.arange(n_src) * n_out, k * n_src))
        assert got[k] == (int((wk * a).sum()) + (n_src >> 1)) // n_src


def test_identity_is_the_half_size_rendering_and_a_constant_stays():
    lut = render.srgb_lut12()
    for w, h in [s for s in sc.SOURCES if s[0] * s[1] < 1 << 16] + sc.MOUNT_SIZES:
        for f, p in rc.batch(w, h, 3):
            assert np.array_equal(scale.render(f, p, w // 2, h // 2, lut), render.render(f, p, lut)), (w, h)
        (black, white), p = rc.param_set(2)
        f = sc.constant_frame(w, h, (black + white) // 2)
        want = render.render(f, p, lut)[0, 0]
        assert want.min() > 0
        for ow, oh in sc.out_sizes(w, h):
            assert (scale.render(f, p, ow, oh, lut) == want).all(), (w, h, ow, oh)


def other_rounding(frame, p, ow, oh, term):
    """the rendering with another rounding term in both passes: term(d) in place of d >> 1"""
    n = render.stages(frame, p)["n"]

    def avg(a, n_out):
        d = a.shape[-1]
        return (a @ scale.weights(d, n_out).T + term(d)) // d
    m = avg(avg(n, ow).transpose(0, 2, 1), oh).transpose(0, 2, 1)
    K = p[4:13]
    acc = np.stack([sum(np.int64(K[3 * i + j]) * m[j] for j in range(3)) for i in range(3)])
    return render.srgb_lut12()[np.clip((acc + 32768) >> 16, 0, 4095)].transpose(1, 2, 0)


def test_rounding_cases_tell_the_roundings_apart():
    """every case gives its byte under the definition; truncation, rounding the half down and rounding up each miss some"""
    lut = render.srgb_lut12()
    assert lut[0] == 0 and lut[1] == 1
    cases = sc.rounding_cases() + sc.half_case(7) + sc.half_case(40000, 2)
    missed = {"floor": 0, "half down": 0, "ceil": 0}
    terms = {"floor": lambda d: 0, "half down": lambda d: (d - 1) >> 1, "ceil": lambda d: d - 1}
    forms = set()
    for f, p, ow, oh, byte in cases:
        got = scale.render(f, p, ow, oh, lut)
        assert got.shape == (oh, ow, 3) and (got == byte).all(), (f.shape, ow, oh, byte)
        assert (other_rounding(f, p, ow, oh, lambda d: d >> 1) == byte).all()
        for name, term in terms.items():
            missed[name] += int((other_rounding(f, p, ow, oh, term) != byte).any())
        forms.add(f.shape[1] % 16 == 0)
    assert all(v > 0 for v in missed.values()) and forms == {True, False}, missed
    kinds = {(d % 2, np.sign(2 * r - d)) for d, q, r, want in sc.ROUNDING}
    assert kinds >= {(0, 0), (0, -1), (0, 1), (1, -1), (1, 1)}                # the half itself, below and above; an odd divisor has no half
    for d, q, r, want in sc.ROUNDING:
        assert want == (2 * (q * d + r) + d) // (2 * d)                        # round half up, in exact arithmetic
    a = sc.half_case(7)
    assert scale.stages(a[0][0], a[0][1], 8, 1)["m"][0].tolist() == [[8] * 8]


def test_white_cases_hold_the_largest_sum():
    for w, h in ((131070, 2), (131056, 2), (2, 131070)):
        for f, p, ow, oh, byte in sc.white_cases(w, h):
            st = scale.stages(f, p, ow, oh)
            j = [k for k in range(3) if p[4 + k] == 1 and st["n"][k].min() == 65535][0]
            assert st["m"][j, 0, 0] == 65535 and (scale.render(f, p, ow, oh) == byte).all()
            short = np.array(f)
            short[(0, 0, 1)[j], (0, 1, 1)[j]] = 65533                          # one pixel of channel j two below (both greens for j = 1)
            short[(0, 1, 1)[j], (0, 0, 1)[j]] = 65533
            assert scale.stages(short, p, ow, oh)["m"][j, 0, 0] == 65534 and (scale.render(short, p, ow, oh) == 0).all()
    assert (1 << 32) - (1 << 18) < 65535 * 65535 + (65535 >> 1) < 1 << 32
    # and the random batches at the widest identity come close to it: a weight of W' on a pixel near the top
    w, h = 131056, 2
    assert max(int(render.stages(f, p)["n"].max()) for f, p in rc.batch(w, h, 3)) * (w // 2) > (1 << 32) - (1 << 20)


def test_constants_and_seams_of_the_fast_form(amd):
    p = plan(amd, 4112, 8, 2055, 3)
    assert (p["chunk"], p["strip_max"], p["band_rows"]) == (sc.CHUNK, sc.STRIP, sc.BAND_ROWS) and p["fast"] == 1
    assert plan(amd, 418, 267, 7, 5)["fast"] == 0
    # strips: the last column of one and the first of the next share a source column
    assert p["nstrips"] >= 2
    lo, hi = scale.spans(2056, 2055)
    assert hi[p["uo"] - 1] == lo[p["uo"]]
    assert plan(amd, 4112, 8, 2056, 4)["nstrips"] >= 2                         # the identity too
    # bands of several output rows, several of them, and a source row that two bands read
    for ow, oh in ((8, 299), (8, 150), (7, 5)):
        p = plan(amd, 16, 600, ow, oh)
        assert p["nbands"] >= 2 and (p["bo"] >= 2 or oh == 5), (ow, oh, p)
    p = plan(amd, 16, 600, 8, 299)
    lo, hi = scale.spans(300, 299)
    assert any(hi[v - 1] == lo[v] for v in range(p["bo"], 299, p["bo"]))        # across a seam
    assert any(hi[v - 1] == lo[v] for v in range(1, p["bo"]))                   # and inside a band: the carry from one output row to the next
    p = plan(amd, 96, 34, 47, 16)
    assert p["bo"] >= 2
    # a single column wider than a step stages: a row of many chunks
    for ow in (1, 7):
        p = plan(amd, 131056, 2, ow, 1)
        assert p["uo"] == 1 and 65528 // ow > 8 * sc.CHUNK
    # every strip's source span fits one chunk wherever a column's does
    for w, h in sc.SOURCES + [(sc.BIG_W, sc.BIG_H)]:
        if w % 16:
            continue
        sizes = sc.out_sizes(w, h) + ([(1280, 472), (448, 165), (160, 59)] if w == sc.BIG_W else [])
        for ow, oh in sizes:
            for nframes in (1, 3, 8):
                p = plan(amd, w, h, ow, oh, nframes)
                pw = w // 2
                assert 1 <= p["uo"] <= min(sc.STRIP, ow) and p["nstrips"] == -(-ow // p["uo"]) and p["nbands"] == -(-oh // p["bo"]) and 1 <= p["bo"] <= oh
                if p["uo"] > 1:
                    for s in range(p["nstrips"]):
                        us0, us1 = s * p["uo"], min((s + 1) * p["uo"], ow)
                        assert (us1 * pw - 1) // ow + 1 - (us0 * pw // ow & ~3) <= sc.CHUNK, (w, h, ow, oh, s)


def test_the_division_by_multiplication_is_exact(amd):
    """floor(n / d) for every divisor a frame can have, at the numerators where a wrong multiplier or shift shows first: around every
    multiple of d near the ends of the 32 bits, the largest sums the definition has, and random ones"""
    g = np.random.default_rng(11)
    top = (1 << 32) - 1
    out = np.zeros(1 << 12, np.uint32)
    for d in list(range(1, 65536, 7)) + [1, 2, 3, 255, 256, 257, 32767, 32768, 32769, 65521, 65528, 65534, 65535] + list(range(65000, 65536)):
        k = np.concatenate([np.arange(1, 40), top // d - np.arange(0, 40), g.integers(1, top // d + 1, 200)]).astype(np.int64)
        k = k[(k >= 1) & (k <= top // d)]
        n = np.concatenate([k * d - 1, k * d, k * d + d - 1, [0, top, 65535 * 65535 + (d >> 1), min(d * 65535 + (d >> 1), top)], g.integers(0, top + 1, 200)])
        n = np.clip(n, 0, top).astype(np.uint32)
        assert amd.mlvfs_amd_test_scale_div(d, len(n), lib.ptr(n), lib.ptr(out)) == 0
        assert np.array_equal(out[:len(n)], n // np.uint32(d)), d
    assert amd.mlvfs_amd_test_scale_div(0, 1, lib.ptr(out), lib.ptr(out)) == lib.ERR_ARG


def test_fit_is_the_largest_size_in_the_box(amd):
    """against a search over all sizes of the box: among the sizes inside the box and the frame, at the rounded aspect of the side
    that limits, none is larger; the library and scale.fit agree"""
    g = np.random.default_rng(5)
    for k in range(400):
        w, h = int(g.integers(2, 400)), int(g.integers(2, 400))
        bw, bh = (int(g.integers(1, 260)), int(g.integers(1, 260))) if k % 8 else (int(g.integers(150, 500)), int(g.integers(150, 500)))
        pw, ph = w // 2, h // 2
        ow, oh = scale.fit(w, h, bw, bh)
        a, b = C.c_int(-7), C.c_int(-7)
        assert amd.mlvfs_amd_rgb_fit(w, h, bw, bh, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (ow, oh), (w, h, bw, bh)
        assert 1 <= ow <= min(bw, pw) and 1 <= oh <= min(bh, ph)
        # brute force: every size (x, y) in the box whose other side is the rounded aspect of the first (at least 1)
        best = (0, 0)
        for x in range(1, min(bw, pw) + 1):
            y = max(1, (2 * x * ph + pw) // (2 * pw))
            if y <= min(bh, ph) and x * y >= best[0] * best[1]:
                best = (x, y)
        alt = (0, 0)
        for y in range(1, min(bh, ph) + 1):
            x = max(1, (2 * y * pw + ph) // (2 * ph))
            if x <= min(bw, pw) and x * y >= alt[0] * alt[1]:
                alt = (x, y)
        if bw >= pw and bh >= ph:
            assert (ow, oh) == (pw, ph)
        elif bw * ph <= bh * pw:
            assert (ow, oh) == best, (w, h, bw, bh, ow, oh, best)
        else:
            assert (ow, oh) == alt, (w, h, bw, bh, ow, oh, alt)
