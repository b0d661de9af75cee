"""Rendered frames at 16 bits, on the CPU (include/mlvfs_amd.h, "rendered frames at 16 bits"): the proof that the cases of
tests/deep_cases.py reach what they claim -- both sides of step 3d's rounding, both clamps, both ends of t, pixels where t16 >> 4 is not
the 8-bit routes' t, both matrix paths, a shaper that is not monotone, N = 0, 2, 3 and 65, every order and tie of the fractions -- and
that each of six wrong definitions changes some sample of them; the consequences the header states; shaper16_srgb pinned in integers;
the Python interface."""
import inspect
import itertools

import numpy as np
import pytest

from mlvfs_amd import demosaic, look, render, scale
from mlvfs_amd.mount import Mount

import deep_cases as dp
import look_cases as lc
import render_cases as rc

LOOKS = {name: (S, n, T) for name, S, n, T in dp.looks()}


def all_frames():
    """[(route, frame, parameters, size, look name)] of the half-size cases and of one size of each other route"""
    out = [(2, f, p, None, name) for batch, _, _, _, name in dp.half_cases() for f, p in batch]
    out += [(1, f, p, None, name) for batch, _, _, _, name in dp.full_cases(48, 8) for f, p in batch]
    out += [(0, f, p, (ow, oh), name) for ow, oh, batch, _, _, _, name in dp.scaled_cases(48, 6) for f, p in batch]
    return out


@pytest.fixture(scope="module")
def staged():
    return [(dp.stages(route, f, p, size), p, name) for route, f, p, size, name in all_frames()]


def test_the_frames_reach_both_sides_of_the_rounding_both_clamps_and_both_ends(staged):
    low = np.concatenate([((st["acc"] + 2048) & 4095).ravel() for st, _, _ in staged])
    assert (low == 4095).any() and (low == 0).any()
    acc = np.concatenate([st["acc"].ravel() for st, _, _ in staged])
    assert (acc < -2048).any() and (((acc + 2048) >> 12) > 65535).any()
    t = np.concatenate([st["t16"].ravel() for st, _, _ in staged])
    assert (t == 0).any() and (t == 65535).any() and ((t > 0) & (t < 65535)).any()
    assert t.min() >= 0 and t.max() <= 65535


def test_some_pixels_differ_from_the_8_bit_index(staged):
    """t16 >> 4 is not the 8-bit routes' t where acc's bits 12 .. 15 are all ones and bit 11 is set: the 8-bit rounding carries"""
    differ = sum(int(((st["t16"] >> 4) != st["t"]).sum()) for st, _, _ in staged)
    same = sum(int(((st["t16"] >> 4) == st["t"]).sum()) for st, _, _ in staged)
    assert differ > 0 and same > 0


def test_both_matrix_paths_occur(staged):
    fits = [demosaic.matrix_fits_32(p) for _, p, _ in staged]
    assert any(fits) and not all(fits)
    # the 32-bit form holds step 3d where it holds step 3: the largest sum with the smaller rounding term
    for _, p, _ in staged:
        if demosaic.matrix_fits_32(p):
            assert all(sum(abs(int(k)) for k in p[4 + 3 * i:7 + 3 * i]) * 65535 + 2048 < 1 << 31 for i in range(3))
    for route in (1, 0):                                         # and in the launches of the two kernels that choose between them
        cases = dp.full_cases(48, 8) if route else [c[2:] for c in dp.scaled_cases(48, 6)]
        assert any(len({demosaic.matrix_fits_32(p) for _, p in c[0]}) == 2 for c in cases)


def test_the_looks():
    assert sorted({n for _, _, n, _ in dp.looks()}) == [0, 2, 3, 17, 65] and set(dp.NS) <= {n for _, _, n, _ in dp.looks()}
    S = dp.case_shaper16()
    assert (np.diff(S.astype(np.int64)) < 0).any() and (np.diff(S.astype(np.int64)) > 0).any()
    assert S[:len(lc.U)].tolist() == lc.U
    used = {c[4] for c in dp.half_cases()}
    assert used == set(LOOKS), "every look runs in some half-size case"


@pytest.mark.parametrize("n", [2, 3, 65])
def test_the_triples_reach_every_order_and_every_tie(n):
    """look_cases' construction behind the 16-bit shaper: all six orders of three distinct fractions, every tie"""
    S, _, T = LOOKS[f"random{n}"]
    st = look.stages16(lc.case_triples(), S, n, T)
    f = st["f"]
    seen = set()
    for a, b, c in itertools.permutations(range(3)):
        if ((f[a] > f[b]) & (f[b] > f[c])).any():
            seen.add((a, b, c))
    assert len(seen) == 6
    for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
        assert ((f[a] == f[b]) & (f[b] > f[c])).any() and ((f[a] == f[b]) & (f[b] < f[c])).any()
    assert ((f[0] == f[1]) & (f[1] == f[2])).any()
    assert st["u"].min() == 0 and st["u"].max() == 65535 and st["i"].max() == n - 2 and st["i"].min() == 0
    # the tetrahedron is the 8-bit look's, word for word: the same v from the same shaper values
    S12 = np.zeros(4096, np.uint16)
    S12[:len(lc.U)] = lc.U
    assert np.array_equal(st["v"], look.stages(lc.case_triples(), S12, n, T)["v"])


@pytest.mark.parametrize("kind", dp.WRONG)
def test_a_wrong_definition_changes_some_sample(staged, kind):
    changed = 0
    for st, _, name in staged:
        S, n, T = LOOKS[name]
        if kind == "step4d" and n == 0:
            continue
        right = dp.file_bytes(render.tone16(st["t16"], (S, n, T)))
        changed += right != dp.wrong(kind, st, S, n, T)
    assert changed > 0
    # the plainest exposure of each: the linear file
    S, n, T = LOOKS["linear0"]
    hits = sum(dp.file_bytes(render.tone16(st["t16"], (S, n, T))) != dp.wrong(kind, st, S, n, T) for st, _, _ in staged)
    assert hits > 0, kind


def test_consequences():
    (f, p), = rc.batch(48, 6, 1, 2)
    st = render.stages(f, p)
    lin = render.render(f, p, look16=LOOKS["linear0"])
    assert lin.dtype == np.uint16 and lin.shape == (3, 24, 3) and np.array_equal(lin.transpose(2, 0, 1), st["t16"])
    assert (render.render(f, p, look16=LOOKS["const0"]) == 12345).all()
    for name in ("random3", "case0"):
        assert np.array_equal(scale.render(f, p, 24, 3, look16=LOOKS[name]), render.render(f, p, look16=LOOKS[name]))
    assert demosaic.render(f, p, look16=LOOKS["srgb17"]).shape == (6, 48, 3)
    with pytest.raises(ValueError):
        render.render(f, p, look=(look.shaper_srgb(), 2, look.identity(2)), look16=LOOKS["linear0"])
    # 8-bit calls are what they were
    assert render.render(f, p).dtype == np.uint8 and "t16" in st


def test_shaper16_srgb_without_floating_point():
    """round(65535 oetf(t / 65535)) in integers.  Below the knee S = round(12.92 t); above it u = S[t] is the rounding of
    65535 (1.055 x^(1 / 2.4) - 0.055) with x = t / 65535: u - 1/2 <= that < u + 1/2, which is, with 2.4 = 12 / 5, all terms scaled by 2000
    and both sides raised to the twelfth power, lo^12 65535^5 <= t^5 d^12 < hi^12 65535^5"""
    S = look.shaper16_srgb()
    assert S.dtype == np.uint16 and S.shape == (65536,) and S[0] == 0 and S[65535] == 65535
    d = 2110 * 65535
    for t in range(65536):
        u = int(S[t])
        if t <= 205:
            assert u == (1292 * t + 50) // 100, t
        else:
            lo, hi = (2 * u - 1) * 1000 + 110 * 65535, (2 * u + 1) * 1000 + 110 * 65535
            assert lo ** 12 * 65535 ** 5 <= t ** 5 * d ** 12 < hi ** 12 * 65535 ** 5, t


def test_the_other_shapers_and_the_image():
    assert np.array_equal(look.shaper16_linear(), np.arange(65536)) and np.array_equal(look.shaper16("linear"), look.shaper16_linear())
    lg = look.shaper16_log2(12)
    assert lg[0] == 0 and lg[65535] == 65535 and (np.diff(lg.astype(np.int64)) >= 0).all() and lg[16] == 0 and lg[17] > 0
    assert np.array_equal(look.shaper16("log2:12"), lg) and np.array_equal(look.shaper16("srgb"), look.shaper16_srgb())
    # twelve stops below white the 16-bit index still has 16 steps; the 12-bit one has one
    assert len(np.unique(lg[16:33])) == 17 and len(np.unique(look.shaper_log2(12)[1:3])) == 2
    for bad in ("gamma", "log2:0"):
        with pytest.raises(ValueError):
            look.shaper16(bad)
    S, n, T = LOOKS["random3"]
    img = look.image16(S, n, T)
    assert len(img) == 131072 + 8 * 27 and img[:131072] == S.astype("<u2").tobytes()
    e = np.frombuffer(img, "<u2", offset=131072).reshape(27, 4)
    assert np.array_equal(e[:, :3], T) and (e[:, 3] == 0).all()
    assert len(look.image16(S)) == 131072
    for args in ((S[:4096], 0, None), (S, 1, T), (S, 66, T), (S, 3, None), (S, 2, T)):
        with pytest.raises(ValueError):
            look.image16(*args)


def test_tiff_header_bits():
    h8, h16 = render.tiff_header(24, 3), render.tiff_header(24, 3, bits=16)
    assert h8 == render.tiff_header(24, 3, 8) and len(h16) == 256
    diff = [k for k in range(256) if h8[k] != h16[k]]
    # BitsPerSample's three shorts at 158, and StripByteCounts' value: entry 9 of the IFD, at 10 + 12 * 9 + 8
    assert set(diff) <= {158, 160, 162} | set(range(126, 130)) and {158, 160, 162} <= set(diff)
    assert int.from_bytes(h16[126:130], "little") == 6 * 24 * 3 and h16[158:164] == bytes([16, 0] * 3)
    with pytest.raises(ValueError):
        render.tiff_header(24, 3, bits=12)


def test_pil_reads_a_16_bit_file():
    Image = pytest.importorskip("PIL.Image")
    import io
    (f, p), = rc.batch(48, 6, 1, 0)
    px = render.render(f, p, look16=LOOKS["srgb17"])
    im = Image.open(io.BytesIO(render.tiff_header(24, 3, bits=16) + dp.file_bytes(px)))
    assert im.mode == "RGB" and im.size == (24, 3)
    assert np.array_equal(np.asarray(im), (px >> 8).astype(np.uint8))


def test_the_python_interface():
    for f in (render.render, demosaic.render, scale.render):
        assert inspect.signature(f).parameters["look16"].default is None
    assert inspect.signature(render.tiff_header).parameters["bits"].default == 8
    assert inspect.signature(Mount.rgb).parameters["look16"].default is None and inspect.signature(Mount.rgb_size).parameters["bits"].default == 8
    assert list(inspect.signature(look.Look16.__init__).parameters)[1:] == ["shaper16", "n", "table"]
    for name in ("apply16", "stages16", "image16", "shaper16_linear", "shaper16_srgb", "shaper16_log2"):
        assert callable(getattr(look, name))
