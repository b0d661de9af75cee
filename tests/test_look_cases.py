"""A look for the rendered frames, the part that needs no GPU: the cases of tests/look_cases.py reach what they claim
-- every order of the three fractions, every tie, the first and the last cell of each axis, both ends of u and v, both sides of a
rounding step in 4c and in 4d --, each of five wrong definitions changes some byte of them, ties have no order, the identity look gives
the plain rendering's bytes, and the .cube reader quantises exactly and refuses what it does not take."""
import itertools

import numpy as np
import pytest

from mlvfs_amd import demosaic, look, render, scale

import look_cases as lc
import render_cases as rc


@pytest.fixture(scope="module")
def staged():
    t = lc.case_triples()
    return t, {name: look.stages(t, S, n, T) for name, S, n, T in lc.looks()}


def test_the_cases_reach_every_order_tie_cell_and_end(staged):
    t, st = staged
    for n in lc.NS:
        s = st[f"random{n}"]
        f, i = s["f"], s["i"]
        if n > 2:                                                # at N = 2 there is one cell
            for c in range(3):
                assert (i[c] == 0).any() and (i[c] == n - 2).any(), (n, c)
        assert (i <= n - 2).all()
        orders = {tuple(o) for o in s["order"].T[(f[0] != f[1]) & (f[1] != f[2]) & (f[0] != f[2])].tolist()}
        assert orders == set(itertools.permutations(range(3))), (n, orders)
        for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):         # the pair a, b equal: above the third, and below it
            assert ((f[a] == f[b]) & (f[a] > f[c])).any() and ((f[a] == f[b]) & (f[a] < f[c])).any(), (n, a, b)
        assert ((f[0] == f[1]) & (f[1] == f[2]) & (f[0] > 0)).any() and (f == 0).all(axis=0).any(), n
        assert (s["u"] == 0).any() and (s["u"] == 65535).any()
        assert (s["w"].sum(axis=0) == 65536).all() and (s["w"] >= 0).all()
    assert (st["zero3"]["v"] == 0).all() and (st["zero3"]["out"] == 0).all()
    assert (st["white17"]["v"] == 65535).all() and (st["white17"]["out"] == 255).all()
    assert (st["allwhite5"]["u"] == 65535).all() and (st["allwhite5"]["v"] == 65535).all()


def test_the_cases_stand_on_both_sides_of_both_rounding_steps(staged):
    t, st = staged
    S, n, T = lc.look_of("edge2")
    s = st["edge2"]
    red_only = (t[1] == 0) & (t[2] == 0)                         # u_g = u_b = 0: the edge from T[0] to T[1]
    by_u = {int(u): (int(v_r), int(v_g), int(o_g)) for u, v_r, v_g, o_g in
            zip(s["u"][0][red_only], s["v"][0][red_only], s["v"][1][red_only], s["out"][1][red_only])}
    # 4c: sum w V = f_r, which is 32767 and 32768 -- the rounding term carries at the second only
    assert by_u[0x7FFF][0] == 0 and by_u[0x8000][0] == 1
    # 4d: v = 128 and 129 -> 0 and 1 (128 + 128 < 257 <= 129 + 128); v = 65406 and 65407 -> 254 and 255
    assert by_u[128][1:] == (128, 0) and by_u[129][1:] == (129, 1)
    assert by_u[65407][1:] == (65406, 254) and by_u[65408][1:] == (65407, 255)
    for name in (f"random{n}" for n in lc.NS):
        r = st[name]["v"] % 257                                  # and in the random tables v + 128 falls on both sides of a multiple
        assert ((r + 128) % 257 == 0).any() and ((r + 129) % 257 == 0).any(), name


@pytest.mark.parametrize("kind", lc.WRONG)
def test_each_wrong_definition_changes_a_byte_of_the_cases(kind):
    t = lc.case_triples()
    changed = {}
    for name, S, n, T in lc.looks():
        if name.startswith("random") or name == "edge2":
            changed[name] = int((lc.wrong(kind, t, S, n, T) != look.apply(t, S, n, T)).sum())
    assert sum(changed.values()) > 0, changed
    if kind != "shift8":                                         # v >> 8 and (v + 128) / 257 differ rarely, anything else at most N
        assert sum(v > 0 for v in changed.values()) >= len(lc.NS) - 1, changed


def test_ties_have_no_order(staged):
    t, st = staged
    for name, S, n, T in lc.looks():
        f = st[name]["f"]
        tie = (f[0] == f[1]) | (f[1] == f[2]) | (f[0] == f[2])
        assert tie.sum() >= 16
        for prefer in itertools.permutations(range(3)):
            s = look.stages(t[:, tie], S, n, T, prefer=prefer)
            assert np.array_equal(s["v"], st[name]["v"][:, tie]) and np.array_equal(s["out"], st[name]["out"][:, tie]), (name, prefer)
    # the two orders do differ in the vertices they read
    S, n, T = lc.look_of("random17")
    a, b = look.stages(t, S, n, T, prefer=(0, 1, 2))["order"], look.stages(t, S, n, T, prefer=(2, 1, 0))["order"]
    assert (a != b).any()


def test_the_identity_look_is_the_plain_rendering():
    lut, S = render.srgb_lut12(), look.shaper_srgb()
    assert S.dtype == np.uint16 and np.array_equal(S, 257 * lut.astype(np.int64))
    grey = np.tile(np.arange(4096, dtype=np.int64), (3, 1))
    rand = lc.random_triples(100000, 5)
    for n in lc.NS:
        T = look.identity(n)
        assert T.shape == (n ** 3, 3) and T[0].tolist() == [0, 0, 0] and T[-1].tolist() == [65535] * 3 and T[1].tolist() == [int(T[1][0]), 0, 0]
        for t in (grey, rand):
            s = look.stages(t, S, n, T)
            assert np.array_equal(s["out"], lut[t]), n
            assert np.abs(s["v"] - s["u"]).max() <= 1, n


def test_swapping_red_and_blue_of_the_table_shows():
    T = lc.random_table(5)
    t = lc.random_triples(100000, 6)
    a = look.apply(t, look.shaper_linear(), 5, T)
    b = look.apply(t, look.shaper_linear(), 5, T.reshape(5, 5, 5, 3).transpose(2, 1, 0, 3).reshape(-1, 3))
    assert (a != b).mean() > 0.9


def test_render_takes_a_look_at_all_three_sizes():
    (black, white), p = rc.param_set(2)
    f = rc.range_frame(48, 8, black, white, seed=3)
    S, n, T = lc.look_of("random17")
    for got, t in ((render.render(f, p, look=(S, n, T)), render.stages(f, p)["t"]),
                   (demosaic.render(f, p, look=(S, n, T)), demosaic.stages(f, p)["t"]),
                   (scale.render(f, p, 7, 3, look=(S, n, T)), scale.stages(f, p, 7, 3)["t"])):
        assert got.dtype == np.uint8 and np.array_equal(got, look.apply(t, S, n, T).transpose(1, 2, 0))
    ident = (look.shaper_srgb(), 3, look.identity(3))
    assert np.array_equal(render.render(f, p, look=ident), render.render(f, p))
    assert np.array_equal(demosaic.render(f, p, look=ident), demosaic.render(f, p))
    assert np.array_equal(scale.render(f, p, 7, 3, look=ident), scale.render(f, p, 7, 3))


def test_both_matrix_paths_meet_in_one_batch():
    """the frame cases' batches of 3 hold parameters that fit 32 bits and parameters that do not"""
    for w, h in lc.HALF_SIZES[2:3] + lc.FULL_SIZES[2:3]:
        fits = [demosaic.matrix_fits_32(p) for batch, *_ in lc.frame_cases(w, h) if len(batch) == 3 for _, p in batch]
        assert any(fits) and not all(fits)


def test_the_shapers():
    lin = look.shaper_linear()
    assert lin[0] == 0 and lin[4095] == 65535 and lin[1] == 16 and (np.diff(lin.astype(np.int64)) > 0).all()
    lg = look.shaper_log2(8)
    assert lg[4095] == 65535 and lg[0] == 0 and lg[15] == 0 and lg[16] > 0 and (np.diff(lg.astype(np.int64)) >= 0).all()   # 4095 / 256 = 15.996
    assert abs(int(lg[2048]) - 65535 * 7 // 8) <= 8                                           # one stop below white is 7 / 8 of the way
    assert np.array_equal(look.shaper("linear"), lin) and np.array_equal(look.shaper("log2:8"), lg) and np.array_equal(look.shaper("srgb"), look.shaper_srgb())
    for bad in ("gamma", "log2:", "log2:0", "log2:-3"):
        with pytest.raises(ValueError):
            look.shaper(bad)


HEAD = "LUT_3D_SIZE 2\n"
ROWS8 = "0 0 0\n1 0 0\n0 1 0\n1 1 0\n0 0 1\n1 0 1\n0 1 1\n1 1 1\n"


def test_read_cube_quantises_exactly(tmp_path):
    half_up = "0.5000152591"                                    # a little above 32768.5 / 65535 = 0.50001525902...
    rows = ["0.5 1 1.0000001", "-0.1 0 1e-5", "%s 0.25 0.75" % half_up, "0.3 0.7 0.9",
            "0.000007629510948348 2 -7", "0.99999 0.999993 1.0", "0.333333 0.666667 0.1", "0.0000076 0.0000077 0.9999924"]
    text = "# a comment\n\nTITLE \"two words\"\n" + HEAD + "DOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 1 1\n\n" + "\n".join(rows) + "\n# the end\n"
    path = tmp_path / "a.cube"
    path.write_text(text)
    n, T = look.read_cube(path)
    assert n == 2 and T.dtype == np.uint16 and T.shape == (8, 3)
    assert T.tolist() == [[32768, 65535, 65535],                # 32767.5 + 0.5 floors to 32768; above 1 clamps
                          [0, 0, 1],                             # below 0 clamps; 0.65535 + 0.5 -> 1
                          [32769, 16384, 49151],                 # 16383.75 + 0.5 -> 16384; 49151.25 + 0.5 -> 49151
                          [19661, 45875, 58982],                 # exactly on the .5 boundary (19660.5, 45874.5, 58981.5 + 0.5): up
                          [0, 65535, 0],                         # 0.49999999999999 / 65535 stays 0
                          [65534, 65535, 65535],                 # 65534.34 -> 65534; 65534.54 -> 65535
                          [21845, 43690, 6554],                  # 21844.98 and 43690.02 round; 6553.5 + 0.5 = 6554 exactly on the boundary
                          [0, 1, 65535]]                         # 0.498 -> 0, 0.5046 -> 1, 65534.502 -> 65535
    # a table written with ten digits reads back as it was, and the interpolation of the two is the same
    S, n17, T17 = lc.look_of("random17")
    assert look.parse_cube(lc.cube_text(17, T17))[1].tolist() == T17.tolist()
    assert look.parse_cube(lc.cube_text(3, look.identity(3)))[1].tolist() == look.identity(3).tolist()


@pytest.mark.parametrize("text", [
    "LUT_1D_SIZE 2\n0 0 0\n1 1 1\n",                            # a 1D table
    HEAD + "LUT_1D_SIZE 2\n" + ROWS8,
    HEAD + "DOMAIN_MIN 0 0 0.1\n" + ROWS8,                       # other domains
    HEAD + "DOMAIN_MAX 1 1 2\n" + ROWS8,
    HEAD + "DOMAIN_MAX 1 1\n" + ROWS8,
    HEAD + "LUT_3D_INPUT_RANGE 0 1\n" + ROWS8,                   # a keyword it does not know
    HEAD + ROWS8 + "1 1 1\n",                                    # a wrong count of rows
    HEAD + ROWS8[6:],
    ROWS8,                                                       # no size
    HEAD + HEAD + ROWS8,                                         # two sizes
    "LUT_3D_SIZE 1\n0 0 0\n", "LUT_3D_SIZE 66\n", "LUT_3D_SIZE 0\n", "LUT_3D_SIZE two\n", "LUT_3D_SIZE 2 2\n" + ROWS8,
    HEAD + ROWS8.replace("1 1 0", "1 1"),                        # a short row
    HEAD + ROWS8.replace("1 1 0", "1 1 0 0"),
    HEAD + ROWS8.replace("1 1 0", "1 x 0"),
    HEAD + ROWS8.replace("1 1 0", "1 1/2 0"),                    # decimals only
    HEAD + ROWS8.replace("1 1 0", "1 nan 0"),
    HEAD + ROWS8.replace("1 1 0", "1 0x1 0"),
    "",
])
def test_read_cube_refuses(tmp_path, text):
    path = tmp_path / "bad.cube"
    path.write_text(text)
    with pytest.raises(ValueError):
        look.read_cube(path)


def test_look_tuples_are_checked():
    S, n, T = lc.look_of("random3")
    for args in ((S[:-1], n, T), (S, n, T[:-1]), (S, 1, T), (S, 66, T), (S, 4, T)):
        with pytest.raises(ValueError):
            look.apply(np.zeros((3, 1), np.int64), *args)
    assert look.image(S, n, T)[:8192] == S.astype("<u2").tobytes() and len(look.image(S, n, T)) == 8192 + 8 * 27
    for bad in (1, 66):
        with pytest.raises(ValueError):
            look.identity(bad)
