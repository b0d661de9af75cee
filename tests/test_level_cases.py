"""The level and gain cases of tests/level_cases.py are what they are there for -- checked with the oracle and the library's host-side
plan (mlvfs_amd_test_frame_plan), without a GPU: the level table's coverage, the pixel populations of every frame (below, at, 1..64,
65..255 and more than 255 above black, wherever the depth has such values; under a tenth saturated), stripes that change pixels,
clamp cases in which a hundredth of the pixels and more ends at white, one-unit-column sets with one unit column per dword, and the
admission rule of the streaming kernels over every black level 0 .. 16384 and one step outside.  Whoever moves a threshold or a
generator learns here which case has become vacuous."""
import numpy as np
import pytest

import level_cases as LC
import stream_shapes as S

LONG = 4000          # frames of 608x250: far beyond what a streaming kernel asks of a launch on 256 CUs


def test_level_table_covers_blacks_and_white_kinds():
    assert {b for b, _, _ in LC.LEVELS} == set(LC.BLACKS) and len(set(LC.LEVELS)) == len(LC.LEVELS)
    for b in LC.BLACKS:
        assert len({k for bb, k, _ in LC.LEVELS if bb == b}) >= 2, b
    for kind in LC.WHITE_KINDS:
        assert len({b for b, k, _ in LC.LEVELS if k == kind}) >= 3, kind
    for b, kind, form in LC.LEVELS:
        assert form == ("generic" if kind == "outer" else "packed"), (b, kind)
        assert (LC.white_of(b, kind) == b + 64) == (kind == "outer")            # no absolute white that is an edge in disguise
    assert LC.white_of(0, "above") > 16383
    both = [{LC.level_geometry(i) for i, c in enumerate(LC.LEVELS) if c[2] == form} for form in ("packed", "generic")]
    assert all(g == set(LC.GEOMETRIES) for g in both), "either form on either geometry"


@pytest.mark.parametrize("black", LC.BLACKS)
def test_footage_has_every_population(black):
    for w, h in LC.GEOMETRIES:
        for kinds in (LC.KINDS[2], LC.KINDS[5]):
            for kind, f in zip(kinds, LC.footage(kinds, w, h, black)):
                assert f.shape == (h, w) and f.dtype == np.uint16 and int(f.max()) <= 16383
                pop, room = LC.populations(f, black), LC.room_for(black)
                for name in pop:
                    assert (pop[name] >= 4) if room[name] else (pop[name] == 0), (kind, w, h, name, pop)
                if black not in LC.SATURATED_BLACKS:
                    assert (f == 16383).mean() < 0.10, (kind, w, h, float((f == 16383).mean()))
    if black == 16319:
        assert int(LC.footage(LC.KINDS[2], 608, 250, black)[0].max()) <= black + 64
    if black == 16384:
        assert all(int(f.max()) < black for f in LC.footage(LC.KINDS[2], 608, 250, black))


def changed_by_stripes(oracle, frames, black, white, coeffs):
    """(pixels the epilogue changes, pixels it moves to white, pixels) over a clip"""
    co = np.array(coeffs, np.int32)
    changed = to_white = total = 0
    for f in frames:
        out = oracle.stripes_apply(f, black, white, 1, co)
        changed += int((out != f).sum())
        to_white += int(((out == white) & (f != white)).sum())
        total += f.size
    return changed, to_white, total


@pytest.mark.parametrize("case", LC.LEVELS, ids=LC.level_id)
def test_level_case_stripes_change_pixels(oracle, case):
    """Family b at every level pair changes pixels -- except at the two blacks where no pixel lies more than 64 above black"""
    black, kind, _ = case
    w, h = LC.level_geometry(LC.LEVELS.index(case))
    changed, _, total = changed_by_stripes(oracle, LC.footage(LC.KINDS[2], w, h, black), black, LC.white_of(black, kind), LC.REALISTIC)
    if black in LC.SATURATED_BLACKS:
        assert changed == 0
    else:
        assert changed * 20 > total, (changed, total)


@pytest.mark.parametrize("case", LC.FAMILY_CASES, ids=LC.family_id)
def test_family_case_is_not_vacuous(oracle, case):
    name, black, white, form, quarters = case
    co = LC.FAMILIES[name]
    w, h = LC.family_geometry(LC.FAMILY_CASES.index(case))
    frames = LC.footage(LC.KINDS[2], w, h, black, quarters)
    for f in frames:
        assert (f == 16383).mean() < 0.10
        pop = LC.populations(f, black)
        assert all(pop[k] >= 4 for k, there in LC.room_for(black).items() if there), pop
    changed, to_white, total = changed_by_stripes(oracle, frames, black, white, co)
    if name[0] in "cde":
        assert changed * 20 > total, (changed, total)
    if name[0] == "e":
        assert white == LC.CLAMP_WHITE and to_white * 100 >= total, f"{to_white} of {total} pixels end at white"
    if name[0] == "d":
        # each d set on its own is outside the packed form, by exactly one coefficient, and by one step
        out = [c for c in co if not -32768 < c - LC.ONE < 32768]
        assert len(out) == 1 and out[0] in (LC.ONE + 32768, LC.ONE - 32768, 0)
        if 0 in co:                                  # stripes.c:261: the column of a zero coefficient is left alone, above white too
            ph = co.index(0)
            f = frames[0]
            assert (f[:, ph::8] > white).any() or white >= 16383
            assert np.array_equal(oracle.stripes_apply(f, black, white, 1, np.array(co, np.int32))[:, ph::8], f[:, ph::8])
    else:
        assert all(-32768 < c - LC.ONE < 32768 for c in co)


def test_coefficient_families():
    F = LC.FAMILIES
    assert set(F["a-unit"]) == {LC.ONE} and F["b-realistic"][:2] == (LC.ONE, LC.ONE)
    assert max(abs(c - LC.ONE) for c in F["b-realistic"]) == 332 and len(set(F["b-realistic"])) == 7      # 0.51 %
    assert LC.HI - LC.ONE == 32767 == LC.ONE - LC.LO
    assert F["c-edge-2to7"][:2] == (LC.ONE, LC.ONE) and set(F["c-edge-2to7"][2:]) == {LC.HI, LC.LO}
    assert set(F["c-edge-all"]) == {LC.HI, LC.LO} and F["c-edge-all"][0] != F["c-edge-all"][1]
    for name in LC.ONE_UNIT_FAMILIES:
        for a, b in zip(F[name][0::2], F[name][1::2]):           # the dwords (0,1) (2,3) (4,5) (6,7)
            assert (a == LC.ONE) != (b == LC.ONE) and {a, b} - {LC.ONE} <= {LC.HI, LC.LO}, (name, a, b)
    m = F["c-one-unit-mirror"]
    assert tuple(F["c-one-unit"]) == tuple(x for pair in zip(m[1::2], m[0::2]) for x in pair)
    assert {F[n][0] == LC.ONE for n in LC.ONE_UNIT_FAMILIES} == {True, False}
    assert set(F["e-gain-1.25"]) == {81920} and set(F["e-gain-edge"]) == {LC.HI}
    assert {b for _, b, _, _, _ in LC.FAMILY_CASES} == set(LC.FAMILY_BLACKS) == {0, 2047, 8191}
    assert {n for n, _, _, _, _ in LC.FAMILY_CASES} == set(F) - {"b-realistic"}


def test_streaming_kernels_admit_every_black_of_the_rule(amd, monkeypatch):
    """The plan of a long launch: with stripes in the packed form (and with none) k_frame_s takes cs2x2 / cs3x3 and k_frame_p5 cs5x5 at
    every black level 0 .. 16384; with the generic form neither ever does; at black -1 and 16385 neither does, whatever the stripes"""
    for v in ("MLVFS_AMD_KF_P", "MLVFS_AMD_KF_P5", "MLVFS_AMD_KF_S"):
        monkeypatch.delenv(v, raising=False)
    w, h = LC.GEOMETRIES[0]
    first = lambda cs, black, stripes: S.frame_plan(w, h, cs, LONG, 256, False, stripes, black=black)["first"]
    want = {2: S.P_S, 3: S.P_S, 5: S.P_P5}
    streaming = (S.P_S, S.P_P5)
    for black in range(0, 16385):
        for cs in (2, 3, 5):
            assert first(cs, black, 1) == want[cs], (cs, black)
    for black in (0, 1, 2047, 16384):
        for cs in (2, 3, 5):
            assert first(cs, black, 0) == want[cs], (cs, black)
    for black in list(range(0, 16385, 37)) + [16384]:
        for cs in (2, 3, 5):
            assert first(cs, black, 2) not in streaming, (cs, black)
    for black in (-1, 16385, -2048, 40000):
        for cs in (2, 3, 5):
            for stripes in (0, 1, 2):
                assert first(cs, black, stripes) not in streaming, (cs, black, stripes)
    assert S.frame_plan(w, h, 5, LONG, 256, True, 1, black=16384)["first"] == S.P_P5          # with a pixel map
    assert S.frame_plan(w, h, 2, LONG, 256, True, 1, black=0)["first"] == S.P_NONE            # k_frame_s takes none


def test_geometries_are_the_cuts_they_are_there_for(amd):
    (w1, h1), (w2, h2) = LC.GEOMETRIES
    s = S.shape(w1, h1, 30)
    assert (s["cols"], s["last_items"], s["fold"], s["segs"], s["vec"]) == (2, 14, 4, 5, 1)
    s = S.shape(w2, h2, 30)
    assert (s["cols"], s["vec"]) == (1, 2)
    for bpp, geoms in LC.REDUCED_GEOMETRIES.items():
        assert all(w % (8 if bpp == 12 else 16) == 0 for w, _ in geoms)
    assert any(w % 16 == 8 for w, _ in LC.REDUCED_GEOMETRIES[12])


@pytest.mark.parametrize("bpp,black,white", LC.REDUCED, ids=[f"{b}bit-black{k}-white{w}" for b, k, w in LC.REDUCED])
def test_reduced_depth_footage(oracle, bpp, black, white):
    top = (1 << bpp) - 1
    assert black + 64 < white <= top
    for w, h in LC.REDUCED_GEOMETRIES[bpp]:
        frames = LC.footage(LC.KINDS[5], w, h, black, bpp=bpp)
        for f in frames:
            assert int(f.max()) <= top
            pop, room = LC.populations(f, black), LC.room_for(black, top)
            assert all(pop[k] >= 4 for k, there in room.items() if there), pop
        changed, _, total = changed_by_stripes(oracle, frames, black, white, LC.REALISTIC)
        assert changed * 20 > total


def test_reduced_depth_levels():
    assert {(b, k) for b, k, _ in LC.REDUCED} == {(12, 0), (12, 511), (12, 512), (12, 1000), (10, 0), (10, 127), (10, 128), (10, 300)}
    assert {w for b, _, w in LC.REDUCED if b == 12} == {3750, 4095} and {w for b, _, w in LC.REDUCED if b == 10} == {937, 1023}


def test_16_bit_cases(oracle):
    w, h = LC.GEOMETRIES[0]
    assert (LC.UNPACKED_BLACK, LC.UNPACKED_WHITE) == (8192, 60000)
    for black, name in LC.UNPACKED_STRIPES:
        f = LC.full_range16(w, h, black, 5)
        assert int(f.max()) == 65535 and int(f.min()) == 0 and (f[1, 8:16] == 65535).all()
        changed, to_white, total = changed_by_stripes(oracle, [f], black, LC.UNPACKED_WHITE, LC.FAMILIES[name])
        assert changed * 20 > total and to_white > 0
    # the largest product of the 32-bit form: (65535 - 0) * 32767 is below 2^31, and the case that forms it is in the list
    assert (0, "e-gain-edge") in LC.UNPACKED_STRIPES and 65535 * (LC.HI - LC.ONE) < 1 << 31
    for cs in (2, 5):
        frames = LC.footage16(LC.KINDS[cs], w, h, LC.UNPACKED_BLACK)
        assert max(int(f.max()) for f in frames) > 16383, "beyond 14 bits"
        for f in frames:
            assert LC.UNPACKED_BLACK - 16384 <= int(f.min()) and int(f.max()) <= LC.UNPACKED_BLACK + 16383     # inside raw2ev (main.c:158-176)
            pop = LC.populations(f, LC.UNPACKED_BLACK)
            assert all(v >= 4 for v in pop.values()), pop


@pytest.mark.parametrize("black", LC.FAMILY_BLACKS)
@pytest.mark.parametrize("green,dim", LC.LONE_GREEN)
def test_lone_green_cells_smooth_to_within_64_of_black(oracle, black, green, dim):
    """No pixel of the input at most 64 above black (none less than 256 above, in the second variant), yet hundreds of smoothed
    pixels there, which stripes leave alone and which the unmasked formula p + ((p - black) * d >> 16) would change"""
    w, h = LC.GEOMETRIES[0]
    d = np.array(LC.REALISTIC, np.int64)[np.arange(w) % 8] - LC.ONE
    for cs in (2, 3, 5):
        f = LC.lone_green_frame(w, h, black, green, dim, 1)
        assert int(f.min()) - black >= dim > 64 and (dim < 256 or int(f.min()) - black >= 256) and int(f.max()) <= 16383
        sm = oracle.chroma_smooth(f, black, cs)
        low = (sm.astype(np.int64) <= black + 64) & (sm != f)
        assert low.sum() >= 500, int(low.sum())
        after = oracle.stripes_apply(sm, black, 16383, 1, np.array(LC.REALISTIC, np.int32))
        assert np.array_equal(after[low], sm[low])
        unmasked = sm.astype(np.int64) + (((sm.astype(np.int64) - black) * d) >> 16)
        assert (unmasked[low] != after[low]).sum() >= 200


def test_cache_levels_outnumber_the_cache():
    """csrc/k_frame.hip keeps 8 output tables per device (E2R_CACHE): 11 levels in turn, with a twelfth in use between them, evict"""
    assert len(set(LC.CACHE_LEVELS)) == 11 and LC.CACHE_NEIGHBOUR not in LC.CACHE_LEVELS
    assert all(0 <= b <= 16384 for b in LC.CACHE_LEVELS)
